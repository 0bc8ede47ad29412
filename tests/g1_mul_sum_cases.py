"""Inputs of the per-lane sum of k G1 products (c12381_g1_mul_sum_batch, g1.hpp g1_scalar_mul_sum), shared by the host-sim and the GPU
tests: seeded subgroup lanes, edge scalars crossed with special points in every term position, and lanes built from RELATED points.
A lane is a list of k (96-byte point, integer scalar) terms; pack() lays lanes out argument-major as the entry point takes them.
Every input is computed on the CPU (g1_torsion.py, the oracle), never taken from the code under test."""
from g1_torsion import X2, ec_add, ec_mul, ec_neg, edge_scalars, eigenpoint, enc, generator, point_of_order
from util import R, golden, prng, scalars

INF = bytes(96)


def b32(k):
    return (k % (1 << 256)).to_bytes(32, "big")


def pack(lanes, k):
    """lanes of k terms -> (pts, scalars), arrays of k * n records with term j of lane i at record j * n + i"""
    assert all(len(ln) == k for ln in lanes)
    return (b"".join(ln[j][0] for j in range(k) for ln in lanes), b"".join(b32(ln[j][1]) for j in range(k) for ln in lanes))


def expected(orc, pts, sc, k, fmt=96, nthreads=8):
    """the pinned value: the oracle's multiply on every term, then its add, term by term"""
    n = len(sc) // (32 * k)
    cols = [orc.g1_mul(pts[96 * n * j:96 * n * (j + 1)], sc[32 * n * j:32 * n * (j + 1)], fmt if k == 1 else 96, nthreads) for j in range(k)]
    acc = cols[0]
    for j in range(1, k):
        acc = orc.g1_add(acc, cols[j], fmt if j == k - 1 else 96)
    return acc


def subgroup_pool(orc, seed, m):
    g = enc(generator())
    pts = orc.g1_mul(g * m, scalars(seed, m), 96, 8)
    return [pts[96 * i:96 * i + 96] for i in range(m)]


def seeded_lanes(orc, k, n, seed):
    """n lanes of k independent random subgroup points with random scalars below 2^256"""
    pool = subgroup_pool(orc, seed, k * n)
    return [[(pool[j * n + i], prng(seed + 1, j * n + i) % (1 << 256)) for j in range(k)] for i in range(n)]


def special_points():
    """(name, point): subgroup, infinity, order 3, order 11, G + T3 (order 3r), two off-subgroup points of the golden file, two eigenpoints"""
    g = generator()
    out = [("gen", enc(g)), ("sub", enc(ec_mul(prng(9601, 0) % R, g))), ("inf", INF), ("o3", enc((0, 2))), ("o11", enc(point_of_order(11))),
           ("g+t3", enc(ec_add(g, (0, 2))))]
    out += [("off%d" % i, bytes.fromhex(h)) for i, h in enumerate(golden("g1")["offsubgroup_points"][:2])]
    out += [("eig%d" % q, enc(eigenpoint(q)[0])) for q in (10177, 859267)]
    return out


def edge_lanes(orc, k, seed=9610):
    """every special point with every edge scalar in every term position; the other terms are random subgroup terms, or (every third
    lane) the same special point with another edge scalar.  Returns (lanes, tags)"""
    pool = subgroup_pool(orc, seed, 64)
    ks = edge_scalars()
    lanes, tags = [], []
    c = 0
    for name, pt in special_points():
        for si, s in enumerate(ks):
            for pos in range(k):
                ln = []
                for j in range(k):
                    if j == pos:
                        ln.append((pt, s))
                    elif c % 3 == 2:
                        ln.append((pt, ks[(si + 7 * (j + 1)) % len(ks)]))
                    else:
                        ln.append((pool[(c + 5 * j) % 64], prng(seed + 2, 4 * c + j) % (1 << 256)))
                lanes.append(ln)
                tags.append((name, s, pos))
                c += 1
    return lanes, tags


def related_lanes(orc, k, seed=9620, reps=6):
    """lanes whose terms are related: Q = P, Q = -P, Q = 2P, Q = phi(P), products that cancel to infinity, all terms at infinity, all
    scalars 0.  Terms beyond the second are infinity, a zero scalar, or (kind ends in '+') random subgroup terms.
    Returns (lanes, kinds); kinds starting with 'cancel' have the point at infinity as their result although a term is not trivial."""
    g = generator()
    pool = subgroup_pool(orc, seed, 16)
    lanes, kinds = [], []

    def rest(i, mode):
        out = []
        for j in range(2, k):
            if mode == "+":
                out.append((pool[(i + j) % 16], prng(seed + 3, 8 * i + j) % (1 << 256)))
            elif (i + j) % 2:
                out.append((INF, prng(seed + 4, 8 * i + j) % (1 << 256)))
            else:
                out.append((pool[(i + j) % 16], R if i % 3 else 0))
        return out

    for i in range(reps):
        a = prng(seed + 5, i) % R
        p = ec_mul(prng(seed + 6, i) % R or 1, g)
        x, y = prng(seed + 7, i) % (1 << 256), prng(seed + 8, i) % (1 << 256)
        phi_p = ec_mul((-X2) % R, p)                             # phi(P) = (beta x, y) = -E(P) = [-x^2]P on G1
        two_p = ec_add(p, p)
        base = [("Q=P", [(enc(p), x), (enc(p), y)]),
                ("Q=P equal scalars", [(enc(p), x), (enc(p), x)]),
                ("Q=-P", [(enc(p), x), (enc(ec_neg(p)), y)]),
                ("Q=2P", [(enc(p), x), (enc(two_p), y)]),
                ("Q=phi(P)", [(enc(p), x), (enc(phi_p), y)]),
                ("cancel Q=-P equal scalars", [(enc(p), a), (enc(ec_neg(p)), a)]),
                ("cancel xP+(r-x)P", [(enc(p), a), (enc(p), R - a)]),
                ("cancel Q=2P", [(enc(p), (2 * a) % R), (enc(two_p), R - a)]),
                ("cancel Q=phi(P)", [(enc(p), X2 % R), (enc(phi_p), 1)]),
                ("all infinity", [(INF, x), (INF, y)]),
                ("all scalars 0", [(enc(p), 0), (enc(two_p), R)])]
        for kind, two in base:
            if k == 1:
                continue
            lanes.append(two + rest(i, ""))
            kinds.append(kind)
            if k > 2 and not kind.startswith(("cancel", "all")):
                lanes.append(two + rest(i, "+"))
                kinds.append(kind + "+")
    return lanes, kinds
