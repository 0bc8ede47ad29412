"""Inputs of the per-lane sum over shared G1 bases (c12381_g1_mul_fixed_sum_batch, fixed_base.hpp g1_fixed_eval_sum), shared by the host-sim
and the GPU tests: seeded subgroup bases, edge scalars in every base position, RELATED bases with lanes that cancel to infinity, addends,
and bases that are no subgroup points.  A case is (bases, scalars, addend): nb points of 96 bytes, nb base-major arrays of n 32-byte
scalars, one 96-byte point or None.  Every input is computed on the CPU (g1_torsion.py, the oracle, golden points), never taken from the
code under test."""
from g1_mul_sum_cases import INF, b32, subgroup_pool
from g1_mul_sum_cases import expected as mul_sum_expected
from g1_torsion import X2, dec, ec_add, ec_mul, ec_neg, edge_scalars, enc, generator
from util import R, golden, prng

O3 = enc((0, 2))                                   # the point of order 3
OFF_CURVE = (1).to_bytes(48, "big") + (1).to_bytes(48, "big")


def expected(orc, bases, sc, addend=None, fmt=96):
    """the pinned value: the oracle's multiply per column (the base replicated n times), then its add column by column, the addend last"""
    nb = len(bases) // 96
    n = len(sc) // (32 * nb)
    pts = b"".join(bases[96 * i:96 * i + 96] * n for i in range(nb))
    acc = mul_sum_expected(orc, pts, sc, nb, fmt if addend is None else 96)
    return acc if addend is None else orc.g1_add(acc, addend * n, fmt)


def neg(pt96):
    return enc(ec_neg(dec(pt96)))


def columns(cols):
    """nb lists of n integers -> the base-major scalar array"""
    return b"".join(b32(k) for col in cols for k in col)


def random_columns(seed, nb, n):
    return [[prng(seed, i * n + j) % (1 << 256) for j in range(n)] for i in range(nb)]


def seeded(orc, nb, n, seed, pool_seed=9800):
    """nb subgroup bases (always the first nb of one pool, so tables are shared between cases) with n lanes of random scalars below 2^256"""
    pool = subgroup_pool(orc, pool_seed, 32)
    return b"".join(pool[:nb]), columns(random_columns(seed, nb, n))


def edge_case(orc, nb, pos, seed=9810, pool_seed=9800):
    """edge_scalars() at base position pos, random scalars (every third lane: other edge scalars) elsewhere"""
    ks = edge_scalars()
    n = len(ks)
    cols = random_columns(seed + pos, nb, n)
    for i in range(nb):
        for j in range(n):
            if i == pos:
                cols[i][j] = ks[j]
            elif j % 3 == 2:
                cols[i][j] = ks[(j + 7 * (i + 1)) % n]
    pool = subgroup_pool(orc, pool_seed, 32)
    return b"".join(pool[:nb]), columns(cols)


def related_cases(orc, nb, seed=9820, reps=5):
    """(kind, bases, scalars, cancel_lanes): H2 = H1, -H1, 2 H1, phi(H1) with lanes of random scalars and lanes whose sum is the point at
    infinity although no term is trivial (a and r - a on one base; a on H and a on -H; 2a on H with r - a on 2H; t x^2 on H with t on phi(H)).
    Bases beyond the second are subgroup points; in the cancelling lanes their scalars are 0 or r."""
    g = generator()
    h = ec_mul(prng(seed, 0) % R or 1, g)
    extra = subgroup_pool(orc, seed + 1, 4)[:nb - 2]
    phi_h = ec_mul((-X2) % R, h)                    # phi(H) = (beta x, y) = [-x^2]H on G1
    kinds = [("H2=H1", h, lambda a: (a, R - a)),
             ("H2=-H1", ec_neg(h), lambda a: (a, a)),
             ("H2=2H1", ec_add(h, h), lambda a: (2 * a % R, R - a)),
             ("H2=phi(H1)", phi_h, lambda a: (a * X2 % R, a))]
    out = []
    for kind, h2, cancel in kinds:
        cols = random_columns(seed + 2, nb, 2 * reps)
        lanes = list(range(1, 2 * reps, 2))
        for t, j in enumerate(lanes):
            a = 1 if t == 0 else prng(seed + 3, t) % R
            cols[0][j], cols[1][j] = cancel(a)
            for i in range(2, nb):
                cols[i][j] = R if (i + t) % 2 else 0
        out.append((kind, enc(h) + enc(h2) + b"".join(extra), columns(cols), lanes))
    return out


def addends(orc, bases, sc):
    """(name, addend): absent, infinity, a subgroup point, the negative of lane 0's sum (lane 0 becomes infinity), the point of order 3"""
    first = expected(orc, bases, sc)[:96]
    assert first != INF
    return [("none", None), ("inf", INF), ("sub", subgroup_pool(orc, 9830, 1)[0]), ("-sum0", neg(first)), ("o3", O3)]


def special_bases():
    """(name, point): bases that no table serves — a golden off-subgroup point, G + T3 (order 3r), the point of order 3, infinity"""
    g = generator()
    return [("off", bytes.fromhex(golden("g1")["offsubgroup_points"][0])), ("g+t3", enc(ec_add(g, (0, 2)))), ("o3", O3), ("inf", INF)]


def generic_case(orc, nb, pos, special, seed=9840, pool_seed=9800):
    """`special` at base position pos among subgroup bases; its column holds edge_scalars() (those below x^2 owe the [r]phi(P) term)"""
    bases, sc = edge_case(orc, nb, pos, seed, pool_seed)
    return bases[:96 * pos] + special + bases[96 * (pos + 1):], sc
