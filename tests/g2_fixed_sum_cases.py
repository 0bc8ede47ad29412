"""Inputs of the per-lane sum over shared G2 bases (c12381_g2_mul_fixed_sum_batch, fixed_base.hpp g2_fixed_eval_sum), shared by the host-sim
and the GPU tests: a seeded pool of G2 bases, edge scalars in every base position, RELATED bases with lanes that cancel to infinity, addends,
bases that no table serves and a point off the twist.  A case is (bases, scalars, addend): nb points of 192 bytes, nb base-major arrays of
n 32-byte scalars, one 192-byte point or None.  Every input is computed on the CPU (g2_twist.py, the oracle, golden points), never taken from
the code under test."""
import functools

from g2_twist import X, dec192, ec_add, ec_mul, ec_neg, enc192, g2_edge_scalars, generator, on_curve, twist_points
from util import R, golden, prng, scalars

INF = bytes(192)
G2GEN = bytes.fromhex(golden("g2")["generator"])
OFF_TWIST = G2GEN[:191] + bytes([G2GEN[191] ^ 1])          # the generator with another y: on no curve point
assert not on_curve(dec192(OFF_TWIST))
POOL_SEED = 9700
_POOLS = {}


@functools.lru_cache(maxsize=None)
def _twist():
    return twist_points()


def b32(k):
    return (k % (1 << 256)).to_bytes(32, "big")


def subgroup_pool(orc, seed, m):
    """m elements of G2: seeded multiples of the generator (the oracle's multiply), computed once per (seed, m)"""
    if (seed, m) not in _POOLS:
        pts = orc.g2_mul(G2GEN * m, scalars(seed, m), 192, 8)
        _POOLS[(seed, m)] = [pts[192 * i:192 * i + 192] for i in range(m)]
    return _POOLS[(seed, m)]


def edge_scalars():
    """g2_edge_scalars(); 0, r, r + 1 and 2^256 - 1 have to be among them"""
    ks = list(g2_edge_scalars())
    for k in (0, R, R + 1, (1 << 256) - 1):
        if k not in ks:
            ks.append(k)
    return ks


def expected(orc, bases, sc, addend=None, fmt=192):
    """the pinned value: the oracle's multiply per column (the base replicated n times), then its add column by column, the addend last"""
    nb = len(bases) // 192
    n = len(sc) // (32 * nb)
    last = nb - 1 if addend is None else nb
    acc = None
    for i in range(nb):
        col = orc.g2_mul(bases[192 * i:192 * i + 192] * n, sc[32 * n * i:32 * n * (i + 1)], fmt if last == 0 else 192, 8)
        acc = col if i == 0 else orc.g2_add(acc, col, fmt if i == last else 192)
    return acc if addend is None else orc.g2_add(acc, addend * n, fmt)


def neg(pt192):
    return enc192(ec_neg(dec192(pt192)))


def columns(cols):
    """nb lists of n integers -> the base-major scalar array"""
    return b"".join(b32(k) for col in cols for k in col)


def random_columns(seed, nb, n):
    return [[prng(seed, i * n + j) % (1 << 256) for j in range(n)] for i in range(nb)]


def seeded(orc, nb, n, seed, pool_seed=POOL_SEED):
    """nb elements of G2 (always the first nb of one pool of 32, so tables are shared between cases) with n lanes of random scalars below 2^256"""
    pool = subgroup_pool(orc, pool_seed, 32)
    return b"".join(pool[:nb]), columns(random_columns(seed, nb, n))


def edge_case(orc, nb, pos, seed=9710, pool_seed=POOL_SEED):
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


@functools.lru_cache(maxsize=None)
def _related_points(seed):
    g = generator()
    h = ec_mul(prng(seed, 0) % R or 1, g)
    return h, ec_neg(h), ec_add(h, h), ec_mul((-X) % R, h)         # psi(H) = [x]H = [-|x|]H on G2


def related_cases(orc, nb, seed=9720, reps=5):
    """(kind, bases, scalars, cancel_lanes): H2 = H1, -H1, 2 H1, psi(H1) with lanes of random scalars and lanes whose sum is the point at
    infinity although no term is trivial (a and r - a on one base; a on H and a on -H; 2a on H with r - a on 2H; t |x| on H with t on psi(H)).
    Bases beyond the second are elements of G2; in the cancelling lanes their scalars are 0 or r."""
    h, neg_h, two_h, psi_h = _related_points(seed)
    extra = subgroup_pool(orc, seed + 1, 4)[:nb - 2]
    kinds = [("H2=H1", h, lambda a: (a, R - a)),
             ("H2=-H1", neg_h, lambda a: (a, a)),
             ("H2=2H1", two_h, lambda a: (2 * a % R, R - a)),
             ("H2=psi(H1)", psi_h, lambda a: (a * X % R, a))]
    out = []
    for kind, h2, cancel in kinds:
        cols = random_columns(seed + 2, nb, 2 * reps)
        lanes = list(range(1, 2 * reps, 2))
        for t, j in enumerate(lanes):
            a = 1 if t == 0 else prng(seed + 3, t) % R
            cols[0][j], cols[1][j] = cancel(a)
            assert cols[0][j] % R and cols[1][j] % R                # no term is trivial
            for i in range(2, nb):
                cols[i][j] = R if (i + t) % 2 else 0
        out.append((kind, enc192(h) + enc192(h2) + b"".join(extra), columns(cols), lanes))
    return out


def addends(orc, bases, sc):
    """(name, addend): absent, infinity, an element of G2, the negative of lane 0's sum (lane 0 becomes infinity), a twist point of order 13"""
    first = expected(orc, bases, sc)[:192]
    assert first != INF
    return [("none", None), ("inf", INF), ("sub", subgroup_pool(orc, 9730, 1)[0]), ("-sum0", neg(first)), ("t13", enc192(_twist()["t13a"]))]


@functools.lru_cache(maxsize=None)
def special_bases():
    """(name, point): bases that no table serves — a twist point of order 13, G + T13 (order 13 r), infinity"""
    p = _twist()
    return (("t13a", enc192(p["t13a"])), ("g+t13", enc192(p["g+t13"])), ("inf", INF))


def generic_case(orc, nb, pos, special, seed=9740, pool_seed=POOL_SEED):
    """`special` at base position pos among elements of G2; its column holds edge_scalars() (zero odd GS digits owe the [r]psi^i(Q) terms)"""
    bases, sc = edge_case(orc, nb, pos, seed, pool_seed)
    return bases[:192 * pos] + special + bases[192 * (pos + 1):], sc
