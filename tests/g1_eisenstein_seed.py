"""The top two digits of the base-8 Eisenstein expansion, as g1_scalar_mul_eis (g1.hpp) seeds its accumulator from them: what is left of
k0 + k1 psi after 42 digits, scalars that reach every value of it, and a predictor of the complete-path lanes of the seeded schedule.
Plain integers on top of tests/g1_eisenstein.py; shared by the CPU, host-sim and GPU tests of the seed."""
import random

from g1_eisenstein import CHAIN_UNITS, CLASSES, DBL, DIGITS, INF, NONE, REPS, TABLE, edge_scalars, mul_unit, recode, split, value
from g1_torsion import X2
from util import R

LOW = DIGITS - 2                                             # position 42: the seed covers it and position 43
SUMS = {(3, 2): ((2, 2), (1, 0), (-5, 2)), (3, 3): ((2, 3), (0, 1), (3, -5))}      # t -> (table element s with t = s + 1, d_43, d_42)


def top_value(k):
    """t = 8 d_43 + d_42: k0 + k1 psi with its 42 lowest digits taken off and divided by 8^42"""
    return value(recode(*split(k))[LOW:])


def exact_digit(z):
    """(entry, unit) of the digit that IS z, or None when the digit of z's class is another element"""
    e, u, d = CLASSES[(z[0] & 7) + 8 * (z[1] & 7)]
    return (e, u) if d == z and e != NONE else None


def corner_scalars(n=400, seed=44101):
    """scalars next to k0 = x^2 - 1 with k1 = floor(r / x^2) = x^2 - 1 (r = x^4 - x^2 + 1: that k1 leaves k0 = 0 alone, so the corner is
    approached from k1 = x^2 - 2), where both coefficients of t reach 3"""
    rng = random.Random(seed)
    ks = [(X2 - 1) * X2, X2 - 1 + (X2 - 2) * X2, R - 1, R - 2]
    for _ in range(n):
        s0, s1 = rng.randrange(4, 126), rng.randrange(4, 126)
        ks.append(X2 - 1 - rng.randrange(1 << s0) + (X2 - 2 - rng.randrange(1 << s1)) * X2)
    assert all(0 <= k < R for k in ks)
    return ks


def occupied_scalars(each=10):
    """scalars whose position 43 is occupied: `each` with t = (3, 2), from anywhere, and `each` with t = (3, 3), which only the corner has"""
    rng = random.Random(44102)
    out = {t: [] for t in SUMS}
    for k in corner_scalars(4000) + [rng.randrange(R) for _ in range(4000)]:
        t = top_value(k)
        if t in out and len(out[t]) < each:
            out[t].append(k)
    assert all(len(v) == each for v in out.values()), {t: len(v) for t, v in out.items()}
    return out[(3, 2)] + out[(3, 3)]


def seed_scalars(n=20000, seed=44100):
    rng = random.Random(seed)
    return edge_scalars() + [rng.randrange(R) for _ in range(n)] + corner_scalars()


def one_scalar_per_top_value():
    """t -> a scalar with that top value, all sixteen: the first of seed_scalars() that reaches it"""
    out = {}
    for k in seed_scalars(3000):
        out.setdefault(top_value(k), k)
    assert sorted(out) == [(a, b) for a in range(4) for b in range(4)], sorted(out)
    return out


def exceptional_seeded(k, q, lam):
    """g1_eisenstein.exceptional for the schedule that seeds the accumulator from the top two digits: the table's chain as there; with
    position 43 empty the highest digit starts the accumulator as before; with position 43 occupied the accumulator starts as s + 1 (SUMS),
    exceptional (Z = 0) when s = 1 (DBL) or s = -1 (INF) on the point; then the digits below position 42 as before."""
    if lam is None:
        red = lambda z: (z[0] % q, z[1] % q)
    else:
        red = lambda z: (z[0] + z[1] * lam) % q
    digs = recode(*split(k))
    if not digs:
        return None
    for i, u in enumerate(CHAIN_UNITS):
        for s in (1, -1):
            if red(REPS[i]) == red(mul_unit((s, 0), u)):
                return TABLE
    acc, inf = (0, 0), True
    if len(digs) == DIGITS:
        t = value(digs[LOW:])
        s, top, low = SUMS[t]
        assert (digs[LOW + 1][2], digs[LOW][2]) == (top, low)
        if red(s) == red((1, 0)):
            return DBL
        if red(s) == red((-1, 0)):
            return INF
        acc, inf = t, False
        digs = digs[:LOW]
    for e, u, d in reversed(digs):
        acc = (8 * acc[0], 8 * acc[1])
        if e == NONE:
            continue
        if inf:
            acc, inf = d, False
            continue
        if red(acc) == red(d):
            return DBL
        if red(acc) == red((-d[0], -d[1])):
            return INF
        acc = (acc[0] + d[0], acc[1] + d[1])
    return None
