"""Python reference of the base-8 Eisenstein digit set of g1_scalar_mul_eis (g1.hpp) and a predictor of the lanes its incomplete formulas
cannot serve.  Plain integers; shared by the CPU, host-sim and GPU tests of that path.

The endomorphism psi(x, y) = (beta x, -y) = [x^2] satisfies psi^2 - psi + 1 = 0, so k0 + k1 psi is an Eisenstein integer a + b psi,
written here as the pair (a, b).  Its norm is a^2 + a b + b^2, the six units are psi^j, and psi (a, b) = (-b, a + b).  A digit is
unit x representative: psi^u REPS[e], one of the 63 non-zero classes mod 8, or nothing (the class of 0)."""
import random

from g1_torsion import X2
from util import R

# each representative is the previous one plus a unit (CHAIN_UNITS): the table is one co-Z chain
REPS = [(1, 0), (2, -1), (2, -2), (2, -3), (1, -3), (0, -3), (1, -4), (2, -4), (3, -5), (3, -4), (4, -4)]
UNITS = [(1, 0), (0, 1), (-1, 1), (-1, 0), (0, -1), (1, -1)]                   # psi^0 .. psi^5
DIGITS = 44                                                                    # digits per scalar (proof: digit_bound)
NONE = 15                                                                      # the entry field of the digit of class 0


def mul_psi(z):
    return -z[1], z[0] + z[1]


def mul_unit(z, u):
    for _ in range(u % 6):
        z = mul_psi(z)
    return z


def norm(z):
    return z[0] * z[0] + z[0] * z[1] + z[1] * z[1]


CHAIN_UNITS = [UNITS.index((REPS[i + 1][0] - REPS[i][0], REPS[i + 1][1] - REPS[i][1])) for i in range(len(REPS) - 1)]


def class_table():
    """index (a mod 8) + 8 (b mod 8) -> (entry, unit, (da, db)); the class of 0 -> (NONE, 0, (0, 0)).  The three classes of the orbit of
    4 are reached by two units each: the smaller one is kept."""
    t = [None] * 64
    t[0] = (NONE, 0, (0, 0))
    for e, rep in enumerate(REPS):
        for u in range(6):
            d = mul_unit(rep, u)
            c = (d[0] & 7) + 8 * (d[1] & 7)
            if t[c] is None:
                t[c] = (e, u, d)
    return t


CLASSES = class_table()


def code(entry, unit):
    """the 7-bit form of a digit: entry in bits 0..3 (NONE for no addition), unit in bits 4..6"""
    return entry | (unit << 4)


def recode(a, b, limit=None):
    """digits of a + b psi, lowest first, as (entry, unit, d): d = rep(k mod 8), k <- (k - d) / 8, until k = 0.  Both coefficients of every
    digit lie in [-5, 5], so a non-negative coefficient stays one: (c - dc) / 8 = (c >> 3) + (dc < 0)."""
    out = []
    while (a, b) != (0, 0):
        e, u, d = CLASSES[(a & 7) + 8 * (b & 7)]
        out.append((e, u, d))
        assert (a - d[0]) % 8 == 0 and (b - d[1]) % 8 == 0
        a, b = (a - d[0]) // 8, (b - d[1]) // 8
        if limit is not None and len(out) > limit:
            raise AssertionError("recoding does not end")
    return out


def value(digs):
    a = b = 0
    for e, u, d in reversed(digs):
        a, b = 8 * a + d[0], 8 * b + d[1]
    return a, b


def packed(a, b):
    """the ten dwords g1.hpp keeps: digit w (of DIGITS, padded with NONE digits) in bits 7 (DIGITS - 1 - w) ..., the top digit lowest"""
    digs = recode(a, b)
    assert len(digs) <= DIGITS
    codes = [code(e, u) for e, u, _ in digs] + [code(NONE, 0)] * (DIGITS - len(digs))
    v = 0
    for w, c in enumerate(codes):
        v |= c << (7 * (DIGITS - 1 - w))
    return [(v >> (32 * i)) & 0xffffffff for i in range(10)]


def split(k):
    k %= R
    k1, k0 = divmod(k, X2)
    return k0, k1


def digit_bound():
    """|k_(n+1)| <= (|k_n| + max|d|) / 8, so |k_n| <= |k| / 8^n + max|d| / 7.  |k|^2 = k0^2 + k0 k1 + k1^2 < 3 * 2^256 for k0, k1 < 2^128;
    the smallest n with (|k| / 8^n + max|d| / 7)^2 < 3 leaves norm 0 or 1 (no Eisenstein integer has norm 2): k_n is 0 or a unit, which
    is its own digit, so n + 1 digits suffice."""
    import math
    dmax = math.sqrt(max(norm(r) for r in REPS))
    kmax = math.sqrt(3.0) * 2.0 ** 128
    n = 0
    while (kmax / 8.0 ** n + dmax / 7) ** 2 >= 3:
        n += 1
    return n + 1


# ---------------------------------------------------------------- scalars the tests of the path share
def edge_scalars():
    """the edge scalars, one scalar per class mod 8 in the lowest digit, the highest digits a seeded search reaches, and scalars whose
    digits are all zero above the first"""
    ks = [0, 1, R - 1, R, (1 << 256) - 1, X2 - 1, X2, X2 + 1, R + 1, 2, 8, R - X2]
    rng = random.Random(44003)
    for c in range(64):                                        # k0 = a, k1 = b mod 8
        ks.append((c & 7) + 8 * rng.randrange(X2 // 8 - 1) + X2 * ((c >> 3) + 8 * rng.randrange(1 << 120)))
    tops = {}
    cands = [rng.randrange(R) for _ in range(3000)] + [R - 1 - rng.randrange(1 << 20) for _ in range(200)]
    cands += [X2 * ((1 << 128) - 1 - rng.randrange(1 << 10)) % R for _ in range(200)] + [rng.randrange(1 << s) for s in range(1, 256, 3)]
    for k in cands:
        digs = recode(*split(k))
        if digs:
            tops.setdefault((len(digs), digs[-1][0], digs[-1][1]), k)
    assert any(n == DIGITS for n, _, _ in tops) and len(tops) >= 12, sorted(tops)
    ks += list(tops.values())
    for c in range(1, 64):                                     # the scalar IS one digit: every digit above the first is zero
        e, u, d = CLASSES[c]
        if d[0] >= 0 and d[1] >= 0:
            ks.append(d[0] + d[1] * X2)
    ks += [8 ** 10, X2 * 8 ** 7, 8 ** 42]                      # one non-zero digit far up, zeros below
    return ks



# ---------------------------------------------------------------- which lanes the incomplete formulas cannot serve
DBL, INF, TABLE = "s=t", "s=-t", "table"


def exceptional(k, q, lam):
    """The first exceptional step of g1_scalar_mul_eis on a point P of order q, or None.  lam = the residue mod q as which psi acts on P (a
    subgroup point: (R, x^2); the order-3 points: (3, 2); an eigenpoint of g1_torsion.eigenpoint(q): (q, lambda)), or None for a point of
    E(Fp)[q] = Z_q x Z_q with q inert (q = 2 mod 3, e.g. 11), whose multiples by Z[psi] form the field Z[psi] / q.
    The table's chain adds psi^u P to entry i: exceptional (TABLE) when entry i = +-psi^u P.  In the loop the accumulator's multiple s is
    tracked: adding t P to an accumulator not at infinity is exceptional when s = t (DBL) or s = -t (INF).  Either leaves Jacobian Z = 0.
    A scalar that is 0 mod R has no digit: the result is infinity without a look at the table."""
    if lam is None:
        red = lambda z: (z[0] % q, z[1] % q)
    else:
        red = lambda z: (z[0] + z[1] * lam) % q
    k0, k1 = split(k)
    digs = recode(k0, k1)
    if not digs:
        return None
    for i, u in enumerate(CHAIN_UNITS):
        for s in (1, -1):
            if red(REPS[i]) == red(mul_unit((s, 0), u)):
                return TABLE
    acc, inf = (0, 0), True
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
