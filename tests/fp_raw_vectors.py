"""Vectors and expected values for the raw-limb tests of the Fp / Fp2 leaf (test_host_sim_fp_raw.py, test_gpu_fp_raw.py).

An Fp element is 14 signed 28-bit limbs carried lazily (csrc/fp.hpp).  The vectors sit AT the bounds the routines document, not near
them: limbs 0..12 at +-L(T) = floor(sqrt((2^63 - 14 2^56 - 2^40) / (14 T))) for a form of T products (balanced, and unbalanced pairs
with LBa = 2^31 - 1), top limbs that put sum VBa VBb at the checker's cap 10^6, at 2^11 and at 1, borrow chains, and many
representations of k p + e for the predicates.  Every vector is checked against its routine's precondition with its real limbs
and its real value (assertions, nothing is filtered); COUNTS pins the number of vectors per op.

The two-lane form of Fp2 (csrc/fp2h.hpp, ops FH2_*: half an element per lane on the device, both halves in one object on the host) is packed
like the whole-element ops FP2_* and shares their expected values — the Fp2 formula, never the lane routine's U / V selection or its
(a + b)(a - b) — and their vectors wherever the preconditions agree; where they do not (FH2_SQR) the limit is derived from the lane
routine's own column inequality, in the comment above the generator (vectors()).

Expected values are plain integer mathematics, not a transliteration of the column scan: a Montgomery reduction of the integer
F = sum +-A_t B_t + R sum k_j C_j returns (F + ((-F / p) mod R) p) / R, written with limbs 0..12 in [0, 2^28) and a signed top limb."""
import random
from math import isqrt

from util import P

NL, LB = 14, 28
M28 = (1 << LB) - 1
RM = 1 << (NL * LB)
RINV = pow(RM, -1, P)
PINV = pow(P, -1, RM)
R2 = RM * RM % P
T31 = (1 << 31) - 1
TOPW = 1 << (LB * (NL - 1))              # weight of the top limb, 2^364
CAP = 10 ** 6                            # the checker's cap on sum VBa VBb
INJ_ROOM = 1 << 37                       # column room the injected forms keep for their addends

OPS = dict(MUL=0, SQR=1, MUL2_ADD=2, MUL2_SUB=3, RED1=4, RED2=5, RED3=6, RED4=7, REDS1=8, REDS2=9, REDS3=10, REDS4=11, INJ=12, INJ_CONST=13,
           SQR_INJ_CONST=14, INJ_LIT=15, QUOT_TOP=16, NORM1=17, NORM1_DBL=18, MUL_SMALL=19, WEAK_REDUCE=20, LINCOMB3P=21, CANON=22, IS_ZERO=23,
           EQUAL=24, SIGN=25, TO_WORDS=26, INV=27, ADD=28, SUB=29, NEG=30, FP2_MUL=32, FP2_SQR=33, FP2_MUL2_ADD=34, FP2_MUL2_SUB=35,
           FP2_MUL_INJ=36, FP2_MUL_IP=37, FP2_IS_ZERO=38, FP2_INV=39, FP2_SIGN=40, SQR2=41, MUL_MSQR2=42, FP2_CONJ=43, FP2_CONJ_MUL_CI=44,
           FP2_CONJ_MUL_NEG_I=45, FP2_CONJ_MUL_A1MI=46, FP2_MUL_FP=47, FP2_NORM1_DBL=48,
           FH2_ADD=64, FH2_SUB=65, FH2_NEG=66, FH2_DBL=67, FH2_NORM1=68, FH2_MUL_SMALL=69, FH2_SELECT=70, FH2_CONJ=71, FH2_MUL_IP=72, FH2_IS_ZERO=73,
           FH2_MUL=74, FH2_SQR=75, FH2_MUL2_ADD=76, FH2_MUL2_SUB=77, FH2_MUL_FP=78, FH2_CONJ_MUL_CI=79, FH2_CONJ_MUL_NEG_I=80, FH2_CONJ_MUL_A1MI=81,
           FH2_ONE=82)
ARITY = dict(MUL=2, SQR=1, MUL2_ADD=4, MUL2_SUB=4, RED1=2, RED2=4, RED3=6, RED4=8, REDS1=2, REDS2=4, REDS3=6, REDS4=8, INJ=4, INJ_CONST=4,
             SQR_INJ_CONST=3, INJ_LIT=4, QUOT_TOP=0, NORM1=1, NORM1_DBL=1, MUL_SMALL=1, WEAK_REDUCE=1, LINCOMB3P=3, CANON=1, IS_ZERO=1, EQUAL=2,
             SIGN=1, TO_WORDS=1, INV=1, ADD=2, SUB=2, NEG=1, FP2_MUL=4, FP2_SQR=2, FP2_MUL2_ADD=8, FP2_MUL2_SUB=8, FP2_MUL_INJ=6, FP2_MUL_IP=2,
             FP2_IS_ZERO=2, FP2_INV=2, FP2_SIGN=2, SQR2=1, MUL_MSQR2=3, FP2_CONJ=2, FP2_CONJ_MUL_CI=3, FP2_CONJ_MUL_NEG_I=2, FP2_CONJ_MUL_A1MI=3,
             FP2_MUL_FP=3, FP2_NORM1_DBL=2,
             FH2_ADD=4, FH2_SUB=4, FH2_NEG=2, FH2_DBL=2, FH2_NORM1=2, FH2_MUL_SMALL=2, FH2_SELECT=4, FH2_CONJ=2, FH2_MUL_IP=2, FH2_IS_ZERO=2, FH2_MUL=4,
             FH2_SQR=2, FH2_MUL2_ADD=8, FH2_MUL2_SUB=8, FH2_MUL_FP=3, FH2_CONJ_MUL_CI=3, FH2_CONJ_MUL_NEG_I=2, FH2_CONJ_MUL_A1MI=3, FH2_ONE=0)
# the two-lane ops always return two elements: both halves, or for the predicate FH2_IS_ZERO the flag of each of the two lanes
OUTPUTS = {name: 2 if name in ("FP2_MUL", "FP2_SQR", "FP2_MUL2_ADD", "FP2_MUL2_SUB", "FP2_MUL_INJ", "FP2_MUL_IP", "FP2_INV", "FP2_CONJ", "FP2_CONJ_MUL_CI",
                               "FP2_CONJ_MUL_NEG_I", "FP2_CONJ_MUL_A1MI", "FP2_MUL_FP", "FP2_NORM1_DBL") or name[:4] == "FH2_" else 1 for name in OPS}
FAMILIES = {
    "product + reduction": ["MUL", "SQR", "MUL2_ADD", "MUL2_SUB", "RED1", "RED2", "RED3", "RED4", "REDS1", "REDS2", "REDS3", "REDS4"],
    "injected reductions": ["INJ", "INJ_CONST", "SQR_INJ_CONST", "INJ_LIT", "QUOT_TOP"],
    "exact carries": ["NORM1", "NORM1_DBL", "MUL_SMALL", "WEAK_REDUCE", "LINCOMB3P"],
    "canonical form and predicates": ["CANON", "IS_ZERO", "EQUAL", "SIGN", "TO_WORDS", "INV"],
    "Fp2": ["FP2_MUL", "FP2_SQR", "FP2_MUL2_ADD", "FP2_MUL2_SUB", "FP2_MUL_INJ", "FP2_MUL_IP", "FP2_IS_ZERO", "FP2_INV", "FP2_SIGN"],
    "doubling and psi forms": ["SQR2", "MUL_MSQR2", "FP2_CONJ", "FP2_CONJ_MUL_CI", "FP2_CONJ_MUL_NEG_I", "FP2_CONJ_MUL_A1MI", "FP2_MUL_FP", "FP2_NORM1_DBL"],
    # csrc/fp2h.hpp: half an element per lane on the device (fp2h_raw_kernel), both halves in one object on the host
    "Fp2, two lanes": ["FH2_ADD", "FH2_SUB", "FH2_NEG", "FH2_DBL", "FH2_NORM1", "FH2_MUL_SMALL", "FH2_SELECT", "FH2_CONJ", "FH2_MUL_IP", "FH2_IS_ZERO", "FH2_MUL",
                       "FH2_SQR", "FH2_MUL2_ADD", "FH2_MUL2_SUB", "FH2_MUL_FP", "FH2_CONJ_MUL_CI", "FH2_CONJ_MUL_NEG_I", "FH2_CONJ_MUL_A1MI", "FH2_ONE"],
}
# vectors per op (asserted after generation; every one of them is run, on the host and on the device)
COUNTS = dict(MUL=2624, SQR=263, MUL2_ADD=1748, MUL2_SUB=1748, RED1=1748, RED2=1748, RED3=1748, RED4=1748, REDS1=1748, REDS2=1748, REDS3=1748,
              REDS4=1748, INJ=1748, INJ_CONST=1748, SQR_INJ_CONST=263, INJ_LIT=1748, QUOT_TOP=4127, NORM1=361, NORM1_DBL=361, MUL_SMALL=1296,
              WEAK_REDUCE=636, LINCOMB3P=1408, CANON=1240, IS_ZERO=1240, EQUAL=1392, SIGN=1240, TO_WORDS=1240, INV=1240, FP2_MUL=1748,
              FP2_SQR=263, FP2_MUL2_ADD=1748, FP2_MUL2_SUB=1748, FP2_MUL_INJ=1748, FP2_MUL_IP=361, FP2_IS_ZERO=1240, FP2_INV=263, FP2_SIGN=1240,
              SQR2=263, MUL_MSQR2=1640, FP2_CONJ=203, FP2_CONJ_MUL_CI=1748, FP2_CONJ_MUL_NEG_I=203, FP2_CONJ_MUL_A1MI=1748, FP2_MUL_FP=1748,
              FP2_NORM1_DBL=361, FH2_ADD=351, FH2_SUB=351, FH2_NEG=203, FH2_DBL=203, FH2_NORM1=361, FH2_MUL_SMALL=1296, FH2_SELECT=203, FH2_CONJ=203,
              FH2_MUL_IP=361, FH2_IS_ZERO=640, FH2_MUL=1748, FH2_SQR=263, FH2_MUL2_ADD=1748, FH2_MUL2_SUB=1748, FH2_MUL_FP=1748, FH2_CONJ_MUL_CI=1748,
              FH2_CONJ_MUL_NEG_I=203, FH2_CONJ_MUL_A1MI=1748, FH2_ONE=40)
N_RANDOM = 128                           # uniformly random vectors per op (the only part that may be resized for run time)


def val(l):
    return sum(x << (LB * i) for i, x in enumerate(l))


def to_limbs(v):
    """limbs 0..12 in [0, 2^28), signed top limb"""
    return [(v >> (LB * i)) & M28 for i in range(NL - 1)] + [v >> (LB * (NL - 1))]


def redc(F):
    q, r = divmod(F + ((-F * PINV) % RM) * P, RM)
    assert r == 0
    return q


def col_ok(sum_lblb, inj_lb=0):
    """the column inequality, in integers and as the checker evaluates it (double precision)"""
    exact = 14 * sum_lblb + 14 * (1 << 56) + (1 << 40) + inj_lb < (1 << 63)
    return exact and 14.0 * float(sum_lblb) + 14.0 * 2.0 ** 56 + 2.0 ** 40 + float(inj_lb) < 2.0 ** 63


def limb_limit(T, room=0):
    L = isqrt(((1 << 63) - 14 * (1 << 56) - (1 << 40) - room) // (14 * T))
    while not col_ok(T * L * L, room):   # the checker's doubles round the sum up by at most a few units of 2^10
        L -= 1
    return L


class Operand:
    __slots__ = ("l", "lb", "vb", "v")

    def __init__(self, limbs, lb=None, vb=None):
        self.l = list(limbs)
        assert len(self.l) == NL and all(-(1 << 31) <= x <= T31 for x in self.l), self.l
        self.v = val(self.l)
        m = max(abs(x) for x in self.l)
        self.lb = float(m if lb is None else lb)
        assert self.lb >= m
        real = abs(self.v) / P
        self.vb = real * (1 + 1e-12) + 1e-30 if vb is None else float(vb)
        assert abs(self.v) <= self.vb * P * (1 + 1e-9) + 1


PATTERNS = ["pos", "neg", "alt", "alt-", "pos1neg@0", "pos1neg@6", "pos1neg@12", "neg1pos@0", "neg1pos@12", "zero", "one", "minus1", "m28", "p28", "n28",
            "random"]


FILL = {"zero": 0, "one": 1, "minus1": -1, "m28": M28, "p28": 1 << LB, "n28": -(1 << LB)}


def fill_fits(pattern, L):
    return abs(FILL.get(pattern, 0)) <= L


def low_limbs(pattern, L, rng):
    n = NL - 1
    if pattern == "pos": return [L] * n
    if pattern == "neg": return [-L] * n
    if pattern == "alt": return [L if i % 2 == 0 else -L for i in range(n)]
    if pattern == "alt-": return [-L if i % 2 == 0 else L for i in range(n)]
    if pattern.startswith("pos1neg@"):
        j = int(pattern[8:]); return [-L if i == j else L for i in range(n)]
    if pattern.startswith("neg1pos@"):
        j = int(pattern[8:]); return [L if i == j else -L for i in range(n)]
    fill = {"zero": 0, "one": 1, "minus1": -1, "m28": M28, "p28": 1 << LB, "n28": -(1 << LB)}
    if pattern in fill:
        assert abs(fill[pattern]) <= L
        return [fill[pattern]] * n
    assert pattern == "random"
    return [rng.randint(-L, L) for _ in range(n)]


def vb_limit(L):
    """the largest value bound whose top limb (VB p / 2^364, plus what the lower limbs carry into it) stays inside the limb limit L"""
    return (min(L, T31) - 8) // 106514


def fit_top(top, L):
    """a ('cap', VB, sign) request brought under the operand's limb limit, explicitly: the top limb is a limb"""
    return ("cap", min(top[1], vb_limit(L)), top[2]) if isinstance(top, tuple) else top


def fit_pair(ta, tb, la, lb_):
    """the value bounds of a product's two operands under their limb limits; what one side cannot hold goes to the other, so that the
    product of the two stays at the target"""
    if not (isinstance(ta, tuple) and isinstance(tb, tuple)):
        return fit_top(ta, la), fit_top(tb, lb_)
    target = ta[1] * tb[1]
    va = min(ta[1], vb_limit(la))
    vb = min(target // va, vb_limit(lb_))
    va = min(target // vb, vb_limit(la))
    return ("cap", va, ta[2]), ("cap", vb, tb[2])


def operand(pattern, L, top, rng, declare_lb=True):
    """limbs 0..12 by pattern at limit L; top = 0 / +1 / -1 or ('cap', VB, sign): the largest top limb that keeps |value| <= VB p"""
    low = low_limbs(pattern, L, rng)
    lowv = val(low)
    if isinstance(top, tuple):
        _, VB, sign = top
        assert VB <= vb_limit(L), (VB, L)                         # the caller asks only for what the limb limit allows (fit_top)
        vmax = VB * P
        t = (vmax - lowv) // TOPW if sign > 0 else -((vmax + lowv) // TOPW)
        o = Operand(low + [t], lb=L if declare_lb else None, vb=VB)
        assert abs(o.v) <= vmax and abs(t) <= L and abs(o.v) > vmax - 2 * TOPW
        return o
    return Operand(low + [top], lb=L if declare_lb else None)


def moved(v, kind, rng, cmax=7):
    """another representation of the integer v: c 2^28 moved between neighbouring limbs"""
    l = to_limbs(v)
    if kind in ("alt", "random"):
        cmax = min(cmax, 6)                      # room for the neighbour's carry inside int32
    if kind == "plain":
        cs = [0] * (NL - 1)
    elif kind == "up":
        cs = [cmax] * (NL - 1)
    elif kind == "down":
        cs = [-cmax] * (NL - 1)
    elif kind == "alt":
        cs = [cmax if i % 2 == 0 else -cmax for i in range(NL - 1)]
    else:
        cs = [rng.randint(-cmax, cmax) for _ in range(NL - 1)]
    for i, c in enumerate(cs):
        l[i] -= c << LB
        l[i + 1] += c
    o = Operand(l)
    assert o.v == v
    return o


MOVES = ["plain", "up", "down", "alt", "random"]


class Vec:
    __slots__ = ("x", "k")

    def __init__(self, x, k=(0, 0, 0, 0)):
        self.x = list(x)
        self.k = list(k) + [0] * (4 - len(k))


# ---------------------------------------------------------------- expected values
def products(name, A):
    """the integer F of a product form and the list of (A_t, B_t) magnitudes for its bound"""
    if name in ("MUL", "RED1", "REDS1", "INJ", "INJ_CONST", "INJ_LIT"): return [(1, A[0], A[1])]
    if name in ("SQR", "SQR_INJ_CONST"): return [(1, A[0], A[0])]
    if name == "MUL2_ADD": return [(1, A[0], A[1]), (1, A[2], A[3])]
    if name == "MUL2_SUB": return [(1, A[0], A[1]), (-1, A[2], A[3])]
    if name == "SQR2": return [(2, A[0], A[0])]
    if name == "MUL_MSQR2": return [(1, A[0], A[1]), (-2, A[2], A[2])]
    if name[:3] == "RED":
        T = int(name[-1]); return [((-1) ** t, A[2 * t], A[2 * t + 1]) for t in range(T)]
    raise KeyError(name)


def injected(name, A, k):
    """list of (multiplier, integer) of the injected addends"""
    if name == "INJ": return [(k[0], A[2]), (k[1], A[3]), (k[2], P)]
    if name == "INJ_CONST": return [(1, A[2]), (-2, A[3]), (3, P)]
    if name == "SQR_INJ_CONST": return [(-1, A[1]), (2, A[2]), (-3, P)]
    if name == "INJ_LIT": return [(3, A[2]), (-1, A[3]), (2, P)]
    return []


def fp2_forms(name, A, k):
    """per output coordinate: (products, injected).  A two-lane op FH2_X has the expectation of FP2_X: the Fp2 formula, not the lane routine."""
    if name[:4] == "FH2_":
        name = "FP2_" + name[4:]
    a, b = A[0], A[1]
    if name == "FP2_MUL_FP":                                       # (a + b i) s
        return [([(1, a, A[2])], []), ([(1, b, A[2])], [])]
    if name == "FP2_CONJ_MUL_CI":                                  # (a - b i) (c i) = b c + a c i
        return [([(1, b, A[2])], []), ([(1, a, A[2])], [])]
    if name == "FP2_CONJ_MUL_A1MI":                                # +-(a - b i) c (1 - i) = +-((a - b) c - (a + b) c i), - when k0 != 0
        s = -1 if k[0] else 1
        return [([(s, a - b, A[2])], []), ([(-s, a + b, A[2])], [])]
    if name in ("FP2_MUL", "FP2_MUL_INJ"):
        c, d = A[2], A[3]
        ia = [(k[0], A[4]), (k[2], P)] if name == "FP2_MUL_INJ" else []
        ib = [(k[1], A[5]), (k[3], P)] if name == "FP2_MUL_INJ" else []
        return [([(1, a, c), (-1, b, d)], ia), ([(1, a, d), (1, b, c)], ib)]
    if name == "FP2_SQR":
        return [([(1, a, a), (-1, b, b)], []), ([(2, a, b)], [])]
    s = 1 if name == "FP2_MUL2_ADD" else -1
    c, d, e, f, g, h = A[2], A[3], A[4], A[5], A[6], A[7]         # (a + b i)(c + d i) +- (e + f i)(g + h i)
    return [([(1, a, c), (-1, b, d), (s, e, g), (-s, f, h)], []), ([(1, a, d), (1, b, c), (s, e, h), (s, f, g)], [])]


def reduce_form(prods, inj):
    F = sum(s * x * y for s, x, y in prods) + RM * sum(m * c for m, c in inj)
    out = redc(F)
    # |value| < (sum VBa VBb p / R + 1 + inj) p, in integers
    assert abs(out) * RM < sum(abs(s * x * y) for s, x, y in prods) + (P + sum(abs(m * c) for m, c in inj)) * RM, "value post-condition"
    l = to_limbs(out)
    assert -(1 << 31) <= l[NL - 1] <= T31
    return l


def canon(v):
    return v * RINV % P


def inv_limbs(v):
    c = canon(v)
    return to_limbs(redc((pow(c, -1, P) if c else 0) * R2))


def expected(name, vec):
    """list of expected raw outputs (14 integers each); None for an output that is checked by properties only (WEAK_REDUCE, QUOT_TOP)"""
    A = [o.v for o in vec.x]
    L = [o.l for o in vec.x]
    k = vec.k
    flag = lambda b: [int(b)] + [0] * (NL - 1)
    if name in ("MUL", "SQR", "MUL2_ADD", "MUL2_SUB", "INJ", "INJ_CONST", "SQR_INJ_CONST", "INJ_LIT", "SQR2", "MUL_MSQR2") or name[:3] == "RED":
        return [reduce_form(products(name, A), injected(name, A, k))]
    if name in FP2_PRODUCTS:
        return [reduce_form(p_, i_) for p_, i_ in fp2_forms(name, A, k)]

    def norm1(l):
        r = [(l[i] & M28) + (l[i - 1] >> LB if i else 0) for i in range(NL - 1)] + [l[NL - 1] + (l[NL - 2] >> LB)]
        assert val(r) == val(l)
        return r

    def norm1_dbl(l):
        r = [((2 * l[i]) & M28) + (l[i - 1] >> (LB - 1) if i else 0) for i in range(NL - 1)] + [2 * l[NL - 1] + (l[NL - 2] >> (LB - 1))]
        assert val(r) == 2 * val(l)
        return r

    if name == "NORM1": return [norm1(L[0])]
    if name == "NORM1_DBL": return [norm1_dbl(L[0])]
    if name == "FH2_NORM1": return [norm1(L[0]), norm1(L[1])]
    if name == "FP2_NORM1_DBL": return [norm1_dbl(L[0]), norm1_dbl(L[1])]
    if name == "FH2_ADD": return [[x + y for x, y in zip(L[0], L[2])], [x + y for x, y in zip(L[1], L[3])]]
    if name == "FH2_SUB": return [[x - y for x, y in zip(L[0], L[2])], [x - y for x, y in zip(L[1], L[3])]]
    if name == "FH2_NEG": return [[-x for x in L[0]], [-x for x in L[1]]]
    if name == "FH2_DBL": return [[2 * x for x in L[0]], [2 * x for x in L[1]]]
    if name == "FH2_MUL_SMALL": return [to_limbs(k[0] * A[0]), to_limbs(k[0] * A[1])]
    if name == "FH2_SELECT": return [L[0], L[1]] if k[0] else [L[2], L[3]]
    if name in ("FP2_CONJ", "FH2_CONJ"): return [L[0], [-x for x in L[1]]]
    if name in ("FP2_CONJ_MUL_NEG_I", "FH2_CONJ_MUL_NEG_I"): return [[-x for x in L[1]], [-x for x in L[0]]]       # (a - b i)(-i) = -b - a i
    if name == "FH2_IS_ZERO": return [flag(A[0] % P == 0 and A[1] % P == 0)] * 2                                 # the flag of each of the two lanes
    if name == "FH2_ONE": return [to_limbs(RM % P), [0] * NL]
    if name == "MUL_SMALL": return [to_limbs(k[0] * A[0])]
    if name == "LINCOMB3P": return [to_limbs(k[0] * A[0] + k[1] * A[1] + k[2] * A[2] + k[3] * P)]
    if name in ("WEAK_REDUCE", "QUOT_TOP"): return [None]
    if name == "CANON": return [to_limbs(canon(A[0]))]
    if name == "IS_ZERO": return [flag(A[0] % P == 0)]
    if name == "EQUAL": return [flag((A[0] - A[1]) % P == 0)]
    if name == "SIGN": return [flag(canon(A[0]) & 1)]
    if name == "TO_WORDS":
        c = canon(A[0])
        return [[((c >> (32 * (11 - j))) & 0xffffffff) for j in range(12)] + [0, 0]]
    if name == "INV": return [inv_limbs(A[0])]
    if name == "ADD": return [[x + y for x, y in zip(L[0], L[1])]]
    if name == "SUB": return [[x - y for x, y in zip(L[0], L[1])]]
    if name == "NEG": return [[-x for x in L[0]]]
    if name in ("FP2_MUL_IP", "FH2_MUL_IP"): return [[x - y for x, y in zip(L[0], L[1])], [x + y for x, y in zip(L[0], L[1])]]
    if name == "FP2_IS_ZERO": return [flag(A[0] % P == 0 and A[1] % P == 0)]
    if name == "FP2_SIGN":
        ca, cb = canon(A[0]), canon(A[1])
        return [flag((cb if ca == 0 else ca) & 1)]
    if name == "FP2_INV":
        n = redc(A[0] * A[0] + A[1] * A[1])
        ni = val(inv_limbs(n))
        return [to_limbs(redc(A[0] * ni)), to_limbs(redc(-A[1] * ni))]
    raise KeyError(name)


def check_outputs(name, vec, outs, bounds=None):
    """outs: raw limbs as the harness returned them (signed 32-bit integers); bounds: host only, (lb, vb) declared per output"""
    exp = expected(name, vec)
    assert len(outs) == len(exp)
    for e, got in zip(exp, outs):
        if name == "TO_WORDS":
            got = [g & 0xffffffff for g in got]
        if e is not None:
            assert list(got) == e, "%s: operands %s k %s\n expected %s\n obtained %s" % (name, [o.l for o in vec.x], vec.k, e, list(got))
    if name == "WEAK_REDUCE":
        got = outs[0]
        assert all(0 <= x <= M28 for x in got[:NL - 1]), got
        assert (val(got) - vec.x[0].v) % P == 0 and 10 * abs(val(got)) <= 16 * P, (vec.x[0].l, got)
    if name == "QUOT_TOP":
        q, top = outs[0][0], vec.k[0]
        # |top 2^364 - q p| <= (1/2 + 2/106513) p
        assert 2 * 106513 * abs(top * TOPW - q * P) <= (106513 + 4) * P, (top, q)
    if name in NORMALISED:
        for got in outs:
            assert all(0 <= x <= M28 for x in got[:NL - 1]), (name, got)
    if bounds is not None and name not in PREDICATES:
        for got, (lb, vb) in zip(outs, bounds):
            assert max(abs(x) for x in got) <= lb and abs(val(got)) <= vb * P * (1 + 1e-9), (name, got, lb, vb)
            assert abs(got[NL - 1]) <= lb


PREDICATES = ("IS_ZERO", "EQUAL", "SIGN", "TO_WORDS", "FP2_IS_ZERO", "FP2_SIGN", "QUOT_TOP", "FH2_IS_ZERO")
# Montgomery products of Fp2 elements, one reduce_form per coordinate (fp2_forms)
FP2_PRODUCTS = ("FP2_MUL", "FP2_SQR", "FP2_MUL2_ADD", "FP2_MUL2_SUB", "FP2_MUL_INJ", "FP2_MUL_FP", "FP2_CONJ_MUL_CI", "FP2_CONJ_MUL_A1MI",
                "FH2_MUL", "FH2_SQR", "FH2_MUL2_ADD", "FH2_MUL2_SUB", "FH2_MUL_FP", "FH2_CONJ_MUL_CI", "FH2_CONJ_MUL_A1MI")
NORMALISED = ("MUL", "SQR", "MUL2_ADD", "MUL2_SUB", "RED1", "RED2", "RED3", "RED4", "REDS1", "REDS2", "REDS3", "REDS4", "INJ", "INJ_CONST", "SQR_INJ_CONST",
              "INJ_LIT", "MUL_SMALL", "WEAK_REDUCE", "LINCOMB3P", "CANON", "INV", "FP2_INV", "SQR2", "MUL_MSQR2", "FH2_MUL_SMALL", "FH2_ONE") + FP2_PRODUCTS


# ---------------------------------------------------------------- preconditions (real limbs, real values)
def lbs(vec):
    return [max(abs(x) for x in o.l) for o in vec.x]


def forms_of(name, k):
    """the bilinear forms of an op, one per output coordinate: ([(weight, operand a, operand b)], [(multiplier, addend operand or None for p)])"""
    if name in ("MUL", "RED1", "REDS1"): forms = [([(1, 0, 1)], [])]
    elif name == "SQR": forms = [([(1, 0, 0)], [])]
    elif name in ("MUL2_ADD", "MUL2_SUB", "RED2", "REDS2"): forms = [([(1, 0, 1), (1, 2, 3)], [])]
    elif name in ("RED3", "REDS3"): forms = [([(1, 0, 1), (1, 2, 3), (1, 4, 5)], [])]
    elif name in ("RED4", "REDS4"): forms = [([(1, 0, 1), (1, 2, 3), (1, 4, 5), (1, 6, 7)], [])]
    elif name == "INJ": forms = [([(1, 0, 1)], [(k[0], 2), (k[1], 3), (k[2], None)])]
    elif name == "INJ_CONST": forms = [([(1, 0, 1)], [(1, 2), (2, 3), (3, None)])]
    elif name == "INJ_LIT": forms = [([(1, 0, 1)], [(3, 2), (1, 3), (2, None)])]
    elif name == "SQR_INJ_CONST": forms = [([(1, 0, 0)], [(1, 1), (2, 2), (3, None)])]
    elif name == "FP2_MUL": forms = [([(1, 0, 2), (1, 1, 3)], []), ([(1, 0, 3), (1, 1, 2)], [])]
    elif name == "FP2_MUL_INJ": forms = [([(1, 0, 2), (1, 1, 3)], [(k[0], 4), (k[2], None)]), ([(1, 0, 3), (1, 1, 2)], [(k[1], 5), (k[3], None)])]
    elif name in ("FP2_SQR", "FP2_INV"): forms = [([(1, 0, 0), (1, 1, 1)], []), ([(2, 0, 1)], [])]
    elif name in ("FP2_MUL2_ADD", "FP2_MUL2_SUB"): forms = [([(1, 0, 2), (1, 1, 3), (1, 4, 6), (1, 5, 7)], []), ([(1, 0, 3), (1, 1, 2), (1, 4, 7), (1, 5, 6)], [])]
    elif name == "SQR2": forms = [([(2, 0, 0)], [])]                                              # fp_mul(a, 2a)
    elif name == "MUL_MSQR2": forms = [([(1, 0, 1), (2, 2, 2)], [])]
    elif name in ("FP2_MUL_FP", "FP2_CONJ_MUL_CI", "FH2_MUL_FP", "FH2_CONJ_MUL_CI"): forms = [([(1, 0, 2)], []), ([(1, 1, 2)], [])]
    # the product operand y.a -+ y.b is a lazy sum: bounds LB(y.a) + LB(y.b) and VB(y.a) + VB(y.b), one product per coordinate
    elif name in ("FP2_CONJ_MUL_A1MI", "FH2_CONJ_MUL_A1MI"): forms = [([(1, 0, 2), (1, 1, 2)], [])]
    # the two-lane products, as fp2h.hpp forms them per lane (role: real / imaginary):
    #   FH2_MUL     fp_mul2: own * U + partner * V with (U, V) = (y.a, -y.b) / (y.a, y.b): the operand pairs of FP2_MUL
    #   FH2_MUL2_*  four such products in one static reduction: the operand pairs of FP2_MUL2_*
    #   FH2_SQR     ONE product of two lazy sums: (a + b)(a - b), bound (LBa + LBb)^2 = LBa^2 + 2 LBa LBb + LBb^2, / (2a) b, whose left
    #               factor is an fp_select of 2 partner and a + b and declares the larger: 2 LBa (LBa + LBb) and 2 LBb (LBa + LBb)
    elif name == "FH2_MUL": forms = forms_of("FP2_MUL", k)
    elif name in ("FH2_MUL2_ADD", "FH2_MUL2_SUB"): forms = forms_of("FP2_MUL2_ADD", k)
    elif name == "FH2_SQR": forms = [([(1, 0, 0), (2, 0, 1), (1, 1, 1)], []), ([(2, 0, 0), (2, 0, 1)], []), ([(2, 1, 1), (2, 0, 1)], [])]
    else: forms = []
    return forms


def reach(name, vec):
    """(sum VBa VBb / 10^6, column bound / 2^63) of a vector, the larger over the op's forms; the column bound from the declared limb limits"""
    A = [abs(o.v) for o in vec.x]
    D = [int(o.lb) for o in vec.x]
    best_v = best_c = 0.0
    for prods, inj in forms_of(name, vec.k):
        vv = sum(abs(s) * A[x] * A[y] for s, x, y in prods)
        cc = 14 * sum(abs(s) * D[x] * D[y] for s, x, y in prods) + 14 * (1 << 56) + (1 << 40) + sum(abs(m) * (D[c] if c is not None else 1 << LB) for m, c in inj)
        best_v, best_c = max(best_v, vv / (CAP * P * P)), max(best_c, cc / (1 << 63))
    return best_v, best_c


def assert_precondition(name, vec):
    A = [abs(o.v) for o in vec.x]
    B = lbs(vec)
    D = [int(o.lb) for o in vec.x]              # the declared limits obey the same inequality (they are what the checker multiplies)
    k = vec.k

    def form(prods, inj=(), w=B):
        ll = sum(abs(s) * w[x] * w[y] for s, x, y in prods)
        il = sum(abs(m) * (w[c] if c is not None else 1 << LB) for m, c in inj)
        assert col_ok(ll, il), (name, "column", ll, il)
        assert sum(abs(s) * A[x] * A[y] for s, x, y in prods) <= CAP * P * P, (name, "value cap")
        assert (sum(abs(s) * A[x] * A[y] for s, x, y in prods) // RM + P + sum(abs(m) * (A[c] if c is not None else P) for m, c in inj)) // TOPW + 2 <= T31, (name, "top limb")

    forms = forms_of(name, k)
    for prods, inj in forms:
        form(prods, inj, B)
        form(prods, inj, D)
    if name in ("SQR", "SQR_INJ_CONST"): assert 2 * D[0] <= T31
    if name in ("FP2_SQR", "FP2_INV"): assert 2 * D[0] <= T31 and 2 * D[1] <= T31
    if name == "FP2_INV": assert col_ok(D[0] << LB) and col_ok(D[1] << LB)
    if name == "NORM1": assert A[0] // TOPW + 4 + (D[0] >> LB) <= T31
    if name == "NORM1_DBL": assert 2 * (A[0] // TOPW) + 8 + (2 * D[0] >> LB) <= T31 and abs(vec.x[0].l[NL - 1]) < (1 << 30) - 16
    if name == "MUL_SMALL": assert k[0] >= 0 and k[0] * A[0] // TOPW + 3 <= T31
    if name == "WEAK_REDUCE": assert A[0] <= 2400 * P and vec.x[0].vb <= 2400.0
    if name == "LINCOMB3P":
        assert (abs(k[0]) * A[0] + abs(k[1]) * A[1] + abs(k[2]) * A[2] + abs(k[3]) * P) // TOPW + 3 <= T31
        assert abs(k[0]) * D[0] + abs(k[1]) * D[1] + abs(k[2]) * D[2] + (abs(k[3]) << LB) < 1 << 62
    if name in ("EQUAL", "ADD", "SUB", "FP2_MUL_IP", "FH2_MUL_IP", "FP2_CONJ_MUL_A1MI", "FH2_CONJ_MUL_A1MI"): assert D[0] + D[1] <= T31
    if name in ("CANON", "IS_ZERO", "SIGN", "TO_WORDS", "INV", "FP2_IS_ZERO", "FP2_SIGN", "FH2_IS_ZERO"): assert all(col_ok(d) for d in D)
    if name == "SQR2": assert 2 * D[0] <= T31
    if name == "MUL_MSQR2": assert 4 * D[2] <= T31                                           # -4c is formed as raw limbs
    if name in ("FH2_ADD", "FH2_SUB"): assert D[0] + D[2] <= T31 and D[1] + D[3] <= T31
    if name in ("FH2_DBL", "FH2_SQR"): assert 2 * D[0] <= T31 and 2 * D[1] <= T31
    if name == "FH2_SQR": assert D[0] + D[1] <= T31
    if name == "FH2_NORM1": assert all(A[i] // TOPW + 4 + (D[i] >> LB) <= T31 for i in (0, 1))
    if name == "FP2_NORM1_DBL": assert all(2 * (A[i] // TOPW) + 8 + (2 * D[i] >> LB) <= T31 and abs(vec.x[i].l[NL - 1]) < (1 << 30) - 16 for i in (0, 1))
    if name == "FH2_MUL_SMALL": assert k[0] >= 0 and all(k[0] * A[i] // TOPW + 3 <= T31 for i in (0, 1))
    if name in ("FH2_NEG", "FH2_CONJ", "FH2_CONJ_MUL_NEG_I", "FP2_CONJ", "FP2_CONJ_MUL_NEG_I"): assert all(x > -(1 << 31) for o in vec.x for x in o.l)
    if name in ("FH2_MUL", "FH2_MUL2_ADD", "FH2_MUL2_SUB"):
        # fp2h_lane_uv takes U and V by fp_select, which declares the larger bound of y's two halves for both: what the checker multiplies is
        # (LBx.a + LBx.b) max(LBy.a, LBy.b) per product pair, and the same in value bounds — no weaker than the pairs really formed (above)
        V = [o.vb for o in vec.x]
        pairs = [(0, 1, 2, 3)] if name == "FH2_MUL" else [(0, 1, 2, 3), (4, 5, 6, 7)]
        assert col_ok(sum((D[a] + D[b]) * max(D[c], D[d]) for a, b, c, d in pairs)), (name, "column, declared by fp_select")
        assert sum((V[a] + V[b]) * max(V[c], V[d]) for a, b, c, d in pairs) <= CAP, (name, "value cap, declared by fp_select")
    if name in ("FH2_SQR", "FH2_CONJ_MUL_A1MI", "FP2_CONJ_MUL_A1MI"):
        V = [o.vb for o in vec.x]                                                             # the lazy sums' DECLARED value bounds are what is multiplied
        assert (V[0] + V[1]) * (max(2 * V[0], 2 * V[1], V[0] + V[1]) if name == "FH2_SQR" else V[2]) <= CAP, (name, "value cap, declared")


# ---------------------------------------------------------------- generators
TOP_PAIRS = [(0, 0), (1, -1), (("cap", 1000, 1), ("cap", 1000, 1)), (("cap", 1000, 1), ("cap", 1000, -1)), (("cap", 1000, -1), ("cap", 1000, -1)),
             (("cap", 20000, -1), ("cap", 50, 1)), (("cap", 45, 1), ("cap", 45, -1)), (("cap", 1, 1), ("cap", 1, 1)), (("cap", 1, -1), ("cap", 1, 1))]
SQUARE_TOPS = [(t, t) for t in (0, 1, -1, ("cap", 1000, 1), ("cap", 1000, -1), ("cap", 45, 1), ("cap", 45, -1), ("cap", 1, 1), ("cap", 1, -1))]
# 1000 x 1000 and 20000 x 50 = the cap 10^6; 45 x 45 <= 2^11: the "(-p, 2p)" case; 1 x 1


def scale_top(top, T):
    """share a value-bound target between the T products of a form"""
    if not isinstance(top, tuple):
        return top
    return ("cap", max(1, isqrt(top[1] * top[1] // T)) if top[1] >= 45 else top[1], top[2])


def product_vectors(name, T, pairs, rng, room=0, square=False, extra=None, amax=T31):
    """pairs: operand index pairs (a_t, b_t) of the T products; extra(rng) -> (further operands, k); amax: the largest limb limit the first
    operand of a pair may take (below 2^31 - 1 where the routine adds two such operands before it multiplies)"""
    L = limb_limit(T, room)
    limits = [(L, L)] if square else [(L, L), (amax, L * L // amax), (min(L * L >> LB, amax - 1), L * L // min(L * L >> LB, amax - 1))]
    out = []
    n_ops = ARITY[name]

    def build(la, lb_, pa, pb, ta, tb, flip):
        x = [None] * n_ops
        for t, (ia, ib) in enumerate(pairs):
            neg = flip and t % 2 == 1
            pa_t = {"pos": "neg", "neg": "pos", "alt": "alt-", "alt-": "alt"}.get(pa, pa) if neg else pa
            fa, fb = fit_pair(scale_top(ta, T), scale_top(tb, T), la, lb_)
            if x[ia] is None: x[ia] = operand(pa_t, la, fa, rng)
            if x[ib] is None: x[ib] = operand(pb, lb_, fb, rng)
        k = [0, 0, 0, 0]
        if extra:
            more, k = extra(rng)
            for i, o in zip([i for i in range(n_ops) if x[i] is None], more): x[i] = o
        assert all(o is not None for o in x)
        return Vec(x, k)

    for la, lb_ in limits:
        for pa in PATTERNS[:-1]:
            for pb in (["pos"] if square else ["pos", "neg", "alt", pa]):
                if square: pb = pa
                # a constant fill of +-2^28 is above the limb limit of the small partner of an unbalanced pair: that operand takes "pos" there,
                # and a pair of limits whose FIRST operand cannot hold pa's fill has no vector for pa (COUNTS is the count after this rule)
                if not fill_fits(pa, la): continue
                if not fill_fits(pb, lb_): pb = "pos"
                for ta, tb in (SQUARE_TOPS if square else TOP_PAIRS):
                    out.append(build(la, lb_, pa, pb, ta, tb, flip=True))
    for i in range(N_RANDOM):
        la, lb_ = limits[i % len(limits)]
        ta, tb = (SQUARE_TOPS if square else TOP_PAIRS)[i % len(SQUARE_TOPS if square else TOP_PAIRS)]
        out.append(build(la, lb_, "random", "random", ta, tb, flip=False))
    return out


KS = [1, -1, 2, -2, 3, -3, 17, -31]


def addend(rng, i):
    """an injected addend: lazy limbs up to 2^31 - 1, value up to 100 p"""
    L = [T31, (1 << LB) + 5, 1 << 29][i % 3]
    return operand(PATTERNS[i % len(PATTERNS)], L, [0, 1, -1, ("cap", 100, 1), ("cap", 100, -1), ("cap", 1, -1)][i % 6], rng)


def inj_extra(n_add, n_k):
    state = [0]

    def f(rng):
        i = state[0]; state[0] += 1
        return [addend(rng, i + j) for j in range(n_add)], [KS[(i + 3 * j) % len(KS)] for j in range(n_k)]
    return f


def carry_vectors(name, rng):
    out = []
    if name in ("NORM1", "NORM1_DBL", "FP2_MUL_IP"):
        L = T31 if name == "NORM1" else (1 << 30) - 1
        tops = [0, 1, -1, ("cap", 9000, 1), ("cap", 9000, -1)]
        for pa in PATTERNS[:-1]:
            for ta in tops:
                x = [operand(pa, L, ta, rng)]
                if name == "FP2_MUL_IP": x.append(operand(PATTERNS[(PATTERNS.index(pa) + 3) % 15], L, ta, rng))
                out.append(Vec(x))
            x = [Operand(low_limbs(pa, L, rng) + [s * (L - 20000)]) for s in (1, -1)]      # top limb at the int32 edge
            out += [Vec([o] + ([operand("alt", L, 0, rng)] if name == "FP2_MUL_IP" else [])) for o in x]
        for i in range(N_RANDOM):
            for full in (False, True):
                l = [rng.randint(-L, L) if not full else rng.choice([-L - 1, L, -1, 0, M28, 1 << LB]) for _ in range(NL - 1)] + [rng.randint(-L // 4, L // 4)]
                x = [Operand(l)]
                if name == "FP2_MUL_IP": x.append(Operand([rng.randint(-L, L) for _ in range(NL)]))
                if len(out) < COUNTS[name]: out.append(Vec(x))
    elif name == "MUL_SMALL":
        for kk in (0, 1, 2, 3, 4, 8, 12, 1000, 20000):
            for pa in PATTERNS:
                for ta in (0, 1, -1, ("cap", 20000 // max(kk, 1), 1), ("cap", 20000 // max(kk, 1), -1), ("cap", 1, 1), ("cap", 1, -1), 53, -97):
                    out.append(Vec([operand(pa, T31, ta, rng)], [kk]))
    elif name == "WEAK_REDUCE":
        for pa in PATTERNS + ["random"] * (N_RANDOM - 1):
            for ta in (0, 1, -1, ("cap", 2400, 1), ("cap", 2400, -1), ("cap", 1, 1), ("cap", 1, -1), ("cap", 1200, 1), ("cap", 37, -1), 53256, 53257, -53257):
                if len(out) < COUNTS[name]: out.append(Vec([operand(pa, T31, ta, rng)]))
    elif name == "LINCOMB3P":
        ks = [1, -1, 2, -2, 3, -3, 100, -100]
        i = 0
        for pa in PATTERNS:
            for ta in (0, 1, -1, ("cap", 30, 1), ("cap", 30, -1), ("cap", 1, -1)):
                for j in range(8):
                    x = [operand(pa, T31, ta, rng), operand(PATTERNS[(i + j) % 16], T31, ta, rng), operand(PATTERNS[(i + 2 * j + 1) % 16], (1 << LB) + 3, ta, rng)]
                    out.append(Vec(x, [ks[(i + j) % 8], ks[(i + 3 * j + 1) % 8], ks[(2 * i + j) % 8], ks[(i + 5 * j + 2) % 8]]))
                    i += 1
        # small values in large lazy limbs under large multipliers: the 64-bit running sum near 2^62
        for i in range(COUNTS[name] - len(out)):
            x = [moved(rng.randint(-3, 3) * (P >> 36) + rng.randint(-5, 5), MOVES[i % 5], rng) for _ in range(3)]
            big = 1 << 29
            out.append(Vec(x, [rng.choice([big, -big, big - 1]), rng.choice([big // 2, -big // 2]), rng.randint(-big // 2, big // 2), rng.randint(-3, 3)]))
    return out


PRED_K = list(range(-12, 13)) + [100, -100, 1000, -1000, 19000, -19000]
PRED_E = [0, 1, -1, 2, -2, (P - 1) // 2, P - 1, 12345678901234567890123]


def predicate_values():
    return [k * P + e for k in PRED_K for e in PRED_E]


def predicate_vectors(name, rng):
    out = []
    vals = predicate_values()
    if name in ("CANON", "IS_ZERO", "SIGN", "TO_WORDS", "INV"):
        for v in vals:
            for mv in MOVES:
                out.append(Vec([moved(v, mv, rng)]))
    elif name == "EQUAL":
        for v in [k * P + e for k in PRED_K if abs(k) <= 1000 for e in PRED_E]:          # the difference's top limb stays inside int32
            for j, (mv, d) in enumerate([("plain", 0), ("up", P), ("down", -3 * P), ("alt", 1), ("random", 7 * P), ("random", -1)]):
                out.append(Vec([moved(v, MOVES[j % 5], rng, cmax=2), moved(v + d, mv, rng, cmax=2)]))
    elif name in ("FP2_IS_ZERO", "FP2_SIGN"):
        for i, v in enumerate(vals):
            for j, mv in enumerate(MOVES):
                w = [0, 5 * P, vals[(i * 7 + j) % len(vals)], -P, 1][j]          # a == 0 (mod p) in all its forms, and generic partners
                pair = [moved(v, mv, rng), moved(w, MOVES[(j + 2) % 5], rng)]
                out.append(Vec(pair if (i + j) % 2 else pair[::-1]))
    return out


def quot_top_vectors(rng):
    tops = set()
    for e in (0, 1, 53256, 53257, 106513, 106514, (1 << 28) - 1, 1 << 27, 2400 * 106513, 2520 * 106513 + 53256):
        for d in (-1, 0, 1):
            tops.add(e + d); tops.add(-(e + d))
    tops = sorted(t for t in tops if -(1 << 28) <= t < (1 << 28))
    for q in range(1, 2520, 79):                                   # both sides of rounding boundaries (q + 1/2) p / 2^364
        b = ((2 * q + 1) * P) // (2 * TOPW)
        tops += [b, b + 1, -b, -b - 1]
    tops += [rng.randint(-(1 << 28), (1 << 28) - 1) for _ in range(COUNTS["QUOT_TOP"] - len(tops))]
    return [Vec([], [t]) for t in tops]


# ---------------------------------------------------------------- Fp2 operands: the psi helpers and the two-lane ops
def paired(name, shift=7):
    """the vectors of a one-operand Fp op as Fp2 operands: each with the one `shift` places on among those of the same multipliers"""
    groups = {}
    for v in vectors(name):
        groups.setdefault(tuple(v.k), []).append(v)
    return [Vec([v.x[0], g[(j + shift) % len(g)].x[0]], v.k) for g in groups.values() for j, v in enumerate(g)]


def neg_extra():
    """no further operand; k0 = neg alternates"""
    state = [0]

    def f(rng):
        state[0] += 1
        return [], [state[0] & 1]
    return f


# limb-wise lazy operations: no product, the only limit is int32.  limits = the limb limit of each Fp2 operand (of both its halves)
#   FH2_NEG, FH2_CONJ, *_CONJ_MUL_NEG_I, FP2_CONJ, FH2_SELECT   |limb| <= 2^31 - 1 (-2^31 has no negative)
#   FH2_DBL                                                     2 LB <= 2^31 - 1:  LB = 2^30 - 1
#   FH2_ADD, FH2_SUB                                            LBx + LBy <= 2^31 - 1: (2^30 - 1, 2^30), (2^31 - 1 - 2^28, 2^28) and the reverse
def lazy_vectors(rng, limit_sets, ks=(0,)):
    out = []
    tops = [0, 1, -1, ("cap", 9000, 1), ("cap", 9000, -1)]
    i = 0
    for limits in limit_sets:
        for pi, pa in enumerate(PATTERNS[:-1]):
            for ta in tops:
                x = [operand(PATTERNS[(pi + 3 * j) % 15] if fill_fits(PATTERNS[(pi + 3 * j) % 15], lim) else "pos", lim, fit_top(ta, lim), rng)
                     for j, lim in enumerate(l for l in limits for _ in (0, 1))]
                out.append(Vec(x, [ks[i % len(ks)]]))
                i += 1
        for _ in range(N_RANDOM // len(limit_sets)):
            out.append(Vec([Operand([rng.randint(-lim, lim) for _ in range(NL)]) for lim in limits for _ in (0, 1)], [ks[i % len(ks)]]))
            i += 1
    return out


def msqr2_vectors(rng):
    """fp_mul_msqr2, a b - 2 c^2 in one reduction: 14 (LBa LBb + 2 LBc^2) + 14 2^56 + 2^40 < 2^63 and 4 LBc <= 2^31 - 1 (-4c is formed as raw
    limbs).  At the inequality three ways: all three operands at L(3); a at 2^31 - 1 against a small b, c at L(3); c at its own cap 2^29 - 1
    with a and b at what that leaves"""
    L3, L1, C = limb_limit(3), limb_limit(1), (1 << 29) - 1
    rest = isqrt(L1 * L1 - 2 * C * C)
    while not col_ok(rest * rest + 2 * C * C):
        rest -= 1
    out = []
    limits = [(L3, L3, L3), (T31, L3 * L3 // T31, L3), (rest, rest, C)]

    def build(la, lb_, lc, pa, pb, pc, ta, tb):
        fa, fb = fit_pair(scale_top(ta, 3), scale_top(tb, 3), la, lb_)
        tc = ("cap", min(scale_top(ta, 3)[1], scale_top(tb, 3)[1]), ta[2]) if isinstance(ta, tuple) else ta      # 2 VBc^2 <= 2/3 of the target VBa VBb
        return Vec([operand(pa, la, fa, rng), operand(pb, lb_, fb, rng), operand(pc, lc, fit_top(tc, lc), rng)])

    for la, lb_, lc in limits:
        for pa in PATTERNS[:-1]:
            if not fill_fits(pa, la): continue
            for pb, pc in (("pos", "pos"), ("neg", "alt"), ("alt", "neg"), (pa, pa)):
                if not fill_fits(pb, lb_): pb = "pos"
                if not fill_fits(pc, lc): pc = "pos"
                for ta, tb in TOP_PAIRS:
                    out.append(build(la, lb_, lc, pa, pb, pc, ta, tb))
    for i in range(N_RANDOM):
        la, lb_, lc = limits[i % 3]
        out.append(build(la, lb_, lc, "random", "random", "random", *TOP_PAIRS[i % len(TOP_PAIRS)]))
    return out


def fh2_is_zero_vectors(rng):
    """every combination of {0, k p (k != 0), e, k p + e} across the two halves, each in several representations"""
    ks, es = [k for k in PRED_K if k], [e for e in PRED_E if e]
    classes = [[0], [k * P for k in ks], es, [k * P + e for k in ks for e in es]]
    out = []
    for ca in classes:
        for cb in classes:
            for j in range(40):
                out.append(Vec([moved(ca[(5 * j) % len(ca)], MOVES[j % 5], rng), moved(cb[(7 * j + 3) % len(cb)], MOVES[(j // 5 + j) % 5], rng)]))
    kinds = {(v.x[0].v == 0, v.x[0].v % P == 0, v.x[1].v == 0, v.x[1].v % P == 0) for v in out}
    assert len(kinds) == 9 and sum(1 for v in out if v.x[0].v % P == 0 and v.x[1].v % P == 0) == 4 * 40
    return out


_CACHE = {}


def vectors(name):
    if name in _CACHE:
        return _CACHE[name]
    rng = random.Random("fp_raw|" + name)
    if name in ("MUL", "RED1", "REDS1"):
        v = product_vectors(name, 1, [(0, 1)], rng)
        if name == "MUL":                                          # the corner of the issue: +-L everywhere, top limb 1000 p / 2^364, and the all-ones borrow chains
            L = limb_limit(1)
            for pa in PATTERNS[:9]:
                for pb in PATTERNS[:9]:
                    for s in (1, -1):
                        v.append(Vec([operand(pa, L, ("cap", 1000, s), rng), operand(pb, L, ("cap", 1000, -s), rng)]))
            while len(v) < COUNTS[name]:
                v.append(Vec([moved(rng.randint(-999, 999) * P + rng.randint(0, P), "random", rng, cmax=1), moved(rng.randint(-999, 999) * P - rng.randint(0, P), "random", rng, cmax=1)]))
    elif name == "SQR": v = product_vectors(name, 1, [(0, 0)], rng, square=True)
    elif name in ("MUL2_ADD", "MUL2_SUB", "RED2", "REDS2"): v = product_vectors(name, 2, [(0, 1), (2, 3)], rng)
    elif name in ("RED3", "REDS3"): v = product_vectors(name, 3, [(0, 1), (2, 3), (4, 5)], rng)
    elif name in ("RED4", "REDS4"): v = product_vectors(name, 4, [(0, 1), (2, 3), (4, 5), (6, 7)], rng)
    elif name in ("INJ", "INJ_CONST", "INJ_LIT"): v = product_vectors(name, 1, [(0, 1)], rng, room=INJ_ROOM, extra=inj_extra(2, 3))
    elif name == "SQR_INJ_CONST": v = product_vectors(name, 1, [(0, 0)], rng, room=INJ_ROOM, square=True, extra=inj_extra(2, 0))
    elif name == "FP2_MUL": v = product_vectors(name, 2, [(0, 2), (1, 3)], rng)
    elif name == "FP2_MUL_INJ": v = product_vectors(name, 2, [(0, 2), (1, 3)], rng, room=INJ_ROOM, extra=inj_extra(2, 4))
    elif name in ("FP2_SQR", "FP2_INV"): v = product_vectors(name, 2, [(0, 0), (1, 1)], rng, square=True)
    elif name in ("FP2_MUL2_ADD", "FP2_MUL2_SUB"): v = product_vectors(name, 4, [(0, 2), (1, 3), (4, 6), (5, 7)], rng)
    # fp_sqr2 = fp_mul(a, 2a): 14 * 2 LBa^2 + ... < 2^63, LBa = L(2), and 2 VBa^2 <= 10^6
    elif name == "SQR2": v = product_vectors(name, 2, [(0, 0)], rng, square=True)
    elif name == "MUL_MSQR2": v = msqr2_vectors(rng)
    # one Fp product per coordinate against the same Fp operand: LBx.a LBs, LBx.b LBs at L(1)^2
    elif name in ("FP2_MUL_FP", "FP2_CONJ_MUL_CI"): v = product_vectors(name, 1, [(0, 2), (1, 2)], rng)
    # the product operand y.a -+ y.b has limb bound 2 LB(y) and value bound 2 VB(y): 14 * 2 LB(y) LB(a) + ... < 2^63 is the inequality of TWO
    # products, LB(y) LB(a) = L(2)^2, and y.a -+ y.b must fit int32: LB(y) <= 2^30 - 1.  k0 = neg alternates.
    elif name == "FP2_CONJ_MUL_A1MI": v = product_vectors(name, 2, [(0, 2), (1, 2)], rng, extra=neg_extra(), amax=(1 << 30) - 1)
    elif name == "FP2_NORM1_DBL": v = paired("NORM1_DBL")
    elif name == "FP2_CONJ": v = lazy_vectors(rng, [(T31,)])
    # the two-lane ops run the vectors of their whole-element counterparts wherever the preconditions agree (the product pairs of the lane
    # routines are those of fp2_mul / fp2_mul2; the limits of both halves of an operand are equal in these sets, so fp_select's declared
    # maximum changes nothing) ...
    elif name in ("FH2_MUL", "FH2_MUL2_ADD", "FH2_MUL2_SUB", "FH2_MUL_IP", "FH2_MUL_FP", "FH2_CONJ_MUL_CI", "FH2_CONJ_MUL_A1MI", "FH2_CONJ"):
        v = vectors("FP2_" + name[4:])
    elif name in ("FP2_CONJ_MUL_NEG_I", "FH2_CONJ_MUL_NEG_I"): v = vectors("FP2_CONJ")
    # ... and FH2_SQR does not: fp2_sqr sums a^2 and b^2 (2 LB^2, L(2)), fp2h_lane_sqr multiplies (a + b)(a - b) and (2b) a: both factors have
    # limb bound 2 LB, so 14 * 4 LB^2 + 14 2^56 + 2^40 < 2^63: LB = L(4) = 382999548, the "2^28.5" of fp2h.hpp (2^28.5 = 379625062 is just
    # below it), and value bound 2 VB each: 4 VB^2 <= 10^6, VB = 500
    elif name == "FH2_SQR":
        assert limb_limit(4) == 382999548 and 2 ** 57 <= limb_limit(4) ** 2 < 2 ** 57 * 1.02
        v = product_vectors(name, 4, [(0, 0), (1, 1)], rng, square=True)
    elif name == "FH2_NORM1": v = paired("NORM1")
    elif name == "FH2_MUL_SMALL": v = paired("MUL_SMALL")
    elif name == "FH2_NEG": v = lazy_vectors(rng, [(T31,)])
    elif name == "FH2_SELECT": v = lazy_vectors(rng, [(T31, T31)], ks=(1, 0))
    elif name == "FH2_DBL": v = lazy_vectors(rng, [((1 << 30) - 1,)])
    elif name in ("FH2_ADD", "FH2_SUB"): v = lazy_vectors(rng, [((1 << 30) - 1, 1 << 30), (T31 - (1 << LB), 1 << LB), (1 << LB, T31 - (1 << LB))])
    elif name == "FH2_IS_ZERO": v = fh2_is_zero_vectors(rng)
    elif name == "FH2_ONE": v = [Vec([]) for _ in range(40)]                        # no operand: the lanes differ by their role alone
    elif name == "QUOT_TOP": v = quot_top_vectors(rng)
    elif name in ("NORM1", "NORM1_DBL", "MUL_SMALL", "WEAK_REDUCE", "LINCOMB3P", "FP2_MUL_IP"): v = carry_vectors(name, rng)
    else: v = predicate_vectors(name, rng)
    for vec in v:
        assert len(vec.x) == ARITY[name]
        assert_precondition(name, vec)
    assert len(v) == COUNTS[name], (name, len(v), COUNTS[name])
    if forms_of(name, [0, 0, 0, 0]):
        # the set stands AT the limits: some vector has sum VBa VBb within 0.2 % of the cap 10^6 (whole top limbs: 1000 p is 1.07e8 of
        # them) and some vector's declared limb limits put the column bound within 10^-6 of 2^63
        rv, rc = max(reach(name, vec)[0] for vec in v), max(reach(name, vec)[1] for vec in v)
        assert 0.998 <= rv <= 1.0 and 0.999999 <= rc < 1.0, (name, rv, rc)
    _CACHE[name] = v
    return v


ALL_OPS = [n for fam in FAMILIES.values() for n in fam]


def pack(name, vecs):
    """(limbs int32 bytes, declared bounds float64 bytes, multipliers int32 bytes)"""
    import numpy as np
    ar = ARITY[name]
    limbs = np.array([o.l for v in vecs for o in v.x], dtype=np.int64).reshape(-1) if ar else np.zeros(NL * len(vecs), dtype=np.int64)
    assert limbs.size == 0 or (limbs.min() >= -(1 << 31) and limbs.max() <= T31)
    bnd = np.array([[o.lb, o.vb] for v in vecs for o in v.x], dtype=np.float64).reshape(-1) if ar else np.zeros(2, dtype=np.float64)
    k = np.array([v.k for v in vecs], dtype=np.int64).reshape(-1)
    return limbs.astype(np.int32).tobytes(), bnd.tobytes(), k.astype(np.int32).tobytes()


def unpack(name, raw, n):
    import numpy as np
    a = np.frombuffer(raw, dtype=np.int32).reshape(n, OUTPUTS[name], NL)
    return a.tolist()


# ---------------------------------------------------------------- closure: post-conditions as invariants
CLOSURE_LANES = 8


def closure(run, steps, seed=20260):
    """From the worst-case outputs of fp_mul, `steps` rounds of lazy add / sub / neg up to the limb limit of one product (a carry round
    when the next addition would pass it) and fp_sqr / fp_mul (whenever an addition would pass 1000 p, so that VBa VBb stays under the
    cap); every step's raw limbs are compared with the prediction, the canonical end values with the residues tracked modulo p.
    run(name, vecs) -> raw outputs per vector.  Returns the number of steps of each kind."""
    rng = random.Random(seed)
    L = limb_limit(1)
    # the corner by construction: limbs 0..12 at +-L(1) in the four sign patterns, top limbs at +-1000 p / 2^364 (VBa VBb = 10^6)
    start = [Vec([operand(pa, L, ("cap", 1000, s), rng), operand(pb, L, ("cap", 1000, -s), rng)])
             for pa, pb in (("pos", "neg"), ("neg", "neg"), ("alt", "alt-"), ("alt-", "pos")) for s in (1, -1)]
    assert len(start) == CLOSURE_LANES
    for v in start:
        assert_precondition("MUL", v)
        for o in v.x:
            assert all(abs(t) == L for t in o.l[:NL - 1]) and max(abs(t) for t in o.l) == L and 999 * P < abs(o.v) <= 1000 * P

    def step(name, vecs):
        outs = run(name, vecs)
        for v, o in zip(vecs, outs):
            check_outputs(name, v, o)
        return [Operand(o[0]) for o in outs]

    x = step("MUL", start)
    y = [v.x[0] for v in start]
    rx = [(v.x[0].v * v.x[1].v * RINV) % P for v in start]
    ry = [o.v % P for o in y]
    kinds = {}
    for _ in range(steps):
        want = rng.choice(["ADD", "ADD", "ADD", "SUB", "SUB", "SUB", "NEG", "NEG", "MUL", "SQR"])
        lbx, lby = max(max(abs(t) for t in o.l) for o in x), max(max(abs(t) for t in o.l) for o in y)
        vx, vy = max(abs(o.v) for o in x), max(abs(o.v) for o in y)
        if want in ("ADD", "SUB") and vx + vy > 1000 * P:
            want = "MUL"
        if want in ("ADD", "SUB") and lbx + lby > L:
            want = "NORM1"
        if want == "NORM1" and lbx < lby:
            x, y, rx, ry = y, x, ry, rx
        kinds[want] = kinds.get(want, 0) + 1
        if want in ("ADD", "SUB", "MUL"):
            new = step(want, [Vec([a, b]) for a, b in zip(x, y)])
            rn = [(a + b) % P if want == "ADD" else (a - b) % P if want == "SUB" else a * b * RINV % P for a, b in zip(rx, ry)]
        else:
            new = step(want, [Vec([a]) for a in x])
            rn = [(-a) % P if want == "NEG" else a * a * RINV % P if want == "SQR" else a for a in rx]
        for o, r in zip(new, rn):
            assert o.v % P == r
        if want == "NORM1":
            x, rx = new, rn
        else:
            x, y, rx, ry = new, x, rn, rx
    for name, ops, rs in (("CANON", x, rx), ("CANON", y, ry)):
        outs = run(name, [Vec([o]) for o in ops])
        for o, r in zip(outs, rs):
            assert o[0] == to_limbs(r * RINV % P)
    return kinds


def closure_fp2h(run, steps, seed=20261):
    """The same for Fp2 through the two-lane ops, mixed as g2_add and g2_dbl mix them: from the worst-case outputs of FH2_MUL2_ADD (every
    operand limb at +-L(4), every value at +-500 p: its column inequality and 4 * 500^2 = the cap), `steps` rounds of lazy add / sub / neg /
    dbl / conj / mul_ip and mul_small, a carry round (FH2_NORM1) when a lazy result would pass L(1) or the next product's own limb limit, and
    mul / sqr / mul2 (x y + y x and x x - y y; always when a lazy result would pass 500 p, which keeps every product under the value cap).
    Every step's raw limbs are compared with the prediction, the canonical end values with the residues tracked in Fp2.
    run(name, vecs) -> raw outputs per vector.  Returns the number of steps of each kind."""
    rng = random.Random(seed)
    L1, L4, VMAX = limb_limit(1), limb_limit(4), 500
    start = [Vec([operand(p_, L4, ("cap", VMAX, s if j % 3 else -s), rng) for j, p_ in enumerate(pats)])
             for pats in (("pos", "neg", "pos", "alt", "neg", "pos", "alt-", "neg"), ("alt", "alt-", "neg", "neg", "pos", "alt", "alt", "pos")) for s in (1, -1)
             for pats in (pats, pats[::-1])]
    assert len(start) == CLOSURE_LANES
    for v in start:
        assert_precondition("FH2_MUL2_ADD", v)
        assert reach("FH2_MUL2_ADD", v)[1] >= 0.999999
        for o in v.x:
            assert all(abs(t) == L4 for t in o.l[:NL - 1]) and (VMAX - 1) * P < abs(o.v) <= VMAX * P

    def step(name, vecs):
        outs = run(name, vecs)
        for v, o in zip(vecs, outs):
            check_outputs(name, v, o)
        return [(Operand(o[0]), Operand(o[1])) for o in outs]

    def mulr(u, v):                       # Montgomery product of residues in Fp2
        return ((u[0] * v[0] - u[1] * v[1]) * RINV % P, (u[0] * v[1] + u[1] * v[0]) * RINV % P)

    x = step("FH2_MUL2_ADD", start)
    y = [(v.x[0], v.x[1]) for v in start]
    rx = [tuple(t % P for t in (v.x[0].v * v.x[2].v - v.x[1].v * v.x[3].v + v.x[4].v * v.x[6].v - v.x[5].v * v.x[7].v,
                                v.x[0].v * v.x[3].v + v.x[1].v * v.x[2].v + v.x[4].v * v.x[7].v + v.x[5].v * v.x[6].v)) for v in start]
    rx = [(a * RINV % P, b * RINV % P) for a, b in rx]
    ry = [(a.v % P, b.v % P) for a, b in y]
    lazy = {"FH2_ADD": 1, "FH2_SUB": 1, "FH2_NEG": 0, "FH2_CONJ": 0, "FH2_DBL": 0, "FH2_MUL_IP": 0, "FH2_MUL_SMALL": 0}
    prods = ["FH2_MUL", "FH2_SQR", "FH2_MUL2_ADD", "FH2_MUL2_SUB"]
    kinds = {}
    for _ in range(steps):
        want = rng.choice(["FH2_ADD", "FH2_ADD", "FH2_SUB", "FH2_SUB", "FH2_NEG", "FH2_CONJ", "FH2_DBL", "FH2_MUL_IP", "FH2_MUL_SMALL"] + prods)
        kk = rng.choice([2, 3])
        lbx, lby = (max(abs(t) for e in ops for o in e for t in o.l) for ops in (x, y))
        vx, vy = (max(abs(o.v) for e in ops for o in e) for ops in (x, y))
        if want in lazy:
            # what the lazy result may reach: (limb, value)
            lb_new, v_new = {"FH2_ADD": (lbx + lby, vx + vy), "FH2_SUB": (lbx + lby, vx + vy), "FH2_NEG": (lbx, vx), "FH2_CONJ": (lbx, vx), "FH2_DBL": (2 * lbx, 2 * vx),
                             "FH2_MUL_IP": (2 * lbx, 2 * vx), "FH2_MUL_SMALL": (0, kk * vx)}[want]
            if v_new > VMAX * P:
                want = rng.choice(prods)
            elif lb_new > L1:
                want = "FH2_NORM1"
                if lbx < lby:
                    x, y, rx, ry, lbx, lby = y, x, ry, rx, lby, lbx
        if want in prods:
            # the product's own limb limit (forms_of): mul 2 LBx LBy, sqr 4 LBx^2, x y + y x 4 LBx LBy, x x - y y 2 LBx^2 + 2 LBy^2, all <= L(1)^2
            need = {"FH2_MUL": 2 * lbx * lby, "FH2_SQR": 4 * lbx * lbx, "FH2_MUL2_ADD": 4 * lbx * lby, "FH2_MUL2_SUB": 2 * lbx * lbx + 2 * lby * lby}[want]
            if not col_ok(need):
                want = "FH2_NORM1"
                if lbx < lby:
                    x, y, rx, ry = y, x, ry, rx
        kinds[want] = kinds.get(want, 0) + 1
        if want in ("FH2_ADD", "FH2_SUB", "FH2_MUL"):
            vecs = [Vec([a[0], a[1], b[0], b[1]]) for a, b in zip(x, y)]
            rn = [tuple((s + t) % P for s, t in zip(a, b)) if want == "FH2_ADD" else tuple((s - t) % P for s, t in zip(a, b)) if want == "FH2_SUB" else mulr(a, b)
                  for a, b in zip(rx, ry)]
        elif want == "FH2_MUL2_ADD":
            vecs = [Vec([*a, *b, *b, *a]) for a, b in zip(x, y)]
            rn = [tuple(2 * t % P for t in mulr(a, b)) for a, b in zip(rx, ry)]
        elif want == "FH2_MUL2_SUB":
            vecs = [Vec([*a, *a, *b, *b]) for a, b in zip(x, y)]
            rn = [tuple((s - t) % P for s, t in zip(mulr(a, a), mulr(b, b))) for a, b in zip(rx, ry)]
        else:
            vecs = [Vec([*a], [kk]) for a in x]
            rn = [{"FH2_NEG": ((-a) % P, (-b) % P), "FH2_CONJ": (a, (-b) % P), "FH2_DBL": (2 * a % P, 2 * b % P), "FH2_MUL_IP": ((a - b) % P, (a + b) % P),
                   "FH2_MUL_SMALL": (kk * a % P, kk * b % P), "FH2_SQR": mulr((a, b), (a, b)), "FH2_NORM1": (a, b)}[want] for a, b in rx]
        for v in vecs:
            assert_precondition(want, v)
        new = step(want, vecs)
        for o, r in zip(new, rn):
            assert (o[0].v % P, o[1].v % P) == r, want
        if want == "FH2_NORM1":
            x, rx = new, rn
        else:
            x, y, rx, ry = new, x, rn, rx
    for ops, rs in ((x, rx), (y, ry)):
        for h in (0, 1):
            outs = run("CANON", [Vec([e[h]]) for e in ops])
            for o, r in zip(outs, rs):
                assert o[0] == to_limbs(r[h] * RINV % P)
    return kinds
