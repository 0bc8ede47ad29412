"""Constructed inputs for the G1 bucket product (msm.hpp, the msm_* kernels of k_g1.hip): degenerate bucket contents, results at infinity,
chosen digits, edge scalars, run lengths at the seams of the overflow cut, the small-scalar bucket, and the switches of width and path.
Plain Python integers, shared by the host-sim, oracle and GPU tests; no input comes from a kernel.

Points.  A pool of 64 subgroup points P_i = [a_i]G with their negatives and their images psi(P_i) = [x^2 mod r]P_i = (beta x, -y); every
subgroup point a case uses is registered with its multiplier of G (MULT), so the expected value of a subgroup-only case is ONE
multiplication [sum a_i (k_i mod r) mod r]G.  Cases with points outside G1 ((0, +-2), an order-11 point, the order-10177 eigenpoint,
G + (0, 2)) expect the oracle's chain of multiply() results ("oracle"): the [r]phi(P) term of a scalar below x^2 is defined there.

Scalars are built from chosen halves, k = k0 + k1 x^2 with k0 < x^2 and k < r (sc): with digits() this restates scalar_glv_split and
msm_digit, so a case can say which bucket every entry lands in.  model() restates msm_window_bits, msm_windows, msm_run_cap and the segment
arithmetic of msm_sizes_kernel; run_order() the order of the records inside a run (the sorts are stable: the k0-halves in term order, then
the k1-halves).  They serve to choose run lengths and to assert, at the bottom of this module, that every seam is hit."""
import functools

from g1_torsion import BETA, X2, dec, ec_add, ec_mul, ec_neg, eigenpoint, enc, endo, generator, point_of_order
from util import P, R, prng

SMALL_EARLY_MAX = 4096                              # kernels.hpp MSM_SMALL_EARLY_MAX: a small-scalar bucket up to this length is summed apart
MSM_CHUNK = 8                                       # msm.hpp: buckets per lane of the window reduction
ORACLE = "oracle"
FAMILIES = ("a", "b", "c", "d", "e", "f", "g")


# ---------------------------------------------------------------- the model of the cut
def window_bits(n):
    return 16 if n >= 4096 else 8


def windows(c):
    return (128 + c - 1) // c


def run_cap(n, c):
    return 2 * ((2 * n) >> c) + 32


def params(n):
    c = window_bits(n)
    return c, windows(c), run_cap(n, c)


def split(k):
    """(k0, k1) of k mod r: k mod r = k0 + k1 x^2, k0 < x^2"""
    k1, k0 = divmod(k % R, X2)
    return k0, k1


def digits(k, c):
    """the c-bit window digits of the two halves of k mod r, lowest window first (the top window of c = 7 has 2 bits, none past bit 128)"""
    k0, k1 = split(k)
    assert k0 < 1 << 128 and k1 < 1 << 128
    m = (1 << c) - 1
    return [(k0 >> (w * c)) & m for w in range(windows(c))], [(k1 >> (w * c)) & m for w in range(windows(c))]


def segments(length, cap):
    """overflow segments of a run: none up to cap entries, then ceil((length - cap) / (cap // 2))"""
    sl = cap // 2
    return 0 if length <= cap else (length - cap + sl - 1) // sl


def model(n, scalars, usable=None, c=None):
    """What the bookkeeping makes of a product: {"c", "W", "cap", "sl", "runs": {(w, d): length}, "small": length of the small-scalar
    bucket, "cut": {(w, d) or "small": number of segments}, "segments": their total}.  usable[i] = False for a term whose point is
    infinity (all its digits count as 0).  The small-scalar bucket is summed apart while it has at most SMALL_EARLY_MAX entries."""
    assert len(scalars) == n
    c = c or window_bits(n)
    W, cap = windows(c), run_cap(n, c)
    runs, small = {}, 0
    for i, k in enumerate(scalars):
        if usable is not None and not usable[i]:
            continue
        d0, d1 = digits(k, c)
        small += split(k)[1] == 0
        for w in range(W):
            for d in (d0[w], d1[w]):
                if d:
                    runs[(w, d)] = runs.get((w, d), 0) + 1
    cut = {b: segments(ln, cap) for b, ln in runs.items() if ln > cap}
    if small > SMALL_EARLY_MAX and small > cap:
        cut["small"] = segments(small, cap)
    return {"c": c, "W": W, "cap": cap, "sl": cap // 2, "runs": runs, "small": small, "cut": cut, "segments": sum(cut.values())}


def run_order(scalars, w, d, c=8):
    """the records of bucket (w, d) in the order the bucket lane meets them: (term, half), half 1 = the record (beta x, -y)"""
    dg = [digits(k, c) for k in scalars]
    return [(i, h) for h in (0, 1) for i in range(len(scalars)) if dg[i][h][w] == d]


# ---------------------------------------------------------------- points
MULT = {None: 0}                                    # subgroup point (affine, None = infinity) -> its multiple of G


def _reg(pt, a):
    assert MULT.setdefault(pt, a % R) == a % R
    return pt


G = _reg(generator(), 1)
A = [prng(9801, i) % (R - 1) + 1 for i in range(64)]
POOL = [_reg(ec_mul(a, G), a) for a in A]
NEG = [_reg(ec_neg(p), -a) for p, a in zip(POOL, A)]
PSI = [_reg(ec_mul(X2 % R, p), X2 * a) for p, a in zip(POOL, A)]
# the beta of msm_prep_one (FP_BETA_A: P' = (beta x, -y) = [x^2]P), not its square
assert all(q == (BETA * p[0] % P, (-p[1]) % P) == endo(p) for p, q in zip(POOL, PSI))
assert all(q != (BETA * BETA % P * p[0] % P, (-p[1]) % P) for p, q in zip(POOL, PSI))
NPSI = [_reg(ec_neg(p), -X2 * a) for p, a in zip(PSI, A)]
_SHIFT = prng(9802, 0) % (R - 1) + 1
_D = ec_mul(_SHIFT, G)
MORE = [_reg(ec_add(p, _D), a + _SHIFT) for p, a in zip(POOL, A)]       # 64 further distinct points for the run-length cases
ALL_SUB = POOL + NEG + PSI

T3, T3N = (0, 2), (0, P - 2)                        # order 3: (beta x, -y) of (0, 2) is its negative
O11 = point_of_order(11)
TE = eigenpoint(10177)[0]
GT3 = ec_add(G, T3)
TORSION = {"T3": T3, "-T3": T3N, "o11": O11, "te": TE, "G+T3": GT3}
assert endo(T3) == T3N and all(t not in MULT for t in TORSION.values())

K1_MAX = (R - 1) // X2                              # the largest k1
TOP0 = (X2 - 1) >> 120                              # the largest digit of the top 8-bit window of k0 ...
TOP1 = K1_MAX >> 120                                # ... and of k1
assert (TOP1 << 120) < K1_MAX


def sc(k0, k1=0):
    """the scalar with the halves k0, k1"""
    k = k0 + k1 * X2
    assert 0 <= k0 < X2 and 0 <= k1 and k < R and split(k) == (k0, k1)
    return k


def from_digits(ds, c=8):
    return sum(d << (c * w) for w, d in enumerate(ds))


def one_digit(w, d, c=8):
    return d << (c * w)


def pattern(j):
    """128-bit halves whose 8-bit digits are non-zero in every window and pairwise different from those of every other j < 8"""
    return from_digits([16 + 13 * j + (7 * w) % 11 for w in range(16)])


assert all(len({(pattern(j) >> (8 * w)) & 255 for j in range(8)}) == 8 for w in range(16)) and pattern(7) < min(X2, K1_MAX)


# ---------------------------------------------------------------- cases
class Case:
    def __init__(self, name, points, scalars, note="", cancelling=False):
        assert len(points) == len(scalars) and all(0 <= k < 1 << 256 for k in scalars)
        self.name, self.family, self.points, self.scalars, self.note, self.cancelling = name, name[0], list(points), list(scalars), note, cancelling
        self.n = len(points)
        self.tiles, self.tile_len = 1, self.n                     # width_case: the first tiles * tile_len terms repeat the first tile_len
        self.subgroup_only = all(p in MULT for p in points)

    @functools.cached_property
    def expected(self):
        """the 96-byte value from integers, or ORACLE"""
        if not self.subgroup_only:
            return ORACLE
        return enc(ec_mul(sum(MULT[p] * (k % R) for p, k in zip(self.points, self.scalars)) % R, G))

    @property
    def source(self):
        return "oracle" if self.expected == ORACLE else "integers"

    @property
    def path(self):
        if self.n < 2:
            return "naive"
        return "16-bit keys" if self.n >= 1 << 15 else "32-bit keys c=%d" % window_bits(self.n)

    def pack(self):
        return b"".join(_enc(p) for p in self.points), b"".join(k.to_bytes(32, "big") for k in self.scalars)

    def model(self, c=None):
        return model(self.n, self.scalars, [p is not None for p in self.points], c)


@functools.lru_cache(maxsize=None)
def _enc(p):
    return enc(p)


def enc49(b96):
    """the compressed form of a 96-byte value: tag 02 | parity of y, then x; infinity = 49 zero bytes"""
    return bytes(49) if b96 == bytes(96) else bytes([2 | (b96[95] & 1)]) + b96[:48]


def _seeded(seed, n):
    pts = [ALL_SUB[prng(seed, i, 8) % len(ALL_SUB)] for i in range(n)]
    return pts, [prng(seed + 1, i, 32) for i in range(n)]


def _family_a():
    p, q, s = POOL[0], POOL[1], POOL[2]
    k = sc(pattern(0), pattern(1))
    out = [Case("a:P,P", [p, p], [k, k], "one bucket adds a point to itself"),
           Case("a:P,-P", [p, NEG[0]], [k, k], "every bucket sums to infinity", True),
           Case("a:P,-P,Q", [p, NEG[0], q], [k, k, k], "an addition after the accumulator became infinity", True),
           Case("a:P,P,-P", [p, p, NEG[0]], [k, k, k], "", True),
           Case("a:P,P,P,P", [p] * 4, [k] * 4),
           Case("a:n=8", [p, p, NEG[0], NEG[0], q, q, q, NEG[1]], [k] * 8, "2Q after P + P - P - P", True)]
    d = 37
    for name, ds in (("one-window", [d] + [0] * 15), ("all-windows", [(pattern(2) >> (8 * w)) & 255 for w in range(16)])):
        v = from_digits(ds)
        # P with (0, v) stores psi(P) under the digits of v; the term psi(P) with (v, 0) stores the same record under the same digits
        out.append(Case("a:psi-twice/" + name, [p, PSI[0], s], [sc(0, v), sc(v, 0), k], "the same record twice in one bucket"))
        out.append(Case("a:psi-cancels/" + name, [p, NPSI[0]], [sc(0, v), sc(v, 0)], "a record and its negative from two terms", True))
        out.append(Case("a:psi-cancels+Q/" + name, [p, NPSI[0], s], [sc(0, v), sc(v, 0), k], "", True))
        # (0, 2): the second record is the negative of the first, so equal digits of k0 and k1 cancel inside the bucket
        out.append(Case("a:T3-self/" + name, [T3, q], [sc(v, v), k], "k0-digit = k1-digit on the order-3 point", True))
        out.append(Case("a:T3-self-alone/" + name, [T3, T3N], [sc(v, v), sc(v, v)], "", True))
    kk = prng(9803, 0) % R
    out.append(Case("a:k,r-k", [p, p], [kk, R - kk], "the products cancel, no bucket does", True))
    out.append(Case("a:k,r-k,Q", [p, p, q], [kk, R - kk, k], "", True))
    return out


def _family_b():
    ks = [0, R, 2 * R, R, 0, 2 * R]
    rnd = [prng(9804, i, 32) for i in range(5)]
    k0, k1 = prng(9805, 0) % R, prng(9805, 1) % R
    k2 = -(A[0] * k0 + A[1] * k1) * pow(A[2], -1, R) % R
    k3 = prng(9805, 2) % R
    k4 = -(X2 * A[3] * k3) * pow(A[4], -1, R) % R
    return [Case("b:scalars-0-r-2r", POOL[:6], ks, "", True),
            Case("b:points-infinity", [None] * 5, rnd, "", True),
            Case("b:zero-scalars", POOL[:7], [0] * 7, "", True),
            Case("b:sum-zero/3", POOL[:3], [k0, k1, k2], "", True),
            Case("b:sum-zero/5", POOL[:3] + [PSI[3], POOL[4]], [k0, k1, k2, k3, k4], "", True),
            Case("b:infinity-among-points", [POOL[0], None, NEG[0], None], [k0, k1, k0, k3], "", True)]


def _family_c():
    out = []
    for d in (255, 1, 7, 8, 9, 248):
        pts, ks = [], []
        for h in (0, 1):
            for w in range(16):
                if w == 15 and d > (TOP0, TOP1)[h]:
                    continue                                      # no such scalar: the half would pass x^2 (or k would pass r)
                v = one_digit(w, d)
                pts.append(ALL_SUB[(16 * h + w) * 3 % len(ALL_SUB)])
                ks.append(sc(v, 0) if h == 0 else sc(0, v))
        out.append(Case("c:single-%d" % d, pts, ks, "one term per (half, window) with this digit alone"))
    pts, ks = [], []
    for j in range(1, 32):                                        # a digit on each side of every chunk boundary of the window reduction
        for d in (MSM_CHUNK * j - 1, MSM_CHUNK * j):
            w, h = j % 15, j & 1
            pts.append(ALL_SUB[(5 * len(ks) + 1) % len(ALL_SUB)])
            ks.append(sc(one_digit(w, d), 0) if h == 0 else sc(0, one_digit(w, d)))
    out.append(Case("c:chunk-seams", pts, ks, "digits 8j - 1 and 8j for every j"))
    t0, t1 = one_digit(15, TOP0), one_digit(15, TOP1)
    out.append(Case("c:top-window-only", POOL[:4], [sc(t0, 0), sc(0, t1), sc(t0, t1), sc(t0, t1)], "the largest top digits, nothing below"))
    full0, full1 = from_digits([255] * 15 + [TOP0 - 1]), from_digits([255] * 15 + [TOP1 - 1])
    out.append(Case("c:all-255/k0", POOL[4:7], [sc(full0, 0)] * 2 + [sc(full0 - 1, 0)], "only the last bucket of every window, k1 = 0"))
    out.append(Case("c:all-255/k1", POOL[7:10], [sc(0, full1)] * 2 + [sc(0, full1 - 1)], "only the last bucket of every window, k0 = 0"))
    out.append(Case("c:all-1", POOL[10:14], [sc(from_digits([1] * 16), 0), sc(0, from_digits([1] * 16))] * 2, "only bucket 1 of every window"))
    vs = [pattern(j) for j in range(4)]
    out.append(Case("c:k0=k1", ALL_SUB[20:28], [sc(v, v) for v in vs + vs], "every run holds both halves of its terms"))
    return out


EDGE = [("0", 0), ("1", 1), ("x2-1", X2 - 1), ("x2", X2), ("x2+1", X2 + 1), ("r-1", R - 1), ("r", R), ("r+1", R + 1), ("2r", 2 * R),
        ("2^256-1", (1 << 256) - 1), ("2^255", 1 << 255)]


def _family_d():
    out = [Case("d:batch", POOL[30:30 + len(EDGE)], [k for _, k in EDGE])]
    out += [Case("d:one/" + name, [POOL[30 + i]], [k], "a single term: the scalar-multiplication route") for i, (name, k) in enumerate(EDGE)]
    return out


def _fill(n, groups):
    """scalars of n terms whose 2n halves (k0 of term 0 .. n-1, then k1 of term 0 .. n-1) take the patterns of `groups` = [(count, j)]"""
    halves = [pattern(j) for count, j in groups for _ in range(count)]
    assert len(halves) == 2 * n
    return [sc(halves[i], halves[n + i]) for i in range(n)]


E_N = 120
E_CAP, E_SL = run_cap(E_N, 8), run_cap(E_N, 8) // 2
# runs of cap, cap + 1, cap + sl, cap + sl + 1, cap + 2 sl entries in every window (patterns 1 .. 5) and one of 14 that holds both halves of
# its terms (pattern 6).  226 entries need more than 120 equal scalars, so a group is a group of equal HALVES: the k0 of terms 0 .. 63 is
# pattern 5 (the run in term order: the bucket lane takes terms 0 .. 31, the segments terms 32 .. 47 and 48 .. 63)
E_GROUPS = [(E_CAP + 2 * E_SL, 5), (E_CAP + E_SL + 1, 4), (7, 6), (E_CAP, 1), (E_CAP + 1, 2), (E_CAP + E_SL, 3), (7, 6)]
E_SEAMS = {1: 0, 2: 1, 3: E_SL, 4: E_SL + 1, 5: 2 * E_SL}             # pattern -> intended run length - cap


def _family_e():
    base_pts = POOL + MORE[:E_N - 64]
    assert len(set(base_pts)) == E_N
    ks = _fill(E_N, E_GROUPS)
    out = [Case("e:seams", base_pts, ks, "runs of cap, cap+1, cap+sl, cap+sl+1, cap+2sl; distinct points")]
    pairs = [x for i in range(E_SL // 2) for x in (MORE[63 - i], _reg(ec_neg(MORE[63 - i]), -MULT[MORE[63 - i]]))]
    out.append(Case("e:seams/segment-infinity", base_pts[:E_CAP] + pairs + base_pts[E_CAP + E_SL:], ks,
                    "the first overflow segment of the longest run is P, -P pairs", True))
    out.append(Case("e:seams/equal-segments", base_pts[:E_CAP + E_SL] + base_pts[E_CAP:E_CAP + E_SL] + base_pts[E_CAP + 2 * E_SL:], ks,
                    "both overflow segments of the longest run hold the same points"))
    three = [(E_CAP + 2 * E_SL + 1, 1), (E_CAP + 2 * E_SL + 2, 2), (E_CAP + 3 * E_SL, 3)]
    three.append((2 * E_N - sum(cnt for cnt, _ in three), 4))
    out.append(Case("e:straddle", base_pts, _fill(E_N, three), "48 cut buckets of three segments each: 144 list entries"))
    n, m = 3000, 2600
    k = sc(pattern(1), pattern(2))
    spts, sks = _seeded(9810, n - m)
    out.append(Case("e:long-run", [POOL[i % 64] for i in range(m)] + spts, [k] * m + sks, "2600 equal scalars: more than 64 segments per bucket"))
    return out


def _family_f():
    p, q = POOL[40], POOL[41]
    big = sc(pattern(3), pattern(4))
    return [Case("f:S-infinity/P,-P", [p, NEG[40]], [3, 5], "S = infinity, the product is not", True),
            Case("f:S-infinity/T3,-T3", [T3, T3N], [4, 7], "every term small, S = infinity", True),
            Case("f:S-infinity/T3,-T3,Q", [T3, T3N, q], [4, 7, big], "", True),
            Case("f:S-in-G1", [p, q, PSI[3]], [3, X2 - 1, 1 << 100]),
            Case("f:S-outside/T3", [T3, p], [5, 6]),
            Case("f:S-outside/G+T3", [GT3, p], [X2 - 1, 6]),
            Case("f:S-outside/o11", [O11, p, TE], [2, 6, 10]),
            Case("f:S-outside/sum-of-two", [T3, O11, p], [1, 1, big], "S = T3 + o11"),
            Case("f:one-small-among-large", [p, q, POOL[42], POOL[43], POOL[44], POOL[45]], [big, big + 1, 77, big + 2, big + X2, R - 1]),
            Case("f:one-small-among-large/G+T3", [p, q, GT3, O11, TE, POOL[45]], [big, big + 1, 77, big + 2, big + X2, R - 1],
                 "only G + T3 owes the extra term"),
            Case("f:x2-1-small,x2-not", [GT3, GT3, O11, O11, TE, TE, T3, T3], [X2 - 1, X2] * 4, "the boundary of the small-scalar bucket")]


@functools.lru_cache(maxsize=None)
def small_cases():
    """the cases of families (a) .. (f), in order"""
    out = _family_a() + _family_b() + _family_c() + _family_d() + _family_e() + _family_f()
    assert len({c.name for c in out}) == len(out)
    return out


def union_terms():
    """the terms of (a), (c), (d: the batch), (f) one after the other"""
    cs = [c for c in small_cases() if c.family in "acf" or c.name == "d:batch"]
    return [p for c in cs for p in c.points], [k for c in cs for k in c.scalars]


G_SIZES = {"g:n=4095": 4095, "g:n=4096": 4096, "g:n=2^15": 1 << 15}


@functools.lru_cache(maxsize=None)
def width_case(name):
    """the union tiled over three quarters of n terms, seeded terms behind it"""
    n = G_SIZES[name]
    up, uk = union_terms()
    reps = (3 * n // 4) // len(up)
    assert reps >= 2
    sp, sk = _seeded(9820 + n % 97, n - reps * len(up))
    c = Case(name, up * reps + sp, uk * reps + sk, "(a), (c), (d), (f) tiled %d times, then seeded terms" % reps)
    c.tiles, c.tile_len = reps, len(up)
    return c


NAMES = [c.name for c in small_cases()] + list(G_SIZES)


def case(name):
    return width_case(name) if name in G_SIZES else next(c for c in small_cases() if c.name == name)


_EXPECTED = {}


def expected96(name, oracle, nthreads=8):
    """the 96-byte expected value of a case: from integers where it has only subgroup points, else the CPU oracle's chain (computed once)"""
    if name not in _EXPECTED:
        c = case(name)
        if c.expected != ORACLE and c.tiles == 1:
            _EXPECTED[name] = c.expected
        elif c.tiles == 1:
            _EXPECTED[name] = oracle.g1_msm(*c.pack(), 96, nthreads)
        else:
            # a tiled case: the product is a sum of multiply() results, so the terms outside G1 of ONE tile go to the oracle, its value
            # times the number of tiles joins the integer sum of all subgroup terms (test_msm_cases.py checks this against the whole chain)
            out = [(p, k) for p, k in zip(c.points[:c.tile_len], c.scalars[:c.tile_len]) if p not in MULT]
            assert all((p in MULT) == (i >= c.tiles * c.tile_len or c.points[i % c.tile_len] in MULT) for i, p in enumerate(c.points))
            part = dec(oracle.g1_msm(b"".join(_enc(p) for p, _ in out), b"".join(k.to_bytes(32, "big") for _, k in out), 96, nthreads))
            a = sum(MULT[p] * (k % R) for p, k in zip(c.points, c.scalars) if p in MULT) % R
            _EXPECTED[name] = enc(ec_add(ec_mul(a, G), ec_mul(c.tiles, part)))
    return _EXPECTED[name]


def family(f):
    return [n for n in NAMES if n[0] == f]


# ---------------------------------------------------------------- the lists hold every seam
def _coverage():
    """rows (case, bucket, cap, sl, length, segments) of the cut buckets of family (e), after asserting what the families promise"""
    cs = small_cases()
    for f in FAMILIES:
        assert family(f), f
    rows = []
    # (e) the five seams, in every window
    by = {c.name: c for c in cs}
    for name in ("e:seams", "e:seams/segment-infinity", "e:seams/equal-segments"):
        m = by[name].model()
        assert (m["c"], m["cap"], m["sl"]) == (8, 32, 16), m
        for j, over in E_SEAMS.items():
            for w in range(16):
                ln = m["runs"][(w, (pattern(j) >> (8 * w)) & 255)]
                assert ln - m["cap"] == over, (name, j, w, ln)
            d = pattern(j) & 255
            rows.append((name, "window 0 digit %d" % d, m["cap"], m["sl"], m["runs"][(0, d)], segments(m["runs"][(0, d)], m["cap"])))
        assert m["runs"][(0, pattern(6) & 255)] == 14 and len(m["cut"]) == 4 * 16 and m["segments"] == 6 * 16
    # the twins: the order of the longest run, its first segment and its total
    d5 = pattern(5) & 255
    for name, want in (("e:seams/segment-infinity", "inf"), ("e:seams/equal-segments", "equal")):
        c = by[name]
        order = run_order(c.scalars, 0, d5)
        assert order == [(i, 0) for i in range(64)]
        mult = [MULT[c.points[i]] for i, _ in order]
        seg0, seg1 = mult[E_CAP:E_CAP + E_SL], mult[E_CAP + E_SL:E_CAP + 2 * E_SL]
        assert sum(mult) % R != 0 and sum(mult[:E_CAP]) % R != 0
        if want == "inf":
            assert sum(seg0) % R == 0 and all((seg0[i] + seg0[i + 1]) % R == 0 for i in range(0, E_SL, 2)) and sum(seg1) % R != 0
        else:
            assert seg0 == seg1 and len(set(seg0)) == E_SL
    assert len(set(by["e:seams"].points)) == E_N                    # distinct multipliers inside every run of the base case
    # more than 64 segments in all, every bucket with the same number that does not divide 64: some bucket's list straddles a multiple of 64
    m = by["e:straddle"].model()
    assert len(m["cut"]) >= 32 and set(m["cut"].values()) == {3} and 64 % 3 and m["segments"] > 64, m["cut"]
    for j in (1, 2, 3):
        d = pattern(j) & 255
        rows.append(("e:straddle", "window 0 digit %d" % d, m["cap"], m["sl"], m["runs"][(0, d)], m["cut"][(0, d)]))
    # one bucket with several heads in the combine step
    m = by["e:long-run"].model()
    assert (m["c"], m["cap"], m["sl"]) == (8, 78, 39) and max(m["cut"].values()) > 64 and sum(v > 64 for v in m["cut"].values()) >= 32
    b = max(m["cut"], key=lambda x: m["cut"][x])
    rows.append(("e:long-run", "window %d digit %d" % b, m["cap"], m["sl"], m["runs"][b], m["cut"][b]))
    assert sum(by["e:long-run"].scalars.count(k) for k in set(by["e:long-run"].scalars[:1])) >= 2600
    # (c) every named digit in some window of each half; the top-window digits are the largest there are
    seen = ({d for c in cs if c.family == "c" for k in c.scalars for d in digits(k, 8)[0]},
            {d for c in cs if c.family == "c" for k in c.scalars for d in digits(k, 8)[1]})
    for h in (0, 1):
        assert {1, 7, 8, 9, 248, 255} <= seen[h] and {MSM_CHUNK * j - e for j in range(1, 32) for e in (0, 1)} <= seen[0] | seen[1]
    assert sc(one_digit(15, TOP0), one_digit(15, TOP1)) < R and (TOP0 + 1) << 120 >= X2 and ((TOP1 + 1) << 120) * X2 >= R
    for c in cs:
        if c.name == "c:k0=k1":
            assert all(digits(k, 8)[0] == digits(k, 8)[1] and 0 not in digits(k, 8)[0] for k in c.scalars)
        if c.name == "c:top-window-only":
            assert all(not any(h[:15]) for k in c.scalars for h in digits(k, 8)) and any(digits(k, 8)[0][15] == TOP0 for k in c.scalars)
    # (d) and (f): the boundary of the small-scalar bucket
    assert split(X2 - 1)[1] == 0 and split(X2)[1] == 1 and {0, R, (1 << 256) - 1, 1 << 255} <= {k for _, k in EDGE}
    for c in cs:
        if c.family == "f":
            S = None
            for p, k in zip(c.points, c.scalars):
                S = ec_add(S, p) if split(k)[1] == 0 else S
            kind = "infinity" if S is None else ("in-G1" if ec_mul(R, S) is None else "outside")
            want = c.name[2:].split("/")[0]
            assert {"S-infinity": "infinity", "S-in-G1": "in-G1", "S-outside": "outside"}.get(want, kind) == kind, (c.name, kind)
    m = by["f:x2-1-small,x2-not"].model()
    assert m["small"] == 4 and by["f:one-small-among-large"].model()["small"] == 1
    # the cancelling cases: infinity and not
    inf = [c.name for c in cs if c.cancelling and c.subgroup_only and c.expected == bytes(96)]
    fin = [c.name for c in cs if c.cancelling and c.subgroup_only and c.expected != bytes(96)]
    assert len(inf) >= 3 and len(fin) >= 3, (inf, fin)
    assert all(c.expected == bytes(96) for c in cs if c.family == "b")
    assert all(c.n <= 8 for c in cs if c.family == "a") and sum(c.n == 1 for c in cs if c.family == "d") == len(EDGE)
    return rows


COVERAGE = _coverage()


def coverage_table():
    head = "%-28s %-22s %4s %3s %5s %3s" % ("case", "bucket", "cap", "sl", "len", "ns")
    return "\n".join([head] + ["%-28s %-22s %4d %3d %5d %3d" % r for r in COVERAGE])


def summary_table():
    """family, case, n, path, source of the expected value"""
    return "\n".join("%s  %-36s n=%-6d %-18s %s" % (case(n).family, n, case(n).n, case(n).path, case(n).source) for n in NAMES)


if __name__ == "__main__":
    print(coverage_table())
    print()
    print(summary_table())
