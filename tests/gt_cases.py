"""Fp12 on plain Python integers and the element lists of the GT tests (test_gt_cases.py, test_host_sim_gt_cases.py, test_gpu_gt_cases.py).

The GT entries (gt_op mul / conj / pow, fexp, gt_is_unity) take ANY 576 bytes as an element of Fp12; the rest of the suite feeds them pairing
values, Miller values, zero and one.  Here: every element class on which the three-lane code could go wrong unseen — basis elements (one
coefficient route of the product each), sparse and subfield elements (zero coefficients through lazy limbs, inversion and Frobenius),
unitary elements outside the cyclotomic subgroup (where the power's route choice shows in the bytes), non-canonical encodings (a coordinate
>= p counts mod p) and near-misses of one — and the lane patterns that place a special element in a wavefront of 21 triples.

The tower is the reference's: Fp2 = Fp[i], i^2 = -1;  Fp4 = Fp2[s], s^2 = 1 + i;  Fp12 = Fp4[w], w^3 = s.  An Fp2 is (a, b) = a + b i, an
Fp4 (a, b) = a + b s, an Fp12 (a, b, c) = a + b w + c w^2.  The bytes are c | b | a, each Fp4 as b | a, each Fp2 as b | a (FP12_toOctet,
include/c12381_hip.h): coordinate k of 0..11 is bytes 48 k .. 48 k + 47, so k = 11 is the Fp part a.a.a and e_11 = 1."""
import functools

from util import P, R, cat, golden, prng

# ------------------------------------------------------------------ Fp2, Fp4
F2_ZERO, F2_ONE = (0, 0), (1, 0)


def f2_add(x, y):
    return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)


def f2_sub(x, y):
    return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)


def f2_neg(x):
    return (-x[0] % P, -x[1] % P)


def f2_mul(x, y):
    return ((x[0] * y[0] - x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def f2_mul_ip(x):                       # times 1 + i
    return ((x[0] - x[1]) % P, (x[0] + x[1]) % P)


def f2_inv(x):
    n = pow(x[0] * x[0] + x[1] * x[1], -1, P)
    return (x[0] * n % P, -x[1] * n % P)


F4_ZERO, F4_ONE = (F2_ZERO, F2_ZERO), (F2_ONE, F2_ZERO)


def f4_add(x, y):
    return (f2_add(x[0], y[0]), f2_add(x[1], y[1]))


def f4_sub(x, y):
    return (f2_sub(x[0], y[0]), f2_sub(x[1], y[1]))


def f4_neg(x):
    return (f2_neg(x[0]), f2_neg(x[1]))


def f4_mul(x, y):
    return (f2_add(f2_mul(x[0], y[0]), f2_mul_ip(f2_mul(x[1], y[1]))), f2_add(f2_mul(x[0], y[1]), f2_mul(x[1], y[0])))


def f4_mul_s(x):                        # (a + b s) s = (1 + i) b + a s
    return (f2_mul_ip(x[1]), x[0])


def f4_inv(x):                          # 1 / (a + b s) = (a - b s) / (a^2 - (1 + i) b^2)
    n = f2_inv(f2_sub(f2_mul(x[0], x[0]), f2_mul_ip(f2_mul(x[1], x[1]))))
    return (f2_mul(x[0], n), f2_neg(f2_mul(x[1], n)))


# ------------------------------------------------------------------ Fp12
ZERO = (F4_ZERO, F4_ZERO, F4_ZERO)
ONE = (F4_ONE, F4_ZERO, F4_ZERO)


def add(x, y):
    return (f4_add(x[0], y[0]), f4_add(x[1], y[1]), f4_add(x[2], y[2]))


def mul(x, y):
    """schoolbook over Fp4 with w^3 = s: nine Fp4 products, no shared subexpressions (the device code's Karatsuba is what is under test)"""
    a = f4_add(f4_mul(x[0], y[0]), f4_mul_s(f4_add(f4_mul(x[1], y[2]), f4_mul(x[2], y[1]))))
    b = f4_add(f4_add(f4_mul(x[0], y[1]), f4_mul(x[1], y[0])), f4_mul_s(f4_mul(x[2], y[2])))
    c = f4_add(f4_add(f4_mul(x[0], y[2]), f4_mul(x[1], y[1])), f4_mul(x[2], y[0]))
    return (a, b, c)


def conj(x):
    """FP12_conj: the Fp4 conjugate a - b s on the coefficients of 1 and w^2, its negative on that of w.  It is x^(p^6) (test_gt_cases.py)."""
    def c4(v):
        return (v[0], f2_neg(v[1]))
    return (c4(x[0]), f4_neg(c4(x[1])), c4(x[2]))


def inv(x):
    """cubic extension over Fp4: with A = a^2 - s b c, B = s c^2 - a b, C = b^2 - a c the inverse is (A + B w + C w^2) / (a A + s (c B + b C))"""
    a, b, c = x
    A = f4_sub(f4_mul(a, a), f4_mul_s(f4_mul(b, c)))
    B = f4_sub(f4_mul_s(f4_mul(c, c)), f4_mul(a, b))
    C = f4_sub(f4_mul(b, b), f4_mul(a, c))
    n = f4_inv(f4_add(f4_mul(a, A), f4_mul_s(f4_add(f4_mul(c, B), f4_mul(b, C)))))
    return (f4_mul(A, n), f4_mul(B, n), f4_mul(C, n))


def power(x, e):
    """the true power x^e, by square-and-multiply from the top bit"""
    r = ONE
    for bit in bin(e)[2:] if e else "":
        r = mul(r, r)
        if bit == "1":
            r = mul(r, x)
    return r


def coords(x):
    """the twelve Fp coordinates in byte order: c.b.b, c.b.a, c.a.b, c.a.a, b.b.b, ..., a.a.a"""
    return [x[j][h][l] for j in (2, 1, 0) for h in (1, 0) for l in (1, 0)]


def from_coords(v):
    v = [int(c) % P for c in v]
    f4 = [((v[4 * j + 3], v[4 * j + 2]), (v[4 * j + 1], v[4 * j])) for j in range(3)]
    return (f4[2], f4[1], f4[0])


def enc(x):
    return b"".join(c.to_bytes(48, "big") for c in coords(x))


def enc_raw(v):
    """twelve integers below 2^384 in byte order, written as they are (non-canonical encodings)"""
    assert len(v) == 12 and all(0 <= c < 1 << 384 for c in v)
    return b"".join(c.to_bytes(48, "big") for c in v)


def dec(b):
    """FP12_fromOctet: every coordinate counts mod p"""
    assert len(b) == 576
    return from_coords([int.from_bytes(b[48 * k:48 * k + 48], "big") for k in range(12)])


def split(b):
    return [b[576 * i:576 * i + 576] for i in range(len(b) // 576)]


# ------------------------------------------------------------------ group-theoretic facts
HARD = (P ** 4 - P ** 2 + 1) // R
assert HARD * R == P ** 4 - P ** 2 + 1 and (P ** 12 - 1) % R == 0


def frob2(x):
    return power(x, P * P)


def is_unitary(x):
    return mul(x, conj(x)) == ONE


def is_cyclotomic(x):
    """x^(p^4 - p^2 + 1) = 1, as f12t_is_cyclotomic asks it: x^(p^4) x = x^(p^2)"""
    f2 = frob2(x)
    return mul(frob2(f2), x) == f2


def fexp_true(x):
    """x^(3 (p^12 - 1) / r), which is what PAIR_fexp returns (not the first power: its hard part carries a factor 3), as
    ((conj(x) / x)^(p^2 + 1))^(3 (p^4 - p^2 + 1) / r) with conj(x) = x^(p^6); zero has no such value (see fexp_expected)"""
    return power(power(mul(conj(x), inv(x)), P * P + 1), 3 * HARD)


# ------------------------------------------------------------------ elements
def _rand(seed, i):
    v = prng(seed, i, 64) % P
    return v if v else 1


def _dense(seed):
    return from_coords([_rand(seed, k) for k in range(12)])


def _sparse(seed, keep):
    """random nonzero coordinates at the byte-order positions in keep, zero elsewhere"""
    return from_coords([_rand(seed, k) if k in keep else 0 for k in range(12)])


A_POS, B_POS, C_POS = range(8, 12), range(4, 8), range(0, 4)      # the coordinates of the coefficients a, b, c


@functools.lru_cache(maxsize=None)
def elements():
    """label -> 576 bytes, in classes (see classes()).  The builders assert the membership facts the tests rest on."""
    e = {}
    # trivial
    e["zero"] = enc(ZERO)
    e["one"] = enc(ONE)
    e["minus_one"] = enc(from_coords([0] * 11 + [P - 1]))
    # basis: 1 in one Fp coordinate
    for k in range(12):
        e["e%d" % k] = enc(from_coords([1 if j == k else 0 for j in range(12)]))
    # sparse and subfield
    e["a_only"] = enc(_sparse(7101, set(A_POS)))
    e["a_fp2"] = enc(_sparse(7102, {10, 11}))
    e["a_fp"] = enc(_sparse(7103, {11}))
    e["b_only"] = enc(_sparse(7104, set(B_POS)))
    e["c_only"] = enc(_sparse(7105, set(C_POS)))
    e["a_zero"] = enc(_sparse(7106, set(B_POS) | set(C_POS)))
    e["c_zero"] = enc(_sparse(7107, set(A_POS) | set(B_POS)))
    # group-theoretic classes
    y = _dense(7110)
    u = mul(conj(y), inv(y))                         # y^(p^6 - 1): norm 1 over Fp6, almost never in the cyclotomic subgroup
    assert is_unitary(u) and not is_cyclotomic(u) and not is_unitary(y)
    v = mul(frob2(u), u)                             # u^(p^2 + 1): the easy part of the final exponentiation, of order not dividing r
    assert is_unitary(v) and is_cyclotomic(v) and power(v, R) != ONE
    gt = split(cat(golden("pairing")["gt"]))
    assert is_cyclotomic(dec(gt[0])) and power(dec(gt[0]), R) == ONE
    assert is_unitary(dec(e["minus_one"])) and not is_cyclotomic(dec(e["minus_one"]))
    e["dense"] = enc(y)
    e["unitary"] = enc(u)
    e["cyclotomic"] = enc(v)
    e["gt"] = gt[0]
    e["gt2"] = gt[1]
    e["miller"] = _miller()
    assert not is_unitary(dec(e["miller"]))
    # non-canonical encodings
    yc = coords(_dense(7120))
    top = (1 << 384) - 1
    e["nc_plus_p"] = enc_raw([c + P for c in yc])
    e["nc_max_k"] = enc_raw([c + (top - c) // P * P for c in yc])
    e["nc_coord_p"] = enc_raw([P if k in (2, 11) else c for k, c in enumerate(yc)])              # exactly p: zero
    e["nc_coord_top"] = enc_raw([top if k in (0, 5, 10) else c for k, c in enumerate(yc)])       # exactly 2^384 - 1
    e["one_p"] = enc_raw([P] * 11 + [P + 1])                                                     # one as (p + 1, p, p, ...)
    for name in ("gt", "cyclotomic"):                # + p on a few coordinates: the same element, so still the windowed route
        c = [int.from_bytes(e[name][48 * k:48 * k + 48], "big") for k in range(12)]
        e[name + "_p"] = enc_raw([v + P if k in (0, 6, 11) else v for k, v in enumerate(c)])
        assert dec(e[name + "_p"]) == dec(e[name]) and e[name + "_p"] != e[name]
    e["zero_p"] = enc_raw([P if k in (1, 7, 11) else 0 for k in range(12)])
    assert all(len(b) == 576 for b in e.values())
    return e


def _miller():
    """the Miller value of the first golden pairing, from the plain-C oracle (the host simulation and the GPU are compared with it on the same
    inputs by test_host_sim.py / test_gpu_pairing.py): dense, not unitary"""
    from oracle.bindings import Oracle
    g = golden("pairing")
    return Oracle("port").miller(bytes.fromhex(g["g1"][0]), bytes.fromhex(g["g2"][0]))


def classes():
    return {
        "trivial": ["zero", "one", "minus_one"],
        "basis": ["e%d" % k for k in range(12)],
        "sparse": ["a_only", "a_fp2", "a_fp", "b_only", "c_only", "a_zero", "c_zero"],
        "group": ["dense", "unitary", "cyclotomic", "gt", "miller"],
        "noncanonical": ["nc_plus_p", "nc_max_k", "nc_coord_p", "nc_coord_top", "one_p", "gt_p", "cyclotomic_p", "zero_p"],
    }


def all_labels():
    return [l for ls in classes().values() for l in ls]


WINDOWED = ("cyclotomic", "gt", "one", "zero", "cyclotomic_p", "gt_p", "one_p", "zero_p")      # members as f12t_is_cyclotomic sees them (zero passes)
GENERIC = ("unitary", "minus_one", "miller", "dense")


def near_one():
    """(label, bytes) for gt_is_unity: the expected verdict is dec(bytes) == ONE"""
    one = [0] * 11 + [1]
    out = [("one", enc_raw(one))]
    for k in range(12):
        out.append(("one+e%d" % k, enc_raw([c + (1 if j == k else 0) for j, c in enumerate(one)])))       # k = 11: two
    out.append(("one, first coordinate 0", enc_raw([0] * 12)))
    out.append(("one as (p + 1, p, ...)", enc_raw([P] * 11 + [P + 1])))
    out.append(("one as p + 1", enc_raw([0] * 11 + [P + 1])))
    out.append(("one as 2p + 1, p in c", enc_raw([P, 0, 0, 2 * P] + [0] * 7 + [2 * P + 1])))
    for k in range(11):                              # p + 1 forms that are NOT one: a 1 hidden under + p in one other coordinate
        out.append(("one_p+e%d" % k, enc_raw([P + (1 if j == k else 0) for j in range(11)] + [P + 1])))
    out.append(("p + 2", enc_raw([P] * 11 + [P + 2])))
    out.append(("minus_one", elements()["minus_one"]))
    out.append(("gt", elements()["gt"]))
    return out


def unity_expected(items):
    return bytes(1 if dec(b) == ONE else 0 for _, b in items)


# ------------------------------------------------------------------ case lists shared by the host simulation and the GPU tests
def mul_pairs():
    """(label, x bytes, y bytes): all 144 basis products, sparse x sparse (+ dense), x . 0 / 1 / -1, non-canonical operands on either side and on both"""
    e = elements()
    out = [("e%d*e%d" % (i, j), e["e%d" % i], e["e%d" % j]) for i in range(12) for j in range(12)]
    sp = classes()["sparse"] + ["dense"]
    out += [("%s*%s" % (a, b), e[a], e[b]) for a in sp for b in sp]
    for a in sp + ["unitary", "gt", "miller", "minus_one", "zero", "one"]:
        for b in ("zero", "one", "minus_one"):
            out.append(("%s*%s" % (a, b), e[a], e[b]))
            out.append(("%s*%s" % (b, a), e[b], e[a]))
    nc = classes()["noncanonical"]
    for a in nc:
        out.append(("%s*dense" % a, e[a], e["dense"]))
        out.append(("b_only*%s" % a, e["b_only"], e[a]))
        out += [("%s*%s" % (a, b), e[a], e[b]) for b in nc]
    return out


def mul_expected(pairs):
    return b"".join(enc(mul(dec(x), dec(y))) for _, x, y in pairs)


def conj_expected(labels):
    e = elements()
    return b"".join(enc(conj(dec(e[l]))) for l in labels)


@functools.lru_cache(maxsize=None)
def fexp_tower():
    """label -> bytes of x^(3 (p^12 - 1) / r) for every label of all_labels() but the encodings of zero (every class whole: the inverses
    and Frobenius images of the basis and sparse elements are sparse or zero in f0, f1, f2)"""
    e = elements()
    return {l: enc(fexp_true(dec(e[l]))) for l in all_labels() if dec(e[l]) != ZERO}


POW_EXPS = (0, 1, 2, 15, 16, R - 1, R, (1 << 256) - 1, prng(7130, 1, 32), prng(7130, 2, 32))
POW_LABELS = ("dense", "unitary", "cyclotomic", "gt", "miller", "minus_one", "zero", "one", "gt_p", "cyclotomic_p", "one_p", "zero_p")


# sparse and subfield bases: f12t_frob is reached from the entries only through the membership test, and only here on such inputs
POW_SPARSE_LABELS = ("a_only", "a_fp2", "a_fp", "b_only", "c_only", "a_zero", "c_zero", "e0", "e7", "e10", "nc_coord_p")
POW_SPARSE_EXPS = (15, POW_EXPS[-2])


def pow_cases(exps=POW_EXPS, which=POW_LABELS):
    """(labels, bases, exponents): every label of `which` with every exponent of exps, label-major"""
    e = elements()
    labels = [(l, x) for l in which for x in exps]
    return labels, b"".join(e[l] for l, _ in labels), b"".join(x.to_bytes(32, "big") for _, x in labels)


def entry_lists(oracle):
    """the mul, is_unity, fexp and pow lists as the entries take them, with their expected bytes: name -> (op, a, b, expected, labels).
    `oracle` is the plain-C oracle: FP12_pow, and the final exponentiation of zero."""
    e = elements()
    pairs = mul_pairs()
    items = near_one()
    fl = all_labels()
    tower = fexp_tower()
    pl, pa, pe = pow_cases()
    sl, sa, se = pow_cases(POW_SPARSE_EXPS, POW_SPARSE_LABELS)       # the membership test's Frobenius maps on sparse and subfield elements
    pl, pa, pe = pl + sl, pa + sa, pe + se
    return {
        "mul": ("mul", b"".join(p[1] for p in pairs), b"".join(p[2] for p in pairs), mul_expected(pairs), [p[0] for p in pairs]),
        "is_unity": ("is_unity", b"".join(b for _, b in items), None, unity_expected(items), [l for l, _ in items]),
        "fexp": ("fexp", b"".join(e[l] for l in fl), None, b"".join(tower[l] if l in tower else oracle.fexp(e[l]) for l in fl), fl),
        "pow": ("pow", pa, pe, oracle.gt_op("pow", pa, pe), pl),
    }


def run_entry_lists(c, lists):
    """every list through a Context's GT entries: [(name, labels that differ)] of the lists with a mismatch"""
    bad = []
    for name, (op, a, b, want, labels) in lists.items():
        got = c.gt_is_unity(a) if op == "is_unity" else (c.fexp(a) if op == "fexp" else c.gt_op(op, a, b))
        d = differs(got, want, len(want) // len(labels), labels)
        if d:
            bad.append((name, d))
    return bad


@functools.lru_cache(maxsize=None)
def true_power(label, exponent):
    return enc(power(dec(elements()[label]), exponent))


# ------------------------------------------------------------------ lane patterns over wavefronts of 21 triples
SPECIAL_AT = (0, 20, 21 + 9, 62)
RAGGED = (1, 20, 21, 22, 43, 64)


def pattern(fillers, special, index, n=63):
    """n labels: the fillers in turn with `special` at `index`"""
    assert 0 <= index < n
    return [special if i == index else fillers[i % len(fillers)] for i in range(n)]


def ragged(fillers, special, n):
    """n labels with the special element last: alone in the last group when n = 1, 22, 43 or 64"""
    return pattern(fillers, special, n - 1, n)


def pattern_exps(seed, n):
    """n exponents: random 256-bit ones, the edge ones in lanes 1 .. 8 (never at an index of SPECIAL_AT: the special element's exponent
    must be one on which the two ladders differ)"""
    edge = [0, 1, 2, 15, 16, R - 1, R, (1 << 256) - 1]
    return [edge[i - 1] if 1 <= i <= len(edge) else prng(seed, i, 32) for i in range(n)]


def differs(got, want, w, labels):
    """the labels of the records that differ, as one string ("" when none does)"""
    assert len(got) == len(want) == w * len(labels), (len(got), len(want), w, len(labels))
    return "; ".join(str(labels[i]) for i in range(len(labels)) if got[w * i:w * i + w] != want[w * i:w * i + w])
