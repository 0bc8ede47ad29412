"""Inputs that send hash-to-G1 (h2c.hpp) and the Zp / Fp helper entries (k_hash_zp.hip, fr.hpp, fp_op_kernel) through their degenerate
branches, worked out on Python integers and shared by the host-sim and GPU tests; every input these tests build comes from here, never
from a kernel's output.  The only constants are the public ones at the top of tools/gen_consts.py (A', B', Z and the 11-isogeny).

The map (ECP_map2point): t = Z u^2, w = t^2 + t, x1 = -B'/A' (1 + 1/w), x2 = t x1; x = x1 if g(x1) = x1^3 + A' x1 + B' is a square, else
x2; y = the square root of g(x) whose parity is u's; then the 11-isogeny E' -> E.  Its branches, as `branch(u)` tags them:
  zero-den   w = 0 (u = 0, or t = -1: u = +-sqrt(-1/11), which exist because 11 and -1 are both non-residues).  The reference divides by
             inverse(0) = 0 and counts 0 as a non-residue: x = x2 = 0, y = 0, a pair that is not on E', and its image (ZERO_DEN_PAIR) is
             not on E
  kernel     x is the x-coordinate of a point of the isogeny's kernel, a common root of ISO11_XDEN and ISO11_YDEN: the image is infinity
  qr / nqr   x1 or x2 is taken; /keep or /neg: whether the root that the one exponentiation delivers — g^((p+1)/4) on the qr branch,
             (Z g)^((p+1)/4) Z u^3 on the other — already has u's parity or is negated
The module asserts that its lists hold every branch (at the bottom): a list that lost one fails on import, on the CPU."""
import functools
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.gen_consts import ISO11_XDEN, ISO11_XNUM, ISO11_YDEN, ISO11_YNUM, SSWU_A, SSWU_B, SSWU_Z    # noqa: E402

from g1_torsion import ec_add, ec_mul, enc, generator, point_of_order                                  # noqa: E402
from util import P, R, prng                                                                            # noqa: E402

COFACTOR = 0xd201000000010001                    # 1 - x: ECP_cfp multiplies by it


# ---------------------------------------------------------------- Fp helpers
def is_square(a):
    """a non-zero square mod p (0 counts as a non-residue, as FP_qr has it)"""
    return pow(a, (P - 1) // 2, P) == 1


def sqrt(a):
    """the root a^((p+1)/4) of a square a (p = 3 mod 4)"""
    return pow(a, (P + 1) // 4, P)


def ev(cs, x, monic):
    acc = 1 if monic else 0
    for c in reversed(cs):
        acc = (acc * x + c) % P
    return acc


def g_prime(x):
    return (x * x * x + SSWU_A * x + SSWU_B) % P


# ---------------------------------------------------------------- the map on integers
def sswu(u):
    """u (any integer, taken mod p) -> (branch, x, y) on E'"""
    u %= P
    t = SSWU_Z * u * u % P
    w = (t * t + t) % P
    if w == 0:
        return "zero-den", 0, 0
    x1 = -SSWU_B * (w + 1) * pow(SSWU_A * w, -1, P) % P
    g1 = g_prime(x1)
    if is_square(g1):
        x, cand, tag = x1, sqrt(g1), "qr"
    else:
        x, cand, tag = t * x1 % P, sqrt(SSWU_Z * g1 % P) * SSWU_Z * u * u * u % P, "nqr"
    assert cand * cand % P == g_prime(x)
    neg = (cand & 1) != (u & 1)
    y = (P - cand) if neg else cand
    if ev(ISO11_XDEN, x, True) == 0:
        assert ev(ISO11_YDEN, x, True) == 0
        return "kernel", x, y
    return tag + ("/neg" if neg else "/keep"), x, y


def branch(u):
    return sswu(u)[0]


def iso11(x, y):
    """the isogeny in affine form (None = infinity: a kernel point)"""
    xd, yd = ev(ISO11_XDEN, x, True), ev(ISO11_YDEN, x, True)
    if xd == 0 or yd == 0:
        return None
    return ev(ISO11_XNUM, x, False) * pow(xd, -1, P) % P, y * ev(ISO11_YNUM, x, False) * pow(yd, -1, P) % P


ZERO_DEN_PAIR = iso11(0, 0)                      # what map_to_point returns for a zero denominator: (x, 0), not on E


def map_to_point(u):
    """u -> the affine point of E (None = infinity), the reference's off-curve pair for a zero denominator"""
    _, x, y = sswu(u)
    return iso11(x, y)


def on_curve(a):
    return a is None or (a[1] * a[1] - a[0] ** 3 - 4) % P == 0


# ---------------------------------------------------------------- rational roots of the isogeny's denominator
def _trim(a):
    while a and a[-1] == 0:
        a.pop()
    return a


def _pmod(a, f):
    """a mod f, ascending coefficients, f monic"""
    a = list(a)
    d = len(f) - 1
    while len(a) > d:
        c = a.pop()
        if c:
            for i in range(d):
                a[len(a) - d + i] = (a[len(a) - d + i] - c * f[i]) % P
    return _trim(a)


def _pmulmod(a, b, f):
    if not a or not b:
        return []
    r = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            r[i + j] = (r[i + j] + x * y) % P
    return _pmod(r, f)


def _ppow(a, e, f):
    r = [1]
    while e:
        if e & 1:
            r = _pmulmod(r, a, f)
        a = _pmulmod(a, a, f)
        e >>= 1
    return r


def _pgcd(a, b):
    a, b = _trim(list(a)), _trim(list(b))
    while b:
        inv = pow(b[-1], -1, P)
        b = [c * inv % P for c in b]
        a, b = b, _pmod(a, b)
    return a


def _psub(a, b):
    n = max(len(a), len(b))
    return _trim([((a[i] if i < len(a) else 0) - (b[i] if i < len(b) else 0)) % P for i in range(n)])


def rational_roots(f):
    """the roots in Fp of a monic polynomial: gcd(f, x^p - x) is the product of its distinct linear factors, split by
    gcd(g, (x + a)^((p-1)/2) - 1) for a = 1, 2, ... (equal-degree splitting with a fixed sequence of shifts)"""
    lin = _pgcd(f, _psub(_ppow([0, 1], P, f), [0, 1]))
    todo, roots, a = [lin], [], 0
    while todo:
        a += 1
        nxt = []
        for g in todo:
            if len(g) == 2:
                roots.append(-g[0] * pow(g[1], -1, P) % P)
                continue
            if len(g) < 2:
                continue
            h = _pgcd(g, _psub(_ppow([a, 1], (P - 1) // 2, g), [1]))
            if 1 < len(h) < len(g):
                q = _pdiv(g, h)
                nxt += [h, q]
            else:
                nxt.append(g)
        todo = nxt
    return sorted(roots)


def _pdiv(a, b):
    """a / b for b | a"""
    a, q = list(a), [0] * (len(a) - len(b) + 1)
    inv = pow(b[-1], -1, P)
    for k in range(len(q) - 1, -1, -1):
        c = a[k + len(b) - 1] * inv % P
        q[k] = c
        for i, y in enumerate(b):
            a[k + i] = (a[k + i] - c * y) % P
    assert not _trim(a)
    return q


def _quadratic(a, b, c):
    """the roots of a t^2 + b t + c in Fp"""
    d = (b * b - 4 * a * c) % P
    if d and not is_square(d):
        return []
    s = sqrt(d)
    i = pow(2 * a, -1, P)
    return sorted({(-b + s) * i % P, (-b - s) * i % P})


@functools.lru_cache(maxsize=None)
def kernel_inputs():
    """[(root index, u)]: every u whose selected candidate is a rational root x0 of ISO11_XDEN.  With c = -B'/A':
    x1 = x0  <=>  w = t^2 + t = c / (x0 - c);   x2 = t x1 = c (t^2 + t + 1) / (t + 1) = x0  <=>  c t^2 + (c - x0) t + (c - x0) = 0;
    u = +-sqrt(t / Z) where that is a square.  A u is kept when the map really takes that candidate."""
    roots = rational_roots(ISO11_XDEN + [1])
    assert len(roots) == 5 and all(ev(ISO11_YDEN, x0, True) == 0 for x0 in roots)
    c = -SSWU_B * pow(SSWU_A, -1, P) % P
    zi = pow(SSWU_Z, -1, P)
    out = []
    for k, x0 in enumerate(roots):
        ts = []
        if x0 != c:
            ts += _quadratic(1, 1, -c * pow(x0 - c, -1, P) % P)
        ts += _quadratic(c, (c - x0) % P, (c - x0) % P)
        for t in ts:
            if not is_square(t * zi % P):
                continue
            u = sqrt(t * zi % P)
            for v in sorted({u, P - u}):
                tag, x, _ = sswu(v)
                if tag == "kernel" and x == x0 and (k, v) not in out:
                    out.append((k, v))
    return out


# ---------------------------------------------------------------- (a) field elements for map_to_point
def zero_den_inputs():
    s = sqrt(-pow(SSWU_Z, -1, P) % P)
    assert SSWU_Z * s * s % P == P - 1
    return [0, s, P - s]


def seeded_by_class(seed=9801, per_class=4):
    """the first per_class values of the seeded stream in each of qr/keep, qr/neg, nqr/keep, nqr/neg"""
    got = {"qr/keep": [], "qr/neg": [], "nqr/keep": [], "nqr/neg": []}
    i = 0
    while any(len(v) < per_class for v in got.values()):
        u = prng(seed, i) % P
        i += 1
        tag = branch(u)
        if tag in got and len(got[tag]) < per_class:
            got[tag].append(u)
    return [u for tag in sorted(got) for u in got[tag]]


def _top384(u):
    """the largest u + k p below 2^384"""
    return u + ((1 << 384) - 1 - u) // P * P


@functools.lru_cache(maxsize=None)
def map_cases():
    """[(name, u < 2^384, branch)]"""
    out = [("zero-den %d" % i, u) for i, u in enumerate(zero_den_inputs())]
    out += [("kernel root %d #%d" % (k, i), u) for i, (k, u) in enumerate(kernel_inputs())]
    out += [("1", 1), ("p-1", P - 1), ("(p-1)/2", (P - 1) // 2), ("(p+1)/2", (P + 1) // 2), ("5", 5)]
    seeded = seeded_by_class()
    out += [("seeded %d" % i, u) for i, u in enumerate(seeded)]
    # unreduced: u + p and the largest u + k p below 2^384, for a u of every kind; 2^384 - 1 itself
    kinds, picked = {}, []
    for name, u in out:
        kinds.setdefault(branch(u), []).append((name, u))
    for tag in sorted(kinds):
        picked += kinds[tag][:2] if tag == "zero-den" else kinds[tag][-1:]
    for name, u in picked:
        out += [(name + " + p", u + P), (name + " + kp", _top384(u))]
    out += [("p", P), ("2^384 - 1", (1 << 384) - 1)]
    return [(name, u, branch(u)) for name, u in out]


def map_bytes():
    return b"".join(u.to_bytes(48, "big") for _, u, _ in map_cases())


# ---------------------------------------------------------------- (b) digests for from_hash
@functools.lru_cache(maxsize=None)
def hash_cases():
    """[(name, 512-bit integer, branch)]: degenerate and seeded digests interleaved, so that every degenerate lane has ordinary
    neighbours"""
    special, seen = [], set()
    for name, u, _ in map_cases():
        if u % P in seen:
            continue
        seen.add(u % P)
        u %= P
        kmax = ((1 << 512) - 1 - u) // P
        special += [(name, u), (name + " + p", u + P), (name + " + %d p" % kmax, u + kmax * P)]
    special += [("2^512 - 1", (1 << 512) - 1), ("2^384", 1 << 384), ("2^384 - 1", (1 << 384) - 1), ("top 128 bits", ((1 << 128) - 1) << 384)]
    seeded = [("seeded digest %d" % i, prng(9802, i)) for i in range(64)]
    out = []
    for i, s in enumerate(special):
        out.append(s)
        if i < len(seeded):
            out.append(seeded[i])
    out += seeded[len(special):]
    return [(name, d, branch(d)) for name, d in out]


def hash_bytes():
    return b"".join(d.to_bytes(64, "big") for _, d, _ in hash_cases())


# ---------------------------------------------------------------- (c) points for cofactor clearing
OFF_CURVE = "off-curve"


@functools.lru_cache(maxsize=None)
def cofactor_cases():
    """[(name, 96 bytes, expected 96 bytes or OFF_CURVE)]: expected = the plain multiple [1 - x]P on Python integers.  E(Fp)[11] is
    Z_11 x Z_11 (no point has order 11^2): `o11 + o11'` is the sum of two independent points of order 11, so the three of them span the
    whole 11^2-element part of the cofactor."""
    g = generator()
    t3 = (0, 2)
    o11 = point_of_order(11)
    start, o11b = 2, o11
    while any(ec_mul(j, o11) == o11b for j in range(11)):          # the next curve point whose 11-part is no multiple of o11
        o11b = point_of_order(11, start)
        start += 1
    pts = [("infinity", None), ("(0, 2)", t3), ("(0, -2)", (0, P - 2)), ("order 11", o11), ("order 11'", o11b), ("o11 + o11'", ec_add(o11, o11b)),
           ("order 10177", point_of_order(10177)), ("G + T3", ec_add(g, t3)), ("G + o11", ec_add(g, o11)), ("G", g)]
    pts += [("subgroup %d" % i, ec_mul(prng(9803, i) % R, g)) for i in range(4)]
    pts += [("image of " + name, map_to_point(u)) for name, u, tag in map_cases() if name.startswith("seeded") and "+" not in name]
    assert all(on_curve(a) for _, a in pts) and not on_curve(ZERO_DEN_PAIR)
    out = [(name, enc(a), enc(ec_mul(COFACTOR, a))) for name, a in pts]
    out.insert(len(out) // 2, ("map_to_point(0)", enc(ZERO_DEN_PAIR), OFF_CURVE))
    return out


# ---------------------------------------------------------------- (d) Zp
_QR = ((1 << 256) // R) * R
ZP_EDGE = [0, 1, 2, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, (1 << 256) - 1, (1 << 256) - 2, _QR, _QR - 1, 1 << 255, (1 << 255) - 1,
           (R - 1) // 2, (R + 1) // 2, 1 << 128, (1 << 128) - 1, (1 << 32) - 1, 1 << 32]
ZP_OPS = ("mul", "add", "sub", "neg", "inv")


def zp_grid():
    """(a bytes, b bytes, [(a, b)]) over ZP_EDGE x ZP_EDGE"""
    pairs = [(a, b) for a in ZP_EDGE for b in ZP_EDGE]
    return b"".join(a.to_bytes(32, "big") for a, _ in pairs), b"".join(b.to_bytes(32, "big") for _, b in pairs), pairs


def zp_expected(op, pairs):
    f = {"mul": lambda a, b: a * b, "add": lambda a, b: a + b, "sub": lambda a, b: a - b, "neg": lambda a, b: -a,
         "inv": lambda a, b: pow(a % R, R - 2, R)}[op]
    return b"".join((f(a, b) % R).to_bytes(32, "big") for a, b in pairs)


_Q512 = ((1 << 512) - 1) // R * R
ZP_DIGESTS = [0, R, R + 1, R - 1, (1 << 512) - 1, _Q512, _Q512 - 1, 1 << 256, (1 << 256) - 1, 1 << 511] + [prng(9804, i) for i in range(32)]


def zp_digest_bytes():
    return b"".join(d.to_bytes(64, "big") for d in ZP_DIGESTS)


def zp_digest_expected():
    return b"".join((d % R).to_bytes(32, "big") for d in ZP_DIGESTS)


# ---------------------------------------------------------------- (e) Fp
_QP = ((1 << 384) // P) * P
FP_EDGE = [0, 1, 2, P - 1, P, P + 1, 2 * P - 1, 2 * P, 9 * P, 9 * P + 1, (1 << 384) - 1, _QP, _QP - 1, (P - 1) // 2, (P + 1) // 2, 1 << 381,
           (1 << 381) - 1, 1 << 383, (1 << 28) - 1, 1 << 28, 1 << 364]
FP_OPS = ("mul", "add", "sub", "sqr", "neg", "inv")


def fp_grid():
    pairs = [(a, b) for a in FP_EDGE for b in FP_EDGE]
    return b"".join(a.to_bytes(48, "big") for a, _ in pairs), b"".join(b.to_bytes(48, "big") for _, b in pairs), pairs


def fp_expected(op, pairs):
    f = {"mul": lambda a, b: a * b, "add": lambda a, b: a + b, "sub": lambda a, b: a - b, "sqr": lambda a, b: a * a, "neg": lambda a, b: -a,
         "inv": lambda a, b: pow(a % P, P - 2, P)}[op]
    return b"".join((f(a, b) % P).to_bytes(48, "big") for a, b in pairs)


# ---------------------------------------------------------------- (f) inner products
# the fold takes 64 terms per lane and stage: one stage up to 64 terms, two up to 4096, three up to 262144, four beyond
FOLD_SIZES = (1, 2, 63, 64, 65, 4095, 4096, 4097, 262144, 262145)


def fold_stages(n):
    s = 1
    while n > 64:
        n, s = (n + 63) // 64, s + 1
    return s


@functools.lru_cache(maxsize=None)
def fold_case(n):
    """(a bytes, b bytes, sum of a[i] b[i] mod r, sum of a[i] mod r): seeded unreduced 256-bit operands with the edge values of ZP_EDGE at
    the ends and on either side of the stage boundaries"""
    a = bytearray(hashlib.shake_256(b"c12381 fold a|%d" % n).digest(32 * n))
    b = bytearray(hashlib.shake_256(b"c12381 fold b|%d" % n).digest(32 * n))
    for j, i in enumerate(sorted({0, n - 1, 63, 64, 4095, 4096})):
        if i < n:
            a[32 * i:32 * i + 32] = ZP_EDGE[(3 + 2 * j + n) % len(ZP_EDGE)].to_bytes(32, "big")
            b[32 * i:32 * i + 32] = ZP_EDGE[(9 + 5 * j + n) % len(ZP_EDGE)].to_bytes(32, "big")
    av = [int.from_bytes(a[32 * i:32 * i + 32], "big") for i in range(n)]
    bv = [int.from_bytes(b[32 * i:32 * i + 32], "big") for i in range(n)]
    return bytes(a), bytes(b), (sum(x * y for x, y in zip(av, bv)) % R).to_bytes(32, "big"), (sum(av) % R).to_bytes(32, "big")


# ---------------------------------------------------------------- the lists hold every branch
def _coverage():
    tags = [tag for _, _, tag in map_cases()]
    count = {t: tags.count(t) for t in set(tags)}
    assert count.get("zero-den", 0) >= 3, count
    assert count.get("kernel", 0) >= 8 and len({k for k, _ in kernel_inputs()}) >= 2, count
    seeded = [tag for name, u, tag in map_cases() if name.startswith("seeded") and u < P]
    for t in ("qr/keep", "qr/neg", "nqr/keep", "nqr/neg"):
        assert seeded.count(t) >= 4, (t, seeded)
    assert sum(t.startswith("qr") for t in seeded) >= 8 and sum(t.startswith("nqr") for t in seeded) >= 8, seeded
    assert any(u >= P for _, u, _ in map_cases()) and any(u == (1 << 384) - 1 for _, u, _ in map_cases())
    htags = [tag for _, _, tag in hash_cases()]
    assert htags.count("zero-den") >= 9 and htags.count("kernel") >= 24
    assert [fold_stages(n) for n in FOLD_SIZES] == [1, 1, 1, 1, 2, 2, 2, 3, 3, 4]
    assert len(ZP_EDGE) == 21 and len(FP_EDGE) == 21          # the largest multiples below 2^256 and 2^384 are 2r and 9p: listed twice
    assert max(ZP_EDGE) < 1 << 256 and max(FP_EDGE) < 1 << 384
    return count


COVERAGE = _coverage()
