"""Structured inputs on the twist E': y^2 = x^3 + 4(1 + i) over Fp2 = Fp[i]/(i^2 + 1): points of small order, the multiples of Q that the
Miller loop passes through, and x coordinates whose right-hand side is real or purely imaginary (where the choice of sqrt(a^2 + b^2) inside
the complex square-root method shows in the decoded bytes).  Plain affine arithmetic on Python integers, shared by the oracle, host-sim and
GPU tests; every input these tests build comes from here, never from a kernel's output.

#E'(Fp2) = H2 * R with H2 = 13^2 23^2 2713 11953 262069 (a 135-digit prime).  E'(Fp2)[13] is Z_13 x Z_13, so there are independent points
of order 13.  |x| = 0xd201000000010000 begins with the bits 1101 = 13: the loop T = Q; for i = 64..1: T = 2T; T += (bit_i(3|x|) - bit_i(|x|)) Q
reaches T = 12 Q at i = 61 and adds Q there, so a Q of order 13 sends it through infinity (degenerate_steps)."""
from util import P, R, golden

X = 0xd201000000010000                      # |x|, the curve parameter is -|x|
H2 = 0x5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5
H2_SMALL_FACTORS = (13, 13, 23, 23, 2713, 11953, 262069)
B2 = (4, 4)                                 # the twist's constant 4 (1 + i)


# ---------------------------------------------------------------- Fp2: (a, b) = a + b i
def f2_add(x, y):
    return (x[0] + y[0]) % P, (x[1] + y[1]) % P


def f2_sub(x, y):
    return (x[0] - y[0]) % P, (x[1] - y[1]) % P


def f2_neg(x):
    return (-x[0]) % P, (-x[1]) % P


def f2_mul(x, y):
    return (x[0] * y[0] - x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P


def f2_sqr(x):
    return f2_mul(x, x)


def f2_inv(x):
    n = pow(x[0] * x[0] + x[1] * x[1], -1, P)
    return x[0] * n % P, (-x[1]) * n % P


def fp_sqrt(a):
    """a square root of a in Fp (p = 3 mod 4), or None"""
    s = pow(a, (P + 1) // 4, P)
    return s if s * s % P == a % P else None


def f2_sqrt(u):
    """a square root of u in Fp2 (either one), or None: the complex method with both roots of the norm tried"""
    a, b = u
    if b == 0:
        s = fp_sqrt(a)
        if s is not None:
            return s, 0
        return 0, fp_sqrt(-a % P)
    n = fp_sqrt((a * a + b * b) % P)
    if n is None:
        return None
    for w1 in (n, P - n):
        ra = fp_sqrt((a + w1) * pow(2, -1, P) % P)
        if ra:
            r = (ra, b * pow(2 * ra, -1, P) % P)
            assert f2_sqr(r) == (a % P, b % P)
            return r
    raise AssertionError("norm is a square but neither (a +- n) / 2 is")


def rhs(x):
    return f2_add(f2_mul(f2_sqr(x), x), B2)


def on_curve(pt):
    return pt is None or f2_sqr(pt[1]) == rhs(pt[0])


# ---------------------------------------------------------------- affine arithmetic on E' (None = infinity)
def ec_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if f2_add(a[1], b[1]) == (0, 0):
            return None
        x2 = f2_sqr(a[0])
        lam = f2_mul(f2_add(f2_add(x2, x2), x2), f2_inv(f2_add(a[1], a[1])))
    else:
        lam = f2_mul(f2_sub(b[1], a[1]), f2_inv(f2_sub(b[0], a[0])))
    x = f2_sub(f2_sub(f2_sqr(lam), a[0]), b[0])
    return x, f2_sub(f2_mul(lam, f2_sub(a[0], x)), a[1])


def ec_neg(a):
    return None if a is None else (a[0], f2_neg(a[1]))


def ec_mul(k, a):
    if k < 0:
        k, a = -k, ec_neg(a)
    r = None
    while k:
        if k & 1:
            r = ec_add(r, a)
        a = ec_add(a, a)
        k >>= 1
    return r


def _f2_bytes(x):
    return x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big")       # imaginary half first (FP2_toBytes)


def enc192(a):
    """192-byte affine encoding x.b | x.a | y.b | y.a, all-zero = infinity"""
    return bytes(192) if a is None else _f2_bytes(a[0]) + _f2_bytes(a[1])


def enc97(x, tag):
    """97-byte compressed encoding of the x coordinate (a, b) under sign tag 0x02 / 0x03"""
    return bytes([tag]) + _f2_bytes(x)


def _f2_from(b):
    return int.from_bytes(b[48:96], "big"), int.from_bytes(b[:48], "big")


def dec192(b):
    return None if b == bytes(192) else (_f2_from(b[:96]), _f2_from(b[96:192]))


def f2_sign(y):
    """FP2_sign: parity of a, or of b when a == 0"""
    return (y[1] if y[0] == 0 else y[0]) & 1


def compress(a):
    return bytes(97) if a is None else enc97(a[0], 0x02 | f2_sign(a[1]))


def generator():
    return dec192(bytes.fromhex(golden("g2")["generator"]))


def point_of_order(q, start=0):
    """a point of prime order q | H2: x = (start + 1, 1), (start + 2, 1), ... until x is on the curve and its q-part is not trivial, then
    multiplied down to order q"""
    m = H2 * R
    assert m % q == 0
    while m % q == 0:
        m //= q
    a = start
    while True:
        a += 1
        x = (a, 1)
        y = f2_sqrt(rhs(x))
        if y is None:
            continue
        t = ec_mul(m, (x, y))
        if t is None:
            continue
        for _ in range(8):
            nxt = ec_mul(q, t)
            if nxt is None:
                return t
            t = nxt
        raise AssertionError("the q-part of a curve point does not vanish: H2 * R is not the group order?")


def independent_points_of_order(q):
    """two points of order q neither of which is a multiple of the other (E'(Fp2)[q] = Z_q x Z_q)"""
    t1 = point_of_order(q)
    span = set()
    s = None
    for _ in range(q):
        s = ec_add(s, t1)
        span.add(s)
    start = 0
    for _ in range(64):
        start += 1
        t2 = point_of_order(q, start)
        if t2 not in span:
            return t1, t2
    raise AssertionError("no second independent point of order %d found" % q)


# ---------------------------------------------------------------- the Miller loop's multiples of Q
def miller_multiples():
    """The 69 steps of the loop as (i, kind, multiple, bt): kind "dbl" doubles T = [multiple]Q, kind "add" adds bt Q (bt = +-1) to
    T = [multiple]Q.  multiple is an integer (not reduced): the loop of PAIR_ate, n = |x|, n3 = 3 n, i = nbits(n3) - 2 .. 1."""
    n, n3 = X, 3 * X
    steps, m = [], 1
    for i in range(n3.bit_length() - 2, 0, -1):
        steps.append((i, "dbl", m, 0))
        m *= 2
        bt = ((n3 >> i) & 1) - ((n >> i) & 1)
        if bt:
            steps.append((i, "add", m, bt))
            m += bt
    return steps


ADD_NEG, ADD_SAME, DBL_INF, ADD_INF = "add T=-Q", "add T=Q", "dbl inf", "add inf"


def degenerate_steps(q):
    """the steps of miller_multiples() that the generic line formulas do not cover when Q has order q, as (i, what): an addition with
    T = -bt Q (the sum is infinity), with T = bt Q (the addition is a doubling), a doubling of infinity, an addition to infinity"""
    out = []
    for i, kind, m, bt in miller_multiples():
        if kind == "dbl":
            if m % q == 0:
                out.append((i, DBL_INF))
        elif m % q == 0:
            out.append((i, ADD_INF))
        elif (m + bt) % q == 0:
            out.append((i, ADD_NEG))
        elif (m - bt) % q == 0:
            out.append((i, ADD_SAME))
    return out


# ---------------------------------------------------------------- x with a real / purely imaginary right-hand side
def _is_qr(a):
    return pow(a, (P - 1) // 2, P) == 1


def real_rhs_x(qr, odd):
    """(x, v): the first x = (a, b), counting b = 2, 3, ... and a = +sqrt, -sqrt of (b^3 - 4) / (3 b), whose right-hand side
    x^3 + 4(1 + i) = (a^3 - 3 a b^2 + 4) + (3 a^2 b - b^3 + 4) i is the real v != 0 with the asked residuosity and parity"""
    b = 1
    while True:
        b += 1
        s = fp_sqrt((b ** 3 - 4) * pow(3 * b, -1, P) % P)
        if not s:
            continue
        for a in (s, P - s):
            v, im = rhs((a, b))
            assert im == 0
            if v != 0 and _is_qr(v) == qr and (v & 1) == int(odd):
                return (a, b), v


def imaginary_rhs_xs():
    """the two x = (a, +-b) with the smallest a >= 1 whose right-hand side is purely imaginary (and not 0): controls, where both roots of
    the norm lead to the same bytes"""
    a = 0
    while True:
        a += 1
        s = fp_sqrt((a ** 3 + 4) * pow(3 * a, -1, P) % P)
        if not s:
            continue
        xs = [(a, s), (a, P - s)]
        if all(rhs(x)[0] == 0 and rhs(x)[1] != 0 for x in xs):
            return xs


REAL_CLASSES = ((False, False), (True, True), (True, False), (False, True))     # (qr, odd); the first two differed before the fix


def reference_root_of_real(v):
    """what FP2_sqrt returns for the real v: w1 is the even one of +-v, so an odd v gives w2 = 0 and the root (0, 0)"""
    if v & 1:
        return 0, 0
    y = f2_sqrt((v, 0))
    return f2_neg(y) if f2_sign(y) else y


# ---------------------------------------------------------------- the inputs of the twist tests
def g2_edge_scalars():
    """0..16 (every window entry), 26 = 2 * 13, |x|^j, the ends of the range, and values whose 4-bit digits in some |x|-adic component are
    all even or all zero"""
    ks = list(range(17)) + [26, X, X * X, X ** 3, R - 1, R, R + 1, (1 << 256) - 1]
    ks += [X + 1, X * X + X, 2 * X ** 3 + 2, 0x2222222222222222, 0x2020202020202020 * X + 0x10, (X ** 3) * 4 + 4 * X]
    return ks


def twist_points():
    """name -> point: the input set of the twist tests (at most about 40 values with the multiples)"""
    t13a, t13b = independent_points_of_order(13)
    g = generator()
    pts = {"inf": None, "t13a": t13a, "t13b": t13b, "t23": point_of_order(23), "t2713": point_of_order(2713), "g+t13": ec_add(g, t13a),
           "g": g, "5g": ec_mul(5, g)}
    m = t13a
    for j in range(2, 13):
        m = ec_add(m, t13a)
        pts["%d*t13a" % j] = m
    return pts


def g1_ordinary(n, seed):
    """n points of G1 as 96-byte encodings: seeded multiples of the generator, computed with g1_torsion's affine arithmetic"""
    import g1_torsion
    from util import prng
    g = g1_torsion.generator()
    return [g1_torsion.enc(g1_torsion.ec_mul(prng(seed, i) % R, g)) for i in range(n)]


def real_rhs_cases():
    """[(label, 97-byte encoding, expected 192-byte decoding)] for the four real classes under both sign tags and the two imaginary
    controls: the expectation is the reference's rule (reference_root_of_real), worked out on Python integers"""
    out = []
    for qr, odd in REAL_CLASSES:
        x, v = real_rhs_x(qr, odd)
        y = reference_root_of_real(v)
        for tag in (2, 3):
            yy = y if f2_sign(y) == (tag & 1) else f2_neg(y)
            out.append(("real rhs %s %s tag %d" % ("residue" if qr else "non-residue", "odd" if odd else "even", tag), enc97(x, tag), enc192((x, yy))))
    for x in imaginary_rhs_xs():
        y = f2_sqrt(rhs(x))
        for tag in (2, 3):
            yy = y if f2_sign(y) == (tag & 1) else f2_neg(y)
            out.append(("imaginary rhs b %s tag %d" % ("odd" if x[1] & 1 else "even", tag), enc97(x, tag), enc192((x, yy))))
    return out
