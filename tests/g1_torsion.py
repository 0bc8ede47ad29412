"""Points of small order on E: y^2 = x^3 + 4 over Fp and a predictor of the lanes that the incomplete formulas of g1_scalar_mul
(g1.hpp: co-Z affine table, Jacobian loop) cannot serve.  Plain affine arithmetic on Python integers, shared by the host-sim, oracle and
GPU tests; every input these tests build comes from here, never from a kernel's output.

The loop's endomorphism is E(x, y) = (beta x, -y), with beta the cube root of unity for which E(G) = [x^2]G.  E satisfies
E^2 - E + 1 = 0, so on a cyclic group of prime order q = 1 mod 3 it can act as one of lambda_1,2 = (1 +- sqrt(-3)) / 2 mod q.  E(Fp)[q] is
Z_q x Z_q for the primes q whose square divides the cofactor, and a generic point of it is no eigenvector; T_e = E(T) - lambda_2 T is one,
with E(T_e) = lambda_1 T_e."""
from util import P, R, golden

X2 = 0xd201000000010000 ** 2
H1 = 0x396c8c005555e1568c00aaab0000aaab           # cofactor of G1: #E(Fp) = H1 * R = 3 11^2 10177^2 859267^2 52437899^2 R


# ---------------------------------------------------------------- affine arithmetic (None = infinity)
def ec_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def ec_neg(a):
    return None if a is None else (a[0], (-a[1]) % P)


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


def enc(a):
    """96-byte affine encoding, all-zero = infinity"""
    return bytes(96) if a is None else a[0].to_bytes(48, "big") + a[1].to_bytes(48, "big")


def dec(b):
    return None if b == bytes(96) else (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:96], "big"))


def generator():
    return dec(bytes.fromhex(golden("g1")["generator"]))


def point_of_order(q, start=1):
    """a point of prime order q | #E(Fp): the q-part of a curve point found by counting x upwards from start + 1, multiplied down to order q"""
    m = H1 * R
    while m % q == 0:
        m //= q
    x = start
    while True:
        x += 1
        rhs = (x ** 3 + 4) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P != rhs:
            continue
        t = ec_mul(m, (x, y))
        if t is None:
            continue
        while ec_mul(q, t) is not None:
            t = ec_mul(q, t)
        return t


# ---------------------------------------------------------------- the endomorphism
def _beta():
    g = generator()
    want = ec_mul(X2 % R, g)
    for c in range(2, 100):
        w = pow(c, (P - 1) // 3, P)
        if w == 1:
            continue
        for b in (w, w * w % P):
            if (b * g[0] % P, (-g[1]) % P) == want:
                return b
    raise AssertionError("no cube root of unity fixes E(G) = [x^2]G")


BETA = _beta()


def endo(a):
    return None if a is None else (BETA * a[0] % P, (-a[1]) % P)


def eigenvalues(q):
    """the roots (1 +- sqrt(-3)) / 2 of l^2 - l + 1 mod a prime q = 1 mod 3"""
    s = next(s for s in range(q) if (s * s + 3) % q == 0)
    h = pow(2, -1, q)
    return (1 + s) * h % q, (1 - s) * h % q


def eigenpoint(q):
    """(T_e, lambda): a point of prime order q with E(T_e) = [lambda] T_e, built as T_e = E(T) - lambda_2 T from a point T of order q"""
    l1, l2 = eigenvalues(q)
    start = 1
    while True:
        t = point_of_order(q, start)
        te = ec_add(endo(t), ec_neg(ec_mul(l2, t)))
        if te is not None:
            assert ec_mul(q, te) is None and endo(te) == ec_mul(l1, te)
            return te, l1
        start = t[0]                                   # T was itself an eigenvector for lambda_2: take the next point


def crt(a, m, b, n):
    """x mod m n with x = a mod m, x = b mod n (coprime moduli)"""
    return (a + (b - a) * pow(m, -1, n) % n * m) % (m * n)


# ---------------------------------------------------------------- which lanes the incomplete formulas cannot serve
def digits(k):
    kb = k + sum(16 << (5 * w) for w in range(26))
    return [((kb >> (5 * w)) & 31) - 16 for w in range(26)]


DBL, INF = "s=t", "s=-t"


def exceptional(k, q, lam):
    """The first exceptional addition of g1_scalar_mul's digit schedule on a point P of order q on which E acts as [lam] (lam mod q),
    or None.  k is reduced mod R and split as k0 + k1 x^2; a digit d of k0 adds [d]P, a digit of k1 adds [d]E(P) = [d lam]P.  The
    accumulator's multiple s of P is tracked mod q: an addition of t P to an accumulator not at infinity is exceptional when s = t (the
    mixed addition meets a doubling, DBL) or s = -t (the sum passes through infinity, INF); either leaves Jacobian Z = 0.
    A subgroup point is (q, lam) = (R, x^2); G + (0, 2) is (3 R, crt(x^2, R, -1, 3)); the order-q eigenpoint of eigenpoint(q) is (q, lambda).
    Tables of points of order 3 or 11 are degenerate before the loop starts (jP = -P for a j <= 16): this predicts the loop only."""
    k %= R
    k1, k0 = divmod(k, X2)
    d0, d1 = digits(k0), digits(k1)
    s, inf = 0, True
    for w in range(25, -1, -1):
        s = 32 * s % q
        for d, t in ((d0[w], d0[w] % q), (d1[w], d1[w] * lam % q)):
            if d == 0:
                continue
            if inf:
                s, inf = t, False
                continue
            if (s - t) % q == 0:
                return DBL
            if (s + t) % q == 0:
                return INF
            s = (s + t) % q
    return None


def edge_scalars():
    ks = [0] + list(range(1, 41)) + [R - 1, R, R + 1, (1 << 256) - 1, X2 - 1, X2, X2 + 1, R - X2]
    ks += [(1 << 124) + 3, (1 << 125) - 1, 5 * X2 + 7, ((1 << 100) + 1) * X2 + 2, 3 * X2 - 40]     # top windows zero in one or both halves
    ks += [(R - j) % R for j in range(2, 8)] + [16, 32 * 16, 32 * 16 + 16]
    return ks
