"""CPU tests of the G1 scalar multiplication's fast path (g1.hpp: co-Z affine table, Jacobian doublings and mixed additions) and of
its complete fallback, under the bounds checker (tests/host_sim/g1_coz.cpp, C12381_CHECK_BOUNDS).  Results are compared with the
oracle lane by lane, and the set of lanes that took the complete path is compared with the set the formulas predict: the lanes whose
Jacobian Z becomes 0 (an addition acc = +-T, a table built on a point of order 3 or 11), and never a lane of a random subgroup batch."""
import ctypes
import os
import subprocess

import pytest

from util import P, R, golden, prng, scalars

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t

X2 = 0xd201000000010000 ** 2
H1 = 0x396c8c005555e1568c00aaab0000aaab           # cofactor of G1: #E(Fp) = H1 * R


@pytest.fixture(scope="module")
def coz():
    so = os.path.join(SIM_DIR, "libsim_g1coz.so")
    src = os.path.join(SIM_DIR, "g1_coz.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-pthread", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def run(coz, pts, sc):
    n = len(sc) // 32
    out = ctypes.create_string_buffer(96 * n)
    comp = ctypes.create_string_buffer(n)
    assert coz.sim_g1coz_mul_batch(sz(n), pts, sc, out, comp) == 0
    return out.raw, list(comp.raw)


# ---------------------------------------------------------------- affine arithmetic on E: y^2 = x^3 + 4 (None = infinity)
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


def ec_mul(k, a):
    r = None
    while k:
        if k & 1:
            r = ec_add(r, a)
        a = ec_add(a, a)
        k >>= 1
    return r


def enc(a):
    return bytes(96) if a is None else a[0].to_bytes(48, "big") + a[1].to_bytes(48, "big")


def point_of_order(q):
    """a point of prime order q | #E(Fp): the q-part of a curve point found by counting x upwards, multiplied down to order q"""
    m = H1 * R
    while m % q == 0:
        m //= q
    x = 1
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


# ---------------------------------------------------------------- which lanes the incomplete formulas cannot serve
def digits(k):
    kb = k + sum(16 << (5 * w) for w in range(26))
    return [((kb >> (5 * w)) & 31) - 16 for w in range(26)]


def exceptional(k, tor=1):
    """the digit schedule of g1_scalar_mul on P = G' + T with G' of order R and T of order tor (1 or 3; the endomorphism acts as x^2 on
    G' and, T being (0, +-2), as -1 on T), tracked as the accumulator's multiples (s mod R, s mod tor): an addition of a table point t
    with the accumulator not at infinity is exceptional when s = +-t in both parts"""
    k %= R
    k1, k0 = divmod(k, X2)
    d0, d1 = digits(k0), digits(k1)
    s, inf, exc = (0, 0), True, False
    for w in range(25, -1, -1):
        s = (32 * s[0] % R, 32 * s[1] % tor)
        for d, t in ((d0[w], (d0[w] % R, d0[w] % tor)), (d1[w], (d1[w] * X2 % R, -d1[w] % tor))):
            if d == 0:
                continue
            if inf:
                s, inf = t, False
                continue
            if all((a - b) % m == 0 for a, b, m in zip(s, t, (R, tor))) or all((a + b) % m == 0 for a, b, m in zip(s, t, (R, tor))):
                exc = True
            s = ((s[0] + t[0]) % R, (s[1] + t[1]) % tor)
    return exc


def edge_scalars():
    ks = [0] + list(range(1, 41)) + [R - 1, R, R + 1, (1 << 256) - 1, X2 - 1, X2, X2 + 1, R - X2]
    ks += [(1 << 124) + 3, (1 << 125) - 1, 5 * X2 + 7, ((1 << 100) + 1) * X2 + 2, 3 * X2 - 40]     # top windows zero in one or both halves
    ks += [(R - j) % R for j in range(2, 8)] + [16, 32 * 16, 32 * 16 + 16]
    return ks


def test_coz_edge_points_and_scalars(coz, oracle_port):
    gen_b = bytes.fromhex(golden("g1")["generator"])
    gen = (int.from_bytes(gen_b[:48], "big"), int.from_bytes(gen_b[48:], "big"))
    sub = ec_mul(prng(9101, 0) % R, gen)
    o3a, o3b = (0, 2), (0, P - 2)
    o11 = point_of_order(11)
    off = golden("g1")["offsubgroup_points"][:2]
    # points: (encoding, kind)
    pts = [(enc(gen), "sub"), (enc(sub), "sub"), (bytes(96), "inf"), (enc(o3a), "small"), (enc(o3b), "small"), (enc(o11), "small"),
           (enc(ec_add(gen, o3a)), "mixed3")] + [(bytes.fromhex(h), "off") for h in off]
    ks = edge_scalars()
    P_, S_, kinds = b"", b"", []
    for pb, kind in pts:
        for k in ks:
            P_ += pb
            S_ += (k % (1 << 256)).to_bytes(32, "big")
            kinds.append((kind, k))
    got, comp = run(coz, P_, S_)
    n = len(kinds)
    exp = oracle_port.g1_mul(P_, S_, 96, 4)
    bad = [i for i in range(n) if got[96 * i:96 * i + 96] != exp[96 * i:96 * i + 96]]
    assert bad == [], [kinds[i] for i in bad[:8]]

    def expected(kind, k):
        if kind == "inf":
            return False
        if kind == "small":                       # the table's ZADDU chain meets jP = -P: Z_T = 0, every lane but k = 0 (mod R)
            return k % R != 0
        if kind in ("sub", "mixed3"):             # mixed3 = G + (0, 2), of order 3R: its table is regular
            return exceptional(k, 3 if kind == "mixed3" else 1)
        return False                              # points of large order off the subgroup: none of these scalars meets an exception

    want = [1 if expected(kind, k) else 0 for kind, k in kinds]
    assert comp == want, [(kinds[i], comp[i]) for i in range(n) if comp[i] != want[i]][:8]
    # the fallback is exercised: every small-order lane with k != 0 mod R takes it, subgroup lanes with small scalars do not
    assert sum(comp) >= 3 * (len(ks) - 2)
    assert not any(c for (kind, k), c in zip(kinds, comp) if kind == "sub" and 0 < k <= 40)


def test_coz_random_subgroup_lanes_never_fall_back(coz, oracle_port):
    """10^4 random points of G1 with random scalars below 2^256: results equal the oracle's, no lane takes the complete path"""
    n = 10000
    gen = bytes.fromhex(golden("g1")["generator"])
    pts = oracle_port.g1_mul(gen * n, scalars(9201, n), 96, 8)
    sc = scalars(9202, n, 1 << 256)
    got, comp = run(coz, pts, sc)
    assert sum(comp) == 0
    assert got == oracle_port.g1_mul(pts, sc, 96, 8)
