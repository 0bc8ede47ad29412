"""CPU tests of the G1 scalar multiplication's fast path (g1.hpp: co-Z affine table, Jacobian doublings and mixed additions) and of
its complete fallback, under the bounds checker (tests/host_sim/g1_coz.cpp, C12381_CHECK_BOUNDS).  Results are compared with the
oracle lane by lane, and the set of lanes that took the complete path is compared with the set the formulas predict (g1_torsion.py).
Two causes give a lane Jacobian Z = 0, and the tests reach them with different points:
- a table built on a point of order 3 or 11 (jP = -P for some j <= 16): every such lane with k != 0 mod r (the edge test);
- an addition acc = +-T inside the loop: never for a point of G1 or of G1 + T3, whose multiples need s = +-t mod r, which the reduced
  GLV halves exclude (the edge test's "sub" and "mixed3" kinds predict and see none); but for eigenpoints of E(x, y) = (beta x, -y) of
  order 10177 and 859267, where s = +-t mod q happens in about 1 % of random lanes, both as a doubling (s = t) and through infinity
  (s = -t) (the eigenpoint test)."""
import ctypes
import os
import subprocess

import pytest

from g1_torsion import DBL, INF, X2, crt, ec_add, ec_mul, edge_scalars, eigenpoint, enc, exceptional, point_of_order
from util import P, R, golden, prng, scalars

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t


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
            return exceptional(k, 3 * R, crt(X2, R, -1, 3)) is not None if kind == "mixed3" else exceptional(k, R, X2 % R) is not None
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


def test_coz_eigenpoint_lanes_take_the_loop_exception(coz, oracle_port):
    """Eigenpoints T_e of order q = 10177 and 859267 (E(T_e) = lambda T_e) with 4000 seeded random 256-bit scalars each plus the edge
    scalars: results equal the oracle's lane by lane, and the lanes that take the complete path are exactly those whose digit schedule
    meets s = +-t mod q, with both cases present"""
    n = 4000
    ks = edge_scalars() + [prng(9301, i) % (1 << 256) for i in range(n)]
    P_, S_, want = b"", b"", []
    for q in (10177, 859267):
        te, lam = eigenpoint(q)
        P_ += enc(te) * len(ks)
        S_ += b"".join(k.to_bytes(32, "big") for k in ks)
        want += [exceptional(k, q, lam) for k in ks]
    got, comp = run(coz, P_, S_)
    exp = oracle_port.g1_mul(P_, S_, 96, 8)
    m = len(want)
    bad = [i for i in range(m) if got[96 * i:96 * i + 96] != exp[96 * i:96 * i + 96]]
    assert bad == [], bad[:8]
    assert comp == [0 if w is None else 1 for w in want], [(i, comp[i], want[i]) for i in range(m) if comp[i] != (want[i] is not None)][:8]
    print("eigenpoint lanes on the complete path: %d of %d (s=t: %d, s=-t: %d)" % (sum(comp), m, want.count(DBL), want.count(INF)))
    assert sum(comp) >= 30 and want.count(DBL) > 0 and want.count(INF) > 0
