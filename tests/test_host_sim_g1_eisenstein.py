"""CPU tests of the base-8 Eisenstein multiplication g1_scalar_mul_eis (g1.hpp) through the stand-alone program tests/host_sim/g1_eisenstein.cpp, built with
C12381_CHECK_BOUNDS: the C++ recoder against the Python reference (tests/g1_eisenstein.py) on the same inputs, and the scalar
multiplication against the oracle byte for byte on the golden G1 vectors and on edge scalars and points, with the lanes that take the
complete path compared with the predictor.

Digits in the top position: every coefficient stays non-negative through the recoding, so the highest non-zero digit of a scalar is itself a
pair of non-negative coefficients and position 43 holds nothing, 1 or psi.  "One scalar per class in the top position" is therefore: every
class that occurs as the highest digit of a seeded search, at position 43 and below it."""
import os
import random
import struct
import subprocess

import pytest

from g1_eisenstein import CHAIN_UNITS, CLASSES, DBL, INF, TABLE, code, edge_scalars, exceptional, packed, recode, split
from g1_torsion import X2, crt, ec_add, eigenpoint, enc, generator, point_of_order
from util import P, R, golden, prng

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")


@pytest.fixture(scope="module")
def prog():
    exe = os.path.join(SIM_DIR, "g1_eisenstein")
    src = os.path.join(SIM_DIR, "g1_eisenstein.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-pthread", "-o", exe, src], check=True)
    return exe


def _run(prog, mode, data):
    r = subprocess.run([prog, mode], input=data, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def _hexline(words):
    return " ".join("%08x" % w for w in words)


def test_tables_agree_with_python(prog):
    lines = _run(prog, "table", b"").decode().split("\n")
    want = [(code(e, u) | ((d[0] < 0) << 7) | ((d[1] < 0) << 8)) for e, u, d in CLASSES]
    assert [int(t, 16) for t in lines[0].split()] == want
    deltas, prev = 0, 0
    for i, u in enumerate(CHAIN_UNITS):
        deltas |= ((u - prev) % 6) << (3 * i)
        prev = u
    assert int(lines[1], 16) == deltas
    assert lines[2] == "1"                                     # FP_BETA_B = FP_BETA_A^2


def _pairs():
    top0, top1 = X2 - 1, (1 << 128) - 1
    pairs = [(a, b) for a in range(65) for b in range(65)]
    pairs += [(top0 + i, top1 + j) for i in (-2, -1, 0) for j in (-2, -1, 0)]
    words = [0xffffffff, 0xaaaaaaaa, 0x55555555, 0x00000000, 0x92492492]
    pats = [sum(w << (32 * i) for i in range(4)) for w in words]
    pairs += [(a, b) for a in pats for b in pats]
    rng = random.Random(44002)
    pairs += [(rng.randrange(X2), rng.randrange(1 << 128)) for _ in range(100000)]
    return pairs


def test_recoder_agrees_with_python(prog):
    pairs = _pairs()
    out = _run(prog, "recode", "".join("%x %x\n" % p for p in pairs).encode()).decode().split("\n")
    assert len(out) == len(pairs) + 1
    bad = [p for p, line in zip(pairs, out) if line != _hexline(packed(*p))]
    assert bad == [], bad[:4]


def test_scalar_digits_agree_with_python(prog):
    ks = edge_scalars() + [prng(44004, i) % (1 << 256) for i in range(2000)]
    out = _run(prog, "digits", "".join("%x\n" % k for k in ks).encode()).decode().split("\n")
    bad = [k for k, line in zip(ks, out) if line != _hexline(packed(*split(k)))]
    assert bad == [], bad[:4]
    low = {recode(*split(k))[0][:2] for k in ks if k % R}
    assert len(low) >= 63                                      # every non-zero class occurs in the lowest position


def test_mul_golden_and_edge_lanes(prog, oracle_port):
    """golden points (subgroup and off the subgroup, the small-scalar rows included) with their own scalars, then the generator, a second
    subgroup point, the point at infinity and the two points of order 3 with every edge scalar: every output byte equals the oracle's (and
    the stored vectors), no bound is violated (the program aborts on one), the order-3 lanes take the complete path and the subgroup and
    infinity lanes are those the predictor names"""
    g = golden("g1")
    lanes = []                                                 # (point, scalar, kind, stored result or None)
    for p, s, m in zip(g["points"], g["scalars"], g["mul96"]):
        lanes.append((bytes.fromhex(p), int(s, 16), "sub", bytes.fromhex(m)))
    for p, s, m in zip(g["offsubgroup_points"], g["offsubgroup_scalars"], g["offsubgroup_mul96"]):
        lanes.append((bytes.fromhex(p), int(s, 16), "off", bytes.fromhex(m)))
    for p, s, m in zip(g["offsubgroup_small_points"], g["offsubgroup_small_scalars"], g["offsubgroup_small_mul96"]):
        lanes.append((bytes.fromhex(p), int(s, 16), "off", bytes.fromhex(m)))
    ks = edge_scalars()
    pts = [(enc(generator()), "sub"), (bytes.fromhex(g["points"][3]), "sub"), (bytes(96), "inf"), (enc((0, 2)), "o3"), (enc((0, P - 2)), "o3"),
           (bytes.fromhex(g["offsubgroup_points"][1]), "off")]
    for pb, kind in pts:
        lanes += [(pb, k, kind, None) for k in ks]
    n = len(lanes)
    P_ = b"".join(ln[0] for ln in lanes)
    S_ = b"".join(ln[1].to_bytes(32, "big") for ln in lanes)
    out = _run(prog, "mul", struct.pack("<Q", n) + P_ + S_)
    assert len(out) == 97 * n
    got = b"".join(out[97 * i:97 * i + 96] for i in range(n))
    comp = [out[97 * i + 96] for i in range(n)]
    exp = oracle_port.g1_mul(P_, S_, 96, 8)
    bad = [i for i in range(n) if got[96 * i:96 * i + 96] != exp[96 * i:96 * i + 96]]
    assert bad == [], [(i, lanes[i][2], hex(lanes[i][1])) for i in bad[:8]]
    assert all(len(ln[3]) == 96 for ln in lanes if ln[3] is not None)
    assert [i for i in range(n) if lanes[i][3] is not None and lanes[i][3] != got[96 * i:96 * i + 96]] == []
    for i, (pb, k, kind, _) in enumerate(lanes):
        if kind == "sub":
            assert comp[i] == (exceptional(k, R, X2 % R) is not None), (i, hex(k))
            assert comp[i] == 0
        elif kind == "inf":
            assert comp[i] == 0
        elif kind == "o3":                                     # beta x = x: the first step of the chain has h = 0
            assert exceptional(k, 3, 2) == (TABLE if k % R else None)
            assert comp[i] == (1 if k % R else 0), (i, hex(k))
    assert sum(1 for ln, c in zip(lanes, comp) if ln[2] == "o3" and c) >= 2 * (len(ks) - 2)


def _mul(prog, P_, S_):
    n = len(S_) // 32
    out = _run(prog, "mul", struct.pack("<Q", n) + P_ + S_)
    assert len(out) == 97 * n
    return b"".join(out[97 * i:97 * i + 96] for i in range(n)), [out[97 * i + 96] for i in range(n)]


def test_mul_torsion_lanes_take_the_predicted_exceptions(prog, oracle_port):
    """Points on which the loop itself meets acc = +-T: the eigenpoint of order 10177 (psi acts as a residue; about 44 x 2 / q of its lanes),
    a point of order 11 (11 is inert: multiples live in Z[psi] / 11, about half of the lanes; its table is regular, no difference of two
    entries being divisible by 11) and G + (0, 2) of order 3r (none).  1500 seeded 256-bit scalars each plus the edge scalars: every
    output byte equals the oracle's and the lanes on the complete path are exactly the predicted ones, both kinds of exception present"""
    ks = edge_scalars() + [prng(44005, i) % (1 << 256) for i in range(1500)]
    te, lam = eigenpoint(10177)
    o11 = point_of_order(11)
    g3 = ec_add(generator(), (0, 2))
    cases = [(te, 10177, lam), (o11, 11, None), (g3, 3 * R, crt(X2, R, -1, 3))]
    P_ = b"".join(enc(pt) * len(ks) for pt, _, _ in cases)
    S_ = b"".join(k.to_bytes(32, "big") for k in ks) * len(cases)
    want = [exceptional(k, q, l) for _, q, l in cases for k in ks]
    got, comp = _mul(prog, P_, S_)
    exp = oracle_port.g1_mul(P_, S_, 96, 8)
    m = len(want)
    bad = [i for i in range(m) if got[96 * i:96 * i + 96] != exp[96 * i:96 * i + 96]]
    assert bad == [], bad[:8]
    assert comp == [0 if w is None else 1 for w in want], [(i, comp[i], want[i]) for i in range(m) if comp[i] != (want[i] is not None)][:8]
    n = len(ks)
    eig, el = want[:n], want[n:2 * n]
    print("complete path: eigenpoint %d of %d (s=t %d, s=-t %d), order 11 %d, G + T3 %d" % (
        n - eig.count(None), n, eig.count(DBL), eig.count(INF), n - el.count(None), n - want[2 * n:].count(None)))
    assert TABLE not in want
    assert eig.count(DBL) + eig.count(INF) >= 5 and el.count(DBL) > 50 and el.count(INF) > 50
    assert want[2 * n:].count(None) == n
