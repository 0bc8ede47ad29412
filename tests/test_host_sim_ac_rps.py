"""CPU tests of the per-lane scalar and byte work of the AC-rps entries (crypto12381_amd/csrc/ac_rps.hpp) compiled for the host with the bounds
checker (tests/host_sim/ac_rps.cpp, C12381_CHECK_BOUNDS), against Python integers and hashlib: the q family — points, index list, disclosed
fields, one index — with its shared prefix and a tail that fits its block (nI = 4: 67 bytes) or spills into a second one (nI = 8: 75 bytes), the
Schnorr transcript, the exponent convolution of pres with 0, 1, r - 1 in attribute and q positions against a brute-force loop (the kept k
included), s0, and the base list of verify and pres with the bound at which pres refuses."""
import ctypes
import hashlib
import itertools
import os
import subprocess

import pytest

from util import P, R, prng

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t
SHAPES = [(1, ()), (1, (0,)), (2, (1,)), (4, (3, 0)), (4, ()), (4, (0, 1, 2, 3)), (10, (0, 3)), (9, tuple(range(8))), (32, (0, 3)), (32, tuple(range(31))),
          (16, (0, 3)), (5, (4, 2))]


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIM_DIR, "libsim_ac_rps.so")
    src = os.path.join(SIM_DIR, "ac_rps.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def idx_array(I):
    return (ctypes.c_uint32 * max(len(I), 1))(*I)


def raw96(pt):
    return bytes(96) if pt is None else pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")


def enc49(pt):
    return bytes(49) if pt is None else bytes([2 | (pt[1] & 1)]) + pt[0].to_bytes(48, "big")


def raw192(pt):
    """x.b | x.a | y.b | y.a, the library's 192-byte G2 record; pt = (xa, xb, ya, yb)"""
    return bytes(192) if pt is None else b"".join(pt[k].to_bytes(48, "big") for k in (1, 0, 3, 2))


def enc97(pt):
    """ECP2_toOctet compressed: 0x02 | FP2_sign(y) — the parity of y.a, of y.b when y.a is zero — then x.b | x.a"""
    if pt is None:
        return bytes(97)
    xa, xb, ya, yb = pt
    return bytes([2 | ((ya if ya else yb) & 1)]) + xb.to_bytes(48, "big") + xa.to_bytes(48, "big")


def q_want(s1, s2, ts, I, aI, ip):
    msg = enc49(s1) + enc49(s2) + enc97(ts) + b"".join(i.to_bytes(8, "little") for i in I) + b"".join(v.to_bytes(48, "big") for v in aI)
    return int.from_bytes(hashlib.sha3_512(msg + ip.to_bytes(8, "little")).digest(), "big") % R


@pytest.mark.parametrize("nI", [0, 1, 3, 4, 8, 9])
@pytest.mark.parametrize("variant", ["plain", "infinities", "y.a = 0"])
def test_q_family(sim, nI, variant):
    """203 + 56 nI bytes; (195 + 56 nI) mod 72 = 51, 35, 3, 59, 67, 51: the tail is 67 bytes at nI = 4 and 75 — a second block — at nI = 8"""
    nattr = nI + 2
    I = list(range(nI - 1, -1, -1)) if nI != 3 else [4, 0, 2]                  # not ascending: the prefix follows the caller's order
    fp = lambda k: prng(9600 + nI, k, 48) % P
    s1, s2, ts = (fp(0), fp(1)), (fp(2), fp(3) | 1), (fp(4), fp(5), fp(6), fp(7))
    if variant == "infinities":
        s2, ts = None, None
    if variant == "y.a = 0":
        ts = (fp(4), fp(5), 0, fp(7) | 1)
    aI = [prng(9700 + nI, k) % R for k in range(nI)]
    if nI >= 3:
        aI[0], aI[1], aI[2] = 0, R - 1, 1
    L = 195 + 56 * nI
    buf, out = ctypes.create_string_buffer(L + 3), ctypes.create_string_buffer(32 * (nI + 1))
    tail = sim.sim_ac_rps_q(raw96(s1), raw96(s2), raw192(ts), sz(nattr), bytes(I) + bytes(1), sz(nI), b"".join(v.to_bytes(48, "big") for v in aI) + bytes(1),
                            buf, out)
    assert tail == L % 72 + 8 and (nI != 8 or tail == 75) and (nI != 4 or tail == 67)
    want_prefix = enc49(s1) + enc49(s2) + enc97(ts) + b"".join(i.to_bytes(8, "little") for i in I) + b"".join(v.to_bytes(48, "big") for v in aI)
    assert buf.raw[:L] == want_prefix
    for k, ip in enumerate(I + [nattr]):
        assert int.from_bytes(out.raw[32 * k:32 * k + 32], "big") == q_want(s1, s2, ts, I, aI, ip), k


@pytest.mark.parametrize("case", range(4))
def test_c0(sim, case):
    """sigma1_ | C | C0, 147 bytes: two whole blocks and three bytes"""
    pts = [(prng(9800 + case, 2 * k, 48) % P, prng(9800 + case, 2 * k + 1, 48) % P) for k in range(3)]
    if case:
        pts[case - 1] = None
    tr, c = ctypes.create_string_buffer(150), ctypes.create_string_buffer(32)
    assert sim.sim_ac_rps_c0(b"".join(raw96(p) for p in pts), tr, c) == 0
    want = b"".join(enc49(p) for p in pts)
    assert tr.raw[:147] == want
    assert int.from_bytes(c.raw, "big") == int.from_bytes(hashlib.sha3_512(want).digest(), "big") % R


def cross_terms(nattr, I, a, q):
    """pres.cpp:38-55 as written: for every k of sequence(2 n + 1) the valid ii (size_t arithmetic: a negative j is in no set) and the exponent"""
    Ip = list(I) + [nattr]
    J = [j for j in range(nattr) if j not in I]
    out = {}
    for k in range(2 * nattr + 1):
        valid = [ii for ii in range(len(Ip)) if (k + Ip[ii] - nattr - 1) in J]
        if valid:
            out[k] = sum(q[ii] * a[k + Ip[ii] - nattr - 1] for ii in valid) % R
    return out


def conv(sim, nattr, I, a, q):
    e, kept = ctypes.create_string_buffer(32 * (2 * nattr + 1)), ctypes.create_string_buffer(2 * nattr + 1)
    assert sim.sim_ac_rps_conv(sz(nattr), idx_array(I), sz(len(I)), b"".join(v.to_bytes(48, "big") for v in a),
                               b"".join(v.to_bytes(32, "big") for v in q) + bytes(1), e, kept) == 0
    return [int.from_bytes(e.raw[32 * k:32 * k + 32], "big") for k in range(2 * nattr + 1)], list(kept.raw)


@pytest.mark.parametrize("nattr,I", SHAPES)
def test_convolution(sim, nattr, I):
    fills = [lambda s, k: prng(s, k) % R, lambda s, k: 0, lambda s, k: 1, lambda s, k: R - 1, lambda s, k: (0, 1, R - 1)[k % 3]]
    for fa in fills:
        for fq in fills:
            a = [fa(9900, k) for k in range(nattr)]
            q = [fq(9901, t) for t in range(len(I) + 1)]
            terms = cross_terms(nattr, I, a, q)
            want = [terms.get(k, 0) for k in range(2 * nattr + 1)]
            keep = [1 if k in terms else 0 for k in range(2 * nattr + 1)]
            assert conv(sim, nattr, I, a, q) == (want, keep)


def plan(sim, nattr, I, cross):
    y, total = ctypes.create_string_buffer(32), ctypes.create_string_buffer(1)
    if not sim.sim_ac_rps_plan(sz(nattr), idx_array(I), sz(len(I)), int(cross), y, total):
        return None
    return list(y.raw[:total.raw[0]])


def plan_want(nattr, I, cross):
    fixed = [nattr - i for i in I] + [0]
    return fixed + (sorted(cross_terms(nattr, I, [1] * nattr, [1] * (len(I) + 1))) if cross else [])


@pytest.mark.parametrize("nattr,I", SHAPES)
def test_plan(sim, nattr, I):
    """verify's list is the fixed part; pres's list is that, then the kept k ascending — or a refusal exactly when it is longer than 32"""
    assert plan(sim, nattr, I, False) == plan_want(nattr, I, False)
    want = plan_want(nattr, I, True)
    assert plan(sim, nattr, I, True) == (want if len(want) <= 32 else None)


def test_pres_bound(sim):
    """every set fits for nattr <= 12, (13, (1 .. 11)) is the smallest shape that does not; (16, (0, 3)) fills the list exactly and 17 attributes
    are the fewest with the set (0, 3) that pres refuses"""
    assert len(plan_want(13, tuple(range(1, 12)), True)) == 35
    for nattr in range(1, 13):
        for nI in range(nattr + 1):
            for I in itertools.combinations(range(nattr), nI):
                assert len(plan_want(nattr, I, True)) <= 32 and plan(sim, nattr, I, True) is not None, (nattr, I)
    assert len(plan(sim, 16, (0, 3), True)) == 32
    sizes = {nattr: len(plan_want(nattr, (0, 3), True)) for nattr in range(4, 33)}
    first = min(n for n, s in sizes.items() if s > 32)
    assert first == 17 and plan(sim, 17, (0, 3), True) is None and plan(sim, 17, (0, 3), False) == [17, 14, 0]


@pytest.mark.parametrize("nattr,I,cross", [(0, (), 0), (33, (), 0), (33, (0, 3), 1), (4, (4,), 0), (4, (0, 0), 1), (4, (0, 1, 2, 3, 0), 0), (4, (1 << 31,), 1),
                                          (4, (36,), 0), (32, tuple(range(32)), 0), (32, tuple(range(32)), 1), (13, tuple(range(1, 12)), 1)])
def test_plan_refuses(sim, nattr, I, cross):
    """the argument errors, nI + 1 > 32, and a pres list that does not fit"""
    if nattr == 13:
        assert len(plan_want(nattr, I, True)) > 32
    assert plan(sim, nattr, I, cross) is None


@pytest.mark.parametrize("vals", [(0, 0, 0), (1, 1, 0), (R - 1, R - 1, R - 1), (0, 5, 7), (5, 0, 7), (prng(9950, 0) % R, prng(9950, 1) % R, prng(9950, 2) % R)])
def test_s0(sim, vals):
    """s0 = rho + (-c0) z with the reference's Zp negation"""
    c0, z, rho = vals
    out = ctypes.create_string_buffer(32)
    assert sim.sim_ac_rps_s0(*(v.to_bytes(32, "big") for v in vals), out) == 0
    assert int.from_bytes(out.raw, "big") == (rho + (-c0 % R) * z) % R
