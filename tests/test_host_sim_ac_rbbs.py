"""CPU tests of the per-lane scalar and byte work of the AC-rbbs entries (crypto12381_amd/csrc/ac_rbbs.hpp) compiled for the host with the bounds
checker (tests/host_sim/ac_rbbs.cpp, C12381_CHECK_BOUNDS), against Python integers and hashlib: the q family with its shared prefix inside one
block, across blocks and on a block boundary, the five-point transcript at message lengths either side of SHA3-512's rate, the exponent
convolution of redact with 0, 1, r - 1 in attribute and q positions against a brute-force double loop (the kept k included), and redact's base
list: three contiguous ranges that hold exactly the terms of C_I, D and C_J."""
import ctypes
import hashlib
import os
import subprocess

import pytest

from util import P, R, prng

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t
SHAPES = [(1, ()), (1, (0,)), (2, (1,)), (2, (0,)), (4, (3, 0)), (4, ()), (4, (0, 1, 2, 3)), (16, (0, 3)), (16, (15, 7, 8, 0)), (5, (4, 2))]


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIM_DIR, "libsim_ac_rbbs.so")
    src = os.path.join(SIM_DIR, "ac_rbbs.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def idx_array(I):
    return (ctypes.c_uint32 * max(len(I), 1))(*I)


@pytest.mark.parametrize("nI", [0, 1, 2, 3, 32])
def test_q_family(sim, nI):
    """48 nI + 8 bytes: 8 (nI = 0), 56 (inside one 72-byte block), 104 (crosses), 152 (the prefix ends on a block boundary), 1544; every i in 0 .. 31"""
    aI = [prng(8600 + nI, k) % R for k in range(nI)]
    if nI >= 3:
        aI[0], aI[1], aI[2] = 0, R - 1, 1
    pre = b"".join(v.to_bytes(48, "big") for v in aI)
    out = ctypes.create_string_buffer(32 * 32)
    assert sim.sim_ac_rbbs_q(pre + bytes(3), sz(nI), sz(32), out) == 0
    for i in range(32):
        want = int.from_bytes(hashlib.sha3_512(pre + i.to_bytes(8, "little")).digest(), "big") % R
        assert int.from_bytes(out.raw[32 * i:32 * i + 32], "big") == want, i


def raw96(pt):
    return bytes(96) if pt is None else pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")


def enc49(pt):
    return bytes(49) if pt is None else bytes([2 | (pt[1] & 1)]) + pt[0].to_bytes(48, "big")


@pytest.mark.parametrize("msg_len", [0, 1, 32, 42, 43, 44, 114, 115, 200])
def test_transcript_and_challenge(sim, msg_len):
    """msg | A_ | B_ | C_J_ | D_ | U; msg_len + 245 is 71 mod the rate at 42 and 0 at 43"""
    pts = [(prng(8700 + msg_len, 2 * k, 48) % P, prng(8700 + msg_len, 2 * k + 1, 48) % P) for k in range(5)]
    pts[msg_len % 5] = None
    msg = prng(8701, msg_len, max(msg_len, 1)).to_bytes(max(msg_len, 1), "big")[:msg_len]
    L = msg_len + 245
    tr, c = ctypes.create_string_buffer(L + 3), ctypes.create_string_buffer(32)
    assert sim.sim_ac_rbbs_challenge(msg, sz(msg_len), b"".join(raw96(p) for p in pts), tr, c) == 0
    want = msg + b"".join(enc49(p) for p in pts)
    assert tr.raw[:L] == want
    assert int.from_bytes(c.raw, "big") == int.from_bytes(hashlib.sha3_512(want).digest(), "big") % R


def conv(sim, nattr, I, a, q):
    e, kept = ctypes.create_string_buffer(64 * nattr), ctypes.create_string_buffer(2 * nattr)
    assert sim.sim_ac_rbbs_conv(sz(nattr), idx_array(I), sz(len(I)), b"".join(v.to_bytes(48, "big") for v in a),
                                b"".join(v.to_bytes(32, "big") for v in q) + bytes(1), e, kept) == 0
    return [int.from_bytes(e.raw[32 * k:32 * k + 32], "big") for k in range(2 * nattr)], list(kept.raw)


@pytest.mark.parametrize("nattr,I", SHAPES)
def test_convolution(sim, nattr, I):
    """e_k = sum_(i in I, k - nattr + i in J) q_i a_(k - nattr + i) against a double loop over (i, j), on which k it keeps as well"""
    J = [j for j in range(nattr) if j not in I]
    fills = [lambda s, k: prng(s, k) % R, lambda s, k: 0, lambda s, k: 1, lambda s, k: R - 1, lambda s, k: (0, 1, R - 1)[k % 3]]
    for fa in fills:
        for fq in fills:
            a = [fa(8800, k) for k in range(nattr)]
            q = [fq(8801, t) for t in range(len(I))]
            want, keep = [0] * (2 * nattr), [0] * (2 * nattr)
            for t, i in enumerate(I):
                for j in J:
                    want[nattr - i + j] = (want[nattr - i + j] + q[t] * a[j]) % R
                    keep[nattr - i + j] = 1
            assert conv(sim, nattr, I, a, q) == (want, keep)


def plan(sim, nattr, I):
    y, acol, counts = ctypes.create_string_buffer(32), ctypes.create_string_buffer(16), ctypes.create_string_buffer(4)
    if not sim.sim_ac_rbbs_plan(sz(nattr), idx_array(I), sz(len(I)), y, acol, counts):
        return None
    return list(y.raw), list(acol.raw), list(counts.raw)


@pytest.mark.parametrize("nattr,I", SHAPES + [(16, tuple(range(16))), (16, ()), (16, (8,)), (16, tuple(range(0, 16, 2)))])
def test_redact_plan(sim, nattr, I):
    """one list, no record twice, at most 2 nattr - 1 entries; [0, nI) is I, [d_first, d_first + nD) is K_D, [cj_first, total) is J; the scalar
    columns follow the list"""
    y, acol, (total, d_first, nD, cj_first) = plan(sim, nattr, I)
    J = [j for j in range(nattr) if j not in I]
    KD = sorted({nattr - i + j for i in I for j in J})
    nI = len(I)
    assert total <= max(2 * nattr - 1, 1) and len(set(y[:total])) == total and nattr not in y[:total]
    assert sorted(y[:nI]) == sorted(I) and sorted(y[cj_first:total]) == J and sorted(y[d_first:d_first + nD]) == KD
    assert acol[:nI] == y[:nI] and acol[nI:nattr] == y[cj_first:total]
    assert [i for i in y[:nI] if i in I] == [i for i in I if i not in KD] + [i for i in I if i in KD]


@pytest.mark.parametrize("nattr,I", [(0, ()), (17, ()), (17, (0, 3)), (32, (0,)), (4, (4,)), (4, (0, 0)), (4, (0, 1, 2, 3, 0)), (4, (1 << 31,)), (4, (36,))])
def test_redact_plan_refuses(sim, nattr, I):
    assert plan(sim, nattr, I) is None
