"""CPU tests of the per-lane scalar and byte work of the AC-bbs entries (crypto12381_amd/csrc/ac_bbs.hpp) compiled for the host with the bounds
checker (tests/host_sim/ac_bbs.cpp, C12381_CHECK_BOUNDS), against Python integers and hashlib: J derived from I and the argument errors, the
243-byte splits, the range checks and the base-major scalar columns, the transcript and c at message lengths either side of SHA3-512's rate,
and the response scalars s, t, u_j with 0, 1, r - 1, r and 2^256 - 1 in every random and secret position."""
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
CORNERS = (0, 1, R - 1, R, (1 << 256) - 1)


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIM_DIR, "libsim_ac_bbs.so")
    src = os.path.join(SIM_DIR, "ac_bbs.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def order(sim, nattr, I):
    arr = (ctypes.c_uint32 * max(len(I), 1))(*I)
    out = ctypes.create_string_buffer(32)
    return list(out.raw[:nattr]) if sim.sim_ac_bbs_order(sz(nattr), arr, sz(len(I)), out) else None


@pytest.mark.parametrize("nattr,I", [(4, ()), (4, (0, 1, 2, 3)), (4, (3, 0)), (4, (0, 3)), (1, ()), (1, (0,)), (32, (0, 3)), (32, tuple(range(31, -1, -1))), (5, (4, 2))])
def test_base_order(sim, nattr, I):
    """I in the caller's order, then J ascending"""
    assert order(sim, nattr, I) == list(I) + [i for i in range(nattr) if i not in I]


@pytest.mark.parametrize("nattr,I", [(0, ()), (33, ()), (4, (4,)), (4, (0, 0)), (4, (1, 2, 1)), (1, (0, 0)), (4, (0, 1, 2, 3, 0)), (4, (1 << 31,)), (4, (36,))])
def test_base_order_refuses(sim, nattr, I):
    """nattr = 0, nattr above the fixed-base bound, an index >= nattr (one that would shift out of the seen-mask included), a repeated index"""
    assert order(sim, nattr, I) is None


def test_split3(sim):
    n = 3
    cols = ctypes.create_string_buffer(3 * 49 * n)
    recs = [bytes((7 * j + b) % 251 for b in range(243)) for j in range(n)]
    for j, r in enumerate(recs):
        assert sim.sim_ac_bbs_split3(sz(n), sz(j), r, cols) == 0
    for k in range(3):
        for j in range(n):
            assert cols.raw[49 * (k * n + j):49 * (k * n + j + 1)] == recs[j][49 * k:49 * k + 49]


def columns(sim, lanes, perm=None):
    """lanes: equal-length lists of field values below 2^384 -> (columns as integers [k][j], ok bytes)"""
    n, count = len(lanes), len(lanes[0])
    f = b"".join(v.to_bytes(48, "big") for ln in lanes for v in ln)
    cols, ok = ctypes.create_string_buffer(32 * n * count), ctypes.create_string_buffer(n)
    assert sim.sim_ac_bbs_zp_columns(sz(n), sz(count), f, bytes(perm) if perm is not None else None, cols, ok) == 0
    return [[int.from_bytes(cols.raw[32 * (k * n + j):32 * (k * n + j + 1)], "big") for j in range(n)] for k in range(count)], ok.raw


def test_zp_columns_and_range_checks(sim):
    """every Zp field of both records — s, t, u_j, disclosed a_i of a presentation; w and the whole attribute span of pres — at r - 1 (accepted),
    r, 2^256 and 2^384 - 1 (refused), one position at a time; columns are base-major and follow the permutation"""
    for count in (1, 2, 4, 32):
        base = [prng(8100 + count, k) % R for k in range(count)]
        lanes, want_ok = [base], [1]
        for pos in range(count):
            for v, ok in ((R - 1, 1), (0, 1), (R, 0), (1 << 256, 0), ((1 << 384) - 1, 0), (R + (1 << 300), 0)):
                lanes.append(base[:pos] + [v] + base[pos + 1:])
                want_ok.append(ok)
        cols, ok = columns(sim, lanes)
        assert ok == bytes(want_ok)
        for j, ln in enumerate(lanes):
            if want_ok[j]:
                assert [cols[k][j] for k in range(count)] == ln
    perm = [3, 0, 1, 2]                                                  # I = (3, 0), J = (1, 2)
    lanes = [[prng(8200, 4 * j + k) % R for k in range(4)] for j in range(5)]
    cols, ok = columns(sim, lanes, perm)
    assert ok == b"\x01" * 5
    assert all(cols[k][j] == lanes[j][perm[k]] for k in range(4) for j in range(5))
    cols, ok = columns(sim, [[1, 2, 3, R]], perm)                        # the refused field sits at position 0 of the base order
    assert ok == b"\x00"


def enc49(pt):
    return bytes(49) if pt is None else bytes([2 | (pt[1] & 1)]) + pt[0].to_bytes(48, "big")


def raw96(pt):
    return bytes(96) if pt is None else pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")


@pytest.mark.parametrize("msg_len", [0, 1, 31, 32, 68, 69, 70, 71, 72, 140, 141, 142, 200])
def test_transcript_and_challenge(sim, msg_len):
    """msg | A_ | B_ | U with the points as serialize writes them (tag from the parity of y, 49 zeros for infinity) and c = SHA3-512 mod r;
    msg_len + 147 crosses the 72-byte rate at 69 and 141"""
    pts = [(prng(8300 + msg_len, 0, 48) % P, prng(8300 + msg_len, 1, 48) % P), (5, 2 * (msg_len + 1)), (7, 2 * msg_len + 1)]
    if msg_len % 3 == 1:
        pts[1] = None
    msg = prng(8301, msg_len, max(msg_len, 1)).to_bytes(max(msg_len, 1), "big")[:msg_len]
    L = msg_len + 147
    tr, c = ctypes.create_string_buffer(L + 3), ctypes.create_string_buffer(32)
    assert sim.sim_ac_bbs_challenge(msg, sz(msg_len), raw96(pts[0]), raw96(pts[1]), raw96(pts[2]), tr, c) == 0
    want = msg + b"".join(enc49(p) for p in pts)
    assert tr.raw[:L] == want
    assert int.from_bytes(c.raw, "big") == int.from_bytes(hashlib.sha3_512(want).digest(), "big") % R


def responses(sim, lanes, nJ):
    """lanes: (rnd[3 + nJ] below 2^256, c below r, w below r, aJ[nJ] below r)"""
    n = len(lanes)
    rnd = b"".join(v.to_bytes(32, "big") for ln in lanes for v in ln[0])
    c32 = b"".join(ln[1].to_bytes(32, "big") for ln in lanes)
    w48 = b"".join(ln[2].to_bytes(48, "big") for ln in lanes)
    a48 = b"".join(v.to_bytes(48, "big") for ln in lanes for v in ln[3])
    st, u, sc = (ctypes.create_string_buffer(max(k * n, 1)) for k in (96, 48 * nJ, 128))
    assert sim.sim_ac_bbs_responses(sz(n), sz(nJ), rnd, c32, w48, a48, st, u, sc) == 0
    for j, (rn, c, w, aJ) in enumerate(lanes):
        r, alpha, beta = (v % R for v in rn[:3])
        delta = [v % R for v in rn[3:]]
        negw = -w % R
        got = [int.from_bytes(st.raw[96 * j + 48 * k:96 * j + 48 * k + 48], "big") for k in range(2)]
        assert got == [(alpha + r * c) % R, (beta + negw * c) % R], (j, lanes[j])
        got = [int.from_bytes(sc.raw[128 * j + 32 * k:128 * j + 32 * k + 32], "big") for k in range(4)]
        assert got == [r, alpha, negw, beta], (j, lanes[j])
        got = [int.from_bytes(u.raw[48 * (nJ * j + k):48 * (nJ * j + k + 1)], "big") for k in range(nJ)]
        assert got == [(delta[k] + r * c * aJ[k]) % R for k in range(nJ)], (j, lanes[j])


def test_responses_prng(sim):
    for nJ in (0, 1, 2, 30):
        responses(sim, [([prng(8400 + j, k, 32) for k in range(3 + nJ)], prng(8401, j) % R, prng(8402, j) % R, [prng(8403 + j, k) % R for k in range(nJ)])
                        for j in range(40)], nJ)


def test_responses_corner_values_in_every_position(sim):
    nJ = 2
    lanes = []
    base = lambda s: ([prng(s, k, 32) for k in range(3 + nJ)], prng(s, 10) % R, prng(s, 11) % R, [prng(s, 12 + k) % R for k in range(nJ)])
    for pos in range(3 + nJ):                                            # the random positions take any value below 2^256
        for v in CORNERS:
            rn, c, w, aJ = base(8500 + pos)
            rn[pos] = v
            lanes.append((rn, c, w, aJ))
    for v in (0, 1, R - 1):                                              # the secret positions and c take residues only
        rn, c, w, aJ = base(8510)
        lanes.append((rn, v, w, aJ))
        lanes.append((rn, c, v, aJ))                                     # w = 0: -0 = 0, t = beta
        for k in range(nJ):
            lanes.append((rn, c, w, aJ[:k] + [v] + aJ[k + 1:]))
    for v in CORNERS:                                                    # the same corner everywhere
        lanes.append(([v] * (3 + nJ), (v % R), (v % R), [v % R] * nJ))
    lanes.append(([R - 1] * (3 + nJ), R - 1, R - 1, [R - 1] * nJ))
    lanes.append(([0] * (3 + nJ), 0, 0, [0] * nJ))
    responses(sim, lanes, nJ)
