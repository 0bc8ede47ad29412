"""CPU tests of the per-signature scalar work of bbs04 sign (crypto12381_amd/csrc/bbs04_sign.hpp) compiled for the host with the bounds
checker (tests/host_sim/bbs04_sign.cpp, C12381_CHECK_BOUNDS): the reduction of the seven random scalars, the nine fixed-base scalar columns
(negations with -0 = 0) and the six Zp fields of the signature equal Python integer arithmetic — for prng inputs and for the corner values
0, 1, r - 1, r and 2^256 - 1 in every input position, c = 0 and x = 0 included."""
import ctypes
import hashlib
import os
import subprocess

import pytest

from util import R, prng

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t
CORNERS = (0, 1, R - 1, R, (1 << 256) - 1)


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIM_DIR, "libsim_bbs04_sign.so")
    src = os.path.join(SIM_DIR, "bbs04_sign.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def model(rnd, c, x):
    """(nine columns, r_x, six fields) of one lane as integers: bbs.cpp:37-56 on scalars reduced mod r"""
    a, b, ra, rb, rx, rd1, rd2 = (v % R for v in rnd)
    cols = [a, b, (a + b) % R, ra, rb, -rd1 % R, -rd2 % R, -(rd1 + rd2) % R, -(ra + rb) % R]
    cx = c * x % R
    f = [c, (ra + c * a) % R, (rb + c * b) % R, (rx + cx) % R, (rd1 + a * cx) % R, (rd2 + b * cx) % R]
    return cols, rx, f


def run(sim, lanes):
    """lanes: (rnd[7], c, x) with rnd values below 2^256, c and x below r"""
    n = len(lanes)
    rnd = b"".join(v.to_bytes(32, "big") for ln in lanes for v in ln[0])
    c32 = b"".join(ln[1].to_bytes(32, "big") for ln in lanes)
    x32 = b"".join(ln[2].to_bytes(32, "big") for ln in lanes)
    cols, rx, f = (ctypes.create_string_buffer(k * n) for k in (288, 32, 288))
    assert sim.sim_bbs04_sign(sz(n), rnd, c32, x32, cols, rx, f) == 0
    for j, ln in enumerate(lanes):
        wc, wrx, wf = model(*ln)
        got_c = [int.from_bytes(cols.raw[32 * (9 * j + k):32 * (9 * j + k + 1)], "big") for k in range(9)]
        got_f = [int.from_bytes(f.raw[48 * (6 * j + k):48 * (6 * j + k + 1)], "big") for k in range(6)]
        assert got_c == wc, (j, ln)
        assert int.from_bytes(rx.raw[32 * j:32 * j + 32], "big") == wrx, (j, ln)
        assert got_f == wf, (j, ln)


def test_prng_lanes(sim):
    run(sim, [([prng(7100 + j, k, 32) for k in range(7)], prng(7200, j) % R, prng(7300, j) % R) for j in range(200)])


def test_corner_values_in_every_position(sim):
    lanes = []
    for pos in range(7):
        for v in CORNERS:
            rnd = [prng(7400 + pos, k, 32) for k in range(7)]
            rnd[pos] = v
            lanes.append((rnd, prng(7401, pos) % R, prng(7402, pos) % R))
    for v in CORNERS:                                        # the same corner in all seven positions: sums and negated sums at their edges
        lanes.append(([v] * 7, prng(7403, v % 97) % R, prng(7404, v % 97) % R))
    base = [prng(7405, k, 32) for k in range(7)]
    for v in (0, 1, R - 1):                                  # c and x take residues only
        lanes.append((base, v, prng(7406, 0) % R))
        lanes.append((base, prng(7407, 0) % R, v))
        lanes.append(([R - 1] * 7, v, R - 1))
    lanes.append(([0] * 7, 0, 0))
    pairs = [(a, b) for a in CORNERS for b in CORNERS]       # the two operands of every sum: alpha + beta, r_alpha + r_beta, r_delta1 + r_delta2
    for a, b in pairs:
        lanes.append(([a, b, a, b, prng(7408, 0, 32), a, b], R - 1, R - 1))
    run(sim, lanes)


def test_negations_keep_zero(sim):
    """mod_negate: -0 = 0, not r — for a zero input, an input equal to r, and sums that vanish mod r"""
    rnd = [0, 0, 5, R - 5, 0, R, 0]                          # r_alpha + r_beta = r, r_delta1 = r
    cols, _, _ = model(rnd, 1, 1)
    assert cols[5] == cols[6] == cols[7] == cols[8] == 0
    run(sim, [(rnd, 1, 1)])


def test_c_from_digest(sim):
    """c = SHA3-512 digest as a big-endian integer mod r (Zp from_hash), the form bbs04_sign_responses takes it in"""
    for i in range(50):
        d = hashlib.sha3_512(b"bbs04 sign|%d" % i).digest()
        out = ctypes.create_string_buffer(32)
        assert sim.sim_bbs04_c_from_digest(d, out) == 0
        assert int.from_bytes(out.raw, "big") == int.from_bytes(d, "big") % R
    for d in (bytes(64), b"\xff" * 64, (R << 256).to_bytes(64, "big")):
        out = ctypes.create_string_buffer(32)
        assert sim.sim_bbs04_c_from_digest(d, out) == 0
        assert int.from_bytes(out.raw, "big") == int.from_bytes(d, "big") % R
