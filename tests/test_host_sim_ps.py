"""CPU tests of the per-lane scalar work of the PS wire entries (crypto12381_amd/csrc/ps.hpp) compiled for the host with the bounds checker
(tests/host_sim/ps_wire.cpp, C12381_CHECK_BOUNDS): the 98-byte split, the message scalars of both modes — SHA3-512 mod r at lengths either side
of the 72-byte rate, encode_to<Zp> units at lengths either side of the 31-byte unit — parse<Zp>'s range check, and the signing scalars
(t, t e), e = x + sum y_i m_i, against hashlib, the oracle's encode_to_zp / zp_from_hash and Python integers, with the corner values 0, 1,
r - 1, r, 2^256 - 1 in every position of x, y_i and t and a lane with e = 0."""
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
HASH, ENCODE = 0, 1
HASH_LENS = (0, 1, 71, 72, 73, 143, 144, 145)             # the SHA3-512 rate is 72
ENCODE_LENS = (0, 1, 30, 31, 32, 62, 63, 93)              # units of 31 bytes, nY = 3
CORNERS = (0, 1, R - 1, R, (1 << 256) - 1)


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIM_DIR, "libsim_ps_wire.so")
    src = os.path.join(SIM_DIR, "ps_wire.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def msg_bytes(seed, j, length):
    return prng(seed, j, max(length, 1)).to_bytes(max(length, 1), "big")[:length]


def scalars_of(orc, mode, msg):
    """the message scalars of one message as integers"""
    if mode == HASH:
        d = hashlib.sha3_512(msg).digest()
        m = int.from_bytes(d, "big") % R
        assert orc.zp_from_hash(d) == m.to_bytes(32, "big")
        return [m]
    enc = orc.encode_to_zp(msg)
    return [int.from_bytes(enc[32 * i:32 * i + 32], "big") for i in range(len(enc) // 32)]


def test_split(sim):
    n = 7
    sig = b"".join(prng(7500, j, 98).to_bytes(98, "big") for j in range(n))
    out = ctypes.create_string_buffer(98 * n)
    assert sim.sim_ps_split(sz(n), sig, out) == 0
    for j in range(n):
        assert out.raw[49 * j:49 * j + 49] == sig[98 * j:98 * j + 49]
        assert out.raw[49 * (n + j):49 * (n + j) + 49] == sig[98 * j + 49:98 * j + 98]


@pytest.mark.parametrize("mode,lens", [(HASH, HASH_LENS), (ENCODE, ENCODE_LENS)])
def test_message_scalars(sim, oracle_port, mode, lens):
    n = 9                                                   # every alignment of the message start twice
    for length in lens:
        msgs = [msg_bytes(7510 + mode, 100 * length + j, length) for j in range(n)]
        want = [scalars_of(oracle_port, mode, m) for m in msgs]
        nmsg = 1 if mode == HASH else (length + 30) // 31
        out = ctypes.create_string_buffer(max(32 * n * nmsg, 1))
        assert sim.sim_ps_messages(mode, sz(n), sz(length), b"".join(msgs), out) == nmsg
        for j in range(n):
            got = [int.from_bytes(out.raw[32 * (i * n + j):32 * (i * n + j) + 32], "big") for i in range(nmsg)]
            assert got == want[j], (mode, length, j)


def test_encode_unit_rule(sim, oracle_port):
    """0x01, the unit's bytes, a short last unit left-aligned and zero-filled — spelled out, apart from the oracle"""
    msg = bytes(range(1, 41))
    out = ctypes.create_string_buffer(64)
    assert sim.sim_ps_messages(ENCODE, sz(1), sz(40), msg, out) == 2
    assert out.raw == b"\x01" + msg[:31] + b"\x01" + msg[31:] + bytes(22)
    assert out.raw == oracle_port.encode_to_zp(msg)


def test_parse_zp_range_check(sim):
    for v, ok in ((0, 1), (1, 1), (R - 1, 1), (R, 0), (R + 1, 0), ((1 << 256) - 1, 0), (1 << 256, 0), ((1 << 384) - 1, 0), ((1 << 383) + 5, 0)):
        out = ctypes.create_string_buffer(32)
        assert sim.sim_zp_parse48(v.to_bytes(48, "big"), out) == ok, hex(v)
        assert int.from_bytes(out.raw, "big") == v % (1 << 256)


def run_sign(sim, orc, mode, nY, length, lanes):
    """lanes: (x, [y_i], t, msg) with x, y_i below 2^384 and t below 2^256"""
    n = len(lanes)
    x48 = b"".join(ln[0].to_bytes(48, "big") for ln in lanes)
    y48 = b"".join(v.to_bytes(48, "big") for ln in lanes for v in ln[1])
    t32 = b"".join(ln[2].to_bytes(32, "big") for ln in lanes)
    msgs = b"".join(ln[3] for ln in lanes)
    sc, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
    assert sim.sim_ps_sign_scalars(mode, sz(n), sz(nY), sz(length), x48, y48 if nY else None, msgs, t32, sc, ok) == 0
    for j, (x, y, t, msg) in enumerate(lanes):
        m = scalars_of(orc, mode, msg)
        good = x < R and all(v < R for v in y[:len(m)])
        assert ok.raw[j] == (1 if good else 0), (j, hex(x))
        got_t = int.from_bytes(sc.raw[64 * j:64 * j + 32], "big")
        got_te = int.from_bytes(sc.raw[64 * j + 32:64 * j + 64], "big")
        if good:
            e = (x + sum(yi * mi for yi, mi in zip(y, m))) % R
            assert (got_t, got_te) == (t % R, t * e % R), (j, mode, length)
        else:
            assert (got_t, got_te) == (0, 0)


@pytest.mark.parametrize("mode,nY,lens", [(HASH, 1, HASH_LENS), (ENCODE, 3, ENCODE_LENS)])
def test_sign_scalars_prng(sim, oracle_port, mode, nY, lens):
    for length in lens:
        lanes = [(prng(7600, j) % R, [prng(7601 + i, j) % R for i in range(nY)], prng(7610, j, 32), msg_bytes(7620 + mode, 100 * length + j, length))
                 for j in range(6)]
        run_sign(sim, oracle_port, mode, nY, length, lanes)


@pytest.mark.parametrize("mode,nY,length", [(HASH, 1, 73), (ENCODE, 3, 93), (ENCODE, 3, 32)])
def test_sign_scalars_corners(sim, oracle_port, mode, nY, length):
    """0, 1, r - 1, r, 2^256 - 1 in every position of x, y_i and t (r and 2^256 - 1 in a key position fail parse<Zp> when the position is in
    use); the 48-byte fields also take 2^384 - 1; one lane has e = 0"""
    lanes = []
    msg = msg_bytes(7700 + mode, length, length)
    base = lambda j: [prng(7701, j) % R, [prng(7702 + i, j) % R for i in range(nY)], prng(7710, j, 32), msg]
    for pos in range(nY + 2):
        for v in CORNERS + ((1 << 384) - 1,):
            ln = base(len(lanes))
            if pos == 0:
                ln[0] = v
            elif pos <= nY:
                ln[1][pos - 1] = v
            elif v < (1 << 256):
                ln[2] = v
            else:
                continue
            lanes.append(tuple(ln))
    for v in CORNERS:                                        # the same corner everywhere
        lanes.append((v, [v] * nY, v, msg))
    m = scalars_of(oracle_port, mode, msg)
    y = [prng(7720 + i, 0) % R for i in range(nY)]
    x0 = -sum(yi * mi for yi, mi in zip(y, m)) % R           # e = 0
    lanes.append((x0, y, prng(7730, 0, 32), msg))
    run_sign(sim, oracle_port, mode, nY, length, lanes)
    n = len(lanes)
    sc, ok = ctypes.create_string_buffer(64), ctypes.create_string_buffer(1)
    assert sim.sim_ps_sign_scalars(mode, sz(1), sz(nY), sz(length), x0.to_bytes(48, "big"), b"".join(v.to_bytes(48, "big") for v in y), msg,
                                   lanes[-1][2].to_bytes(32, "big"), sc, ok) == 0
    assert ok.raw == b"\x01" and sc.raw[32:] == bytes(32) and sc.raw[:32] != bytes(32) and n > 20


def test_unused_y_is_not_checked(sim, oracle_port):
    """ENCODE mode, nY = 3, a 31-byte message: one unit, so y_2 and y_3 take no part — not even in the range check"""
    msg = msg_bytes(7800, 0, 31)
    run_sign(sim, oracle_port, ENCODE, 3, 31, [(5, [7, R, (1 << 384) - 1], 9, msg), (5, [R, 1, 1], 9, msg)])
