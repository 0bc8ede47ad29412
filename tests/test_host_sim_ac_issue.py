"""CPU tests of crypto12381_amd/csrc/ac_issue.hpp compiled for the host with the bounds checker (tests/host_sim/ac_issue.cpp, C12381_CHECK_BOUNDS),
against Python integers: the Horner sum ym and the power y^(nattr+1) for nattr = 1, 2, 4, 32 with attribute values 0, 1, r - 1 and y = 0, 1, r - 1; the
range check at r - 1, r and 2^384 - 1; rnd = 0, r, 2^256 - 1; the scalar columns of a lane at their base-major positions.  And
tests/host_sim/ac_issue_layouts.cpp, a stand-alone program built with -fsanitize=address,undefined that carves the new slab layouts on mallocs of
exactly their size."""
import ctypes
import os
import subprocess

import pytest

from util import R, prng

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t
HPP = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
TOP = (1 << 384) - 1
NATTRS = (1, 2, 4, 32)


def _stale(target, srcs):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in srcs)


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIM_DIR, "libsim_ac_issue.so")
    src = os.path.join(SIM_DIR, "ac_issue.cpp")
    if _stale(so, [src] + HPP):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def test_the_new_layouts_are_aligned_disjoint_and_inside_their_slabs():
    exe = os.path.join(SIM_DIR, "ac_issue_layouts")
    src = os.path.join(SIM_DIR, "ac_issue_layouts.cpp")
    if _stale(exe, [src] + HPP):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ac issue layouts ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


def b48(v):
    return v.to_bytes(48, "big")


def num(buf):
    return int.from_bytes(buf.raw, "big")


def horner(sim, y, a):
    ym, pw = ctypes.create_string_buffer(48), ctypes.create_string_buffer(48)
    sim.sim_ac_issue_horner(b48(y), b"".join(b48(v) for v in a), sz(len(a)), ym, pw)
    return num(ym), num(pw)


def attribute_sets(nattr):
    yield [0] * nattr
    yield [1] * nattr
    yield [R - 1] * nattr
    yield [(0, 1, R - 1)[i % 3] for i in range(nattr)]
    yield [(R - 1, 0, 1)[i % 3] for i in range(nattr)]
    yield [prng(8100 + nattr, i) % R for i in range(nattr)]


@pytest.mark.parametrize("nattr", NATTRS)
def test_horner_and_the_power_of_y(sim, nattr):
    for y in (0, 1, R - 1, 2, prng(8200, nattr) % R):
        for a in attribute_sets(nattr):
            want = sum(v * pow(y, i + 1, R) for i, v in enumerate(a)) % R
            assert horner(sim, y, a) == (want, pow(y, nattr + 1, R)), (nattr, y, a[:3])
    assert horner(sim, 1, [R - 1] * nattr)[0] == (-nattr) % R
    assert horner(sim, R - 1, [1] * nattr) == ((-(nattr % 2)) % R, pow(-1, nattr + 1, R))
    assert horner(sim, 0, [R - 1] * nattr) == (0, 0)


def test_the_range_check(sim):
    low = ctypes.create_string_buffer(32)
    for v, ok in ((0, 1), (1, 1), (R - 1, 1), (R, 0), (R + 1, 0), (1 << 256, 0), (TOP, 0), ((1 << 255) + (1 << 300), 0)):
        assert sim.sim_ac_issue_range(b48(v), low) == ok and num(low) == v % (1 << 256), hex(v)
    for sk, count, ok in ((b48(R - 1), 1, 1), (b48(R), 1, 0), (b48(5) + b48(R - 1), 2, 1), (b48(5) + b48(R), 2, 0), (b48(TOP) + b48(5), 2, 0),
                          (b48(5) + b48(R), 1, 1), (b48(0) + b48(0), 2, 1)):
        assert sim.sim_ac_issue_sk(sk, sz(count)) == ok


def test_the_random_scalar(sim):
    out = ctypes.create_string_buffer(48)
    for v in (0, 1, R - 1, R, R + 1, 2 * R, 2 * R + 7, (1 << 256) - 1):
        sim.sim_ac_issue_random(v.to_bytes(32, "big"), out)
        assert num(out) == v % R
    assert (1 << 256) < 3 * R


@pytest.mark.parametrize("nattr", NATTRS)
def test_the_lanes_write_their_columns_base_major(sim, nattr):
    n = 5
    x, y = prng(8300, 0) % R, prng(8300, 1) % R
    for j, (a, rnd, ok) in enumerate([([prng(8400, i) % R for i in range(nattr)], prng(8401, 0, 32), 1), ([R - 1] * nattr, 0, 1), ([0] * nattr, R, 1),
                                     ([1] * (nattr - 1) + [R], (1 << 256) - 1, 0), ([TOP] + [2] * (nattr - 1), 7, 0)]):
        attr, r32 = b"".join(b48(v) for v in a), rnd.to_bytes(32, "big")
        cols, w32, d32 = (ctypes.create_string_buffer(b"\x07" * k) for k in (32 * nattr * n, 32 * n, 32 * n))
        assert sim.sim_ac_issue_bbs_lane(b48(x), attr, sz(nattr), r32, sz(n), sz(j), cols, w32, d32) == ok
        at = lambda buf, k: int.from_bytes(buf.raw[32 * k:32 * k + 32], "big")
        assert [at(cols, i * n + j) for i in range(nattr)] == [v % (1 << 256) for v in a]
        assert at(w32, j) == rnd % R and at(d32, j) == (x + rnd) % R
        assert all(cols.raw[32 * k:32 * k + 32] == b"\x07" * 32 for k in range(nattr * n) if k % n != j)       # no other lane's slot is touched
        assert all(w32.raw[32 * k:32 * k + 32] == b"\x07" * 32 == d32.raw[32 * k:32 * k + 32] for k in range(n) if k != j)
        cols, al32, sc2 = (ctypes.create_string_buffer(b"\x07" * k) for k in (32 * nattr * n, 32 * n, 64 * n))
        assert sim.sim_ac_issue_rps_lane(b48(x) + b48(y), attr, sz(nattr), r32, sz(n), sz(j), cols, al32, sc2) == ok
        assert [at(cols, i * n + j) for i in range(nattr)] == [v % (1 << 256) for v in a] and at(al32, j) == rnd % R
        if ok:
            ym = sum(v * pow(y, i + 1, R) for i, v in enumerate(a)) % R
            assert at(sc2, j) == (x + ym) % R and at(sc2, n + j) == (rnd % R) * pow(y, nattr + 1, R) % R
        assert all(sc2.raw[32 * k:32 * k + 32] == b"\x07" * 32 for k in range(2 * n) if k % n != j)
