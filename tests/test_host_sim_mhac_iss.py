"""CPU tests of crypto12381_amd/csrc/mhac_iss.hpp compiled for the host with the bounds checker (tests/host_sim/mhac_iss.cpp, C12381_CHECK_BOUNDS),
against Python: polynomial for t = 1 (no coefficients), t = 8, x = 64 (the largest power, 64^7 = 2^42), coefficients 0 and r - 1 and values at and
above r; lambda for S in order, permuted and at the ends (0 and nparties - 1 = 63), lambda = 1 for t = 1, sum lambda = 1, and the argument errors of
S; the base lists and the rnd offsets for every shape the GPU tests use.  And tests/host_sim/mhac_iss_layouts.cpp, a stand-alone program built with
-fsanitize=address,undefined that carves the new slab layouts on mallocs of exactly their size."""
import ctypes
import os
import subprocess

import pytest

import mhac_bbs_cases as mh
import mhac_iss_cases as mi
from util import R, prng

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t
HPP = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]


def _stale(target, srcs):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in srcs)


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIM_DIR, "libsim_mhac_iss.so")
    src = os.path.join(SIM_DIR, "mhac_iss.cpp")
    if _stale(so, [src] + HPP):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def test_the_new_layouts_are_aligned_disjoint_and_inside_their_slabs():
    exe = os.path.join(SIM_DIR, "mhac_iss_layouts")
    src = os.path.join(SIM_DIR, "mhac_iss_layouts.cpp")
    if _stale(exe, [src] + HPP):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mhac iss layouts ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


def u32(v):
    return (ctypes.c_uint32 * max(len(v), 1))(*v)


def poly(sim, x, a0, coeffs):
    rnd = mi.rnd_bytes([a0] + list(coeffs))
    out = ctypes.create_string_buffer(48)
    assert sim.sim_mhac_iss_polynomial(ctypes.c_uint32(x), rnd, sz(0), sz(1), sz(len(coeffs)), out) == 0
    return int.from_bytes(out.raw, "big")


@pytest.mark.parametrize("t", [1, 2, 3, 5, 8])
def test_polynomial(sim, t):
    edge = [0, R - 1, 1, R, R + 5, (1 << 256) - 1]
    for case in range(8):
        a0 = edge[case % len(edge)] if case < 6 else prng(5000 + t, case) % (1 << 256)
        coeffs = [edge[(case + i) % len(edge)] if case % 2 == 0 else prng(5100 + t, 10 * case + i) % (1 << 256) for i in range(t - 1)]
        for x in (1, 2, 6, 63, 64):
            want = (a0 + sum(c * x ** (i + 1) for i, c in enumerate(coeffs))) % R
            assert poly(sim, x, a0, coeffs) == want == mh.polynomial(x, a0 % R, [c % R for c in coeffs]), (t, case, x)
    assert poly(sim, 64, 0, [R - 1] * (t - 1)) == (-(sum(64 ** (i + 1) for i in range(t - 1)))) % R      # every coefficient r - 1 at the largest x
    assert 64 ** 7 == 1 << 42 and float(64 ** 7) == 64.0 ** 7


def lam_of(sim, S, nparties):
    lam, st = ctypes.create_string_buffer(48 * 8), ctypes.create_string_buffer(8)
    if not sim.sim_mhac_iss_lambda(u32(S), sz(len(S)), sz(nparties), lam, st):
        return None
    assert list(st.raw[:len(S)]) == list(S) and st.raw[len(S):] == bytes(8 - len(S))
    vals = [int.from_bytes(lam.raw[48 * k:48 * k + 48], "big") for k in range(8)]
    assert vals[len(S):] == [0] * (8 - len(S))
    return vals[:len(S)]


@pytest.mark.parametrize("S,nparties", [((0, 1, 2), 6), ((0, 2, 5), 6), ((5, 0, 2), 6), ((2, 5, 0), 6), ((0,), 1), ((3,), 6), ((63,), 64), ((0, 63), 64), ((63, 0), 64),
                                        (tuple(range(8)), 8), ((7, 6, 5, 4, 3, 2, 1, 0), 8), ((0, 9, 18, 27, 36, 45, 54, 63), 64), (tuple(range(56, 64)), 64),
                                        ((1, 0, 4, 2, 3), 6), ((62, 63), 64)])
def test_lambda(sim, S, nparties):
    xs = [i + 1 for i in S]
    got = lam_of(sim, S, nparties)
    assert got == [mh.lagrange(xs, k) for k in range(len(S))] == [mi.lam_at(xs, k) for k in range(len(S))]
    assert sum(got) % R == 1
    if len(S) == 1:
        assert got == [1]
    # a permutation of S permutes lambda with it
    rev = lam_of(sim, S[::-1], nparties)
    assert rev == got[::-1]


def test_the_argument_errors_of_s_and_the_shape(sim):
    assert lam_of(sim, (0, 0), 6) is None and lam_of(sim, (0, 6), 6) is None and lam_of(sim, (1 << 31, 0), 6) is None
    assert lam_of(sim, (0, 1, 2), 2) is None and lam_of(sim, (0,), 65) is None and lam_of(sim, (64,), 64) is None
    assert lam_of(sim, tuple(range(9)), 16) is None and lam_of(sim, (), 4) is None
    assert not sim.sim_mhac_iss_lambda(None, sz(1), sz(4), ctypes.create_string_buffer(384), ctypes.create_string_buffer(8))
    ok = lambda t, n: bool(sim.sim_mhac_iss_shape_ok(sz(t), sz(n)))
    assert ok(1, 1) and ok(8, 8) and ok(8, 64) and ok(1, 64) and ok(3, 6)
    assert not ok(0, 4) and not ok(9, 16) and not ok(3, 2) and not ok(1, 0) and not ok(1, 65) and not ok(1 << 40, 1 << 40)


# (m, Prv, Rev) of the GPU tests, and a public_indexes order for iss
SHAPES = [(4, (0, 2), (1,)), (4, (), (1,)), (4, (0, 1, 2, 3), ()), (4, (2, 0), (1,)), (4, (0, 2), (1, 3)), (4, (0, 2), ()), (1, (), ()), (1, (0,), ()),
          (32, (0, 2), (1, 31, 17)), (5, (1, 3), (4, 0))]


@pytest.mark.parametrize("m,Prv,Rev", SHAPES)
def test_base_lists_and_rnd_offsets(sim, m, Prv, Rev):
    Pub, Hid, HidPub, RevPub, PubHid = mh.sets(m, Prv, Rev)
    for pub_idx in (Pub, Pub[::-1], Pub[1:] + Pub[:1]):
        bufs = [ctypes.create_string_buffer(32) for _ in range(4)]
        lens = (sz * 3)()
        assert sim.sim_mhac_iss_lists(sz(m), u32(Prv), sz(len(Prv)), u32(Rev), sz(len(Rev)), u32(pub_idx), sz(len(pub_idx)), *bufs, lens) == 1
        alist, plist, tlist, tat = (list(b.raw) for b in bufs)
        assert lens[0] == len(Prv) and alist == list(Prv) + [0] * (32 - len(Prv))
        assert lens[1] == len(pub_idx) and plist == list(pub_idx) + [0] * (32 - len(pub_idx))
        want_at = RevPub + PubHid
        assert lens[2] == len(Pub) and tat[:len(Pub)] == want_at and tlist[:len(Pub)] == [Pub[k] for k in want_at]
        assert tat[len(Pub):] == [0] * (32 - len(Pub)) and tlist[len(Pub):] == [0] * (32 - len(Pub))
    for t in (1, 2, 3, 5, 8):
        counts = (sz * 35)()
        sim.sim_mhac_iss_rnd(sz(m), sz(len(Prv)), sz(t), counts)
        assert counts[0] == mi.attr_rnd_count(m, Prv, t) and [counts[1 + ii] for ii in range(len(Prv))] == [m + ii * (t - 1) for ii in range(len(Prv))]
        assert counts[33] == t and counts[34] == 1


def test_pub_idx_errors(sim):
    def refused(m, pub_idx):
        bufs = [ctypes.create_string_buffer(32) for _ in range(4)]
        lens = (sz * 3)()
        assert sim.sim_mhac_iss_lists(sz(m), u32(()), sz(0), u32(()), sz(0), u32(pub_idx), sz(len(pub_idx)), *bufs, lens) == 1
        return lens[1] == (1 << 64) - 1
    assert refused(4, (0, 0)) and refused(4, (4,)) and refused(4, (0, 1, 2, 3, 0)) and refused(4, (1 << 31,))
    assert not refused(4, ()) and not refused(4, (3, 1)) and not refused(32, tuple(range(31, -1, -1)))
