"""CPU tests of the bucket product's arithmetic (msm.hpp: msm_prep_one, msm_bucket_one with the complete mixed addition g1_add_affine,
msm_wreduce_one, msm_horner, msm_small_term) on the constructed inputs of msm_cases.py, under the bounds checker (tests/host_sim/sim.cpp,
C12381_CHECK_BOUNDS: a bound that fails aborts the process): equal points and a point with its negative in one bucket, additions after
the accumulator became infinity, the two records of a term meeting those of another, chosen digits, edge scalars, long runs, the
small-scalar bucket with a sum at infinity, inside and outside G1.  The simulation sums every run in one piece: the cut into overflow
segments is the device's, and the GPU test's business (test_gpu_msm_cases.py).  Expected values: Python integers for subgroup points,
the oracle's chain of multiply() results where a point lies outside G1."""
import ctypes
import os
import subprocess

import pytest

import msm_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t

SMALL = [n for n in mc.NAMES if n[0] != "g"]                      # families (a) .. (f): at most 3000 terms
NARROW = [n for n in SMALL if mc.case(n).n <= 130]


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIM_DIR, "libsim.so")
    srcs = [os.path.join(SIM_DIR, "sim.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-pthread", "-o", so,
                        os.path.join(SIM_DIR, "sim.cpp")], check=True)
    return ctypes.CDLL(so)


def product(sim, pts, sc, fmt, c):
    out = ctypes.create_string_buffer(b"\x5a" * fmt, fmt)
    assert sim.sim_g1_msm_pippenger(sz(len(sc) // 32), pts, sc, out, fmt, c) == 0
    return out.raw


@pytest.mark.parametrize("name", SMALL)
def test_native_width(sim, oracle_port, name):
    """c = 8, both output formats"""
    c = mc.case(name)
    assert c.n <= 3000 and mc.window_bits(c.n) == 8
    pts, sc = c.pack()
    exp = mc.expected96(name, oracle_port)
    assert product(sim, pts, sc, 96, 0) == exp
    assert product(sim, pts, sc, 49, 0) == mc.enc49(exp)


@pytest.mark.parametrize("c", [4, 7])
@pytest.mark.parametrize("name", NARROW)
def test_forced_narrow_widths(sim, oracle_port, name, c):
    """c = 4 (32 windows) and c = 7 (19 windows, the top one of 2 bits: the mask of msm_digit past bit 128 and d < nb in msm_wreduce_one)"""
    pts, sc = mc.case(name).pack()
    assert product(sim, pts, sc, 96, c) == mc.expected96(name, oracle_port)


def test_sixteen_bit_windows_once(sim, oracle_port):
    """c = 16: (a), (c), (d), (f) as ONE product (a call at this width walks 2^19 buckets on the CPU)"""
    up, uk = mc.union_terms()
    u = mc.Case("g:union", up, uk)
    assert u.n >= 300 and not u.subgroup_only
    pts, sc = u.pack()
    assert product(sim, pts, sc, 96, 16) == oracle_port.g1_msm(pts, sc, 96, 8)
