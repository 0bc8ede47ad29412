"""The case lists of msm_cases.py against the header and the oracle, on the CPU: the Python restatement of msm_window_bits / msm_windows /
msm_run_cap equals the header's (sim_msm_params), the digits equal scalar_glv_split, every expected value derived from integers equals the
oracle's chain of multiply() results (so the integer model and the oracle pin each other), and the coverage report holds."""
import ctypes
import os
import subprocess

import pytest

import msm_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIM_DIR, "libsim.so")
    srcs = [os.path.join(SIM_DIR, "sim.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-pthread", "-o", so,
                        os.path.join(SIM_DIR, "sim.cpp")], check=True)
    return ctypes.CDLL(so)


@pytest.mark.parametrize("n", [1, 2, 120, 127, 128, 3000, 4095, 4096, 1 << 15])
def test_model_equals_the_header(sim, n):
    c, W, cap = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint32()
    assert sim.sim_msm_params(sz(n), ctypes.byref(c), ctypes.byref(W), ctypes.byref(cap)) == 0
    assert (c.value, W.value, cap.value) == mc.params(n)


def test_halves_equal_the_split_of_the_header(sim):
    """sc(k0, k1) and split() against scalar_glv_split on every scalar of the small cases"""
    ks = sorted({k for c in mc.small_cases() for k in c.scalars})
    assert len(ks) > 300
    for k in ks:
        k0, k1 = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 4)()
        sim.sim_glv_split(k.to_bytes(32, "big"), k0, k1)
        got = tuple(sum(int(v[i]) << (32 * i) for i in range(4)) for v in (k0, k1))
        assert got == mc.split(k), hex(k)


@pytest.mark.parametrize("name", [n for n in mc.NAMES if n[0] != "g" and mc.case(n).subgroup_only])
def test_integer_expected_equals_the_oracle(oracle_port, name):
    c = mc.case(name)
    pts, sc = c.pack()
    assert c.expected == oracle_port.g1_msm(pts, sc, 96, 8)
    assert mc.enc49(c.expected) == oracle_port.g1_compress(c.expected) == oracle_port.g1_msm(pts, sc, 49, 8)


def test_coverage_report():
    """the seams of the cut, as the model sees them; the table names the case that hits each"""
    print(mc.coverage_table())
    rows = mc.COVERAGE
    seam = {ln - cap for name, _, cap, sl, ln, ns in rows if name == "e:seams"}
    assert seam == {0, 1, 16, 17, 32}
    assert any(ns > 64 for *_, ns in rows)
    assert {f: len(mc.family(f)) > 0 for f in mc.FAMILIES} == dict.fromkeys(mc.FAMILIES, True)
    # the widths and paths of family (g); more small scalars than the early kernel takes at 2^15 terms
    assert [mc.case(n).path for n in mc.family("g")] == ["32-bit keys c=8", "32-bit keys c=16", "16-bit keys"]
    big = mc.case("g:n=2^15")
    assert sum(mc.split(k)[1] == 0 and p is not None for p, k in zip(big.points, big.scalars)) > mc.SMALL_EARLY_MAX
    assert all(not mc.case(n).subgroup_only for n in mc.family("g"))


def test_a_list_that_loses_a_seam_fails(monkeypatch):
    """the coverage assertions are live: without the run of cap + 1 entries, or with the long run shortened, they fail"""
    groups = [(cnt - 1, j) if j == 2 else ((cnt + 1, j) if j == 1 else (cnt, j)) for cnt, j in mc.E_GROUPS]
    monkeypatch.setattr(mc, "E_GROUPS", groups)
    mc.small_cases.cache_clear()
    try:
        with pytest.raises(AssertionError):
            mc._coverage()
    finally:
        monkeypatch.undo()
        mc.small_cases.cache_clear()
    assert mc._coverage() == mc.COVERAGE


def test_tiled_expected_equals_the_whole_chain(oracle_port):
    """family (g) computes its expected value from one tile's terms outside G1 and integers: at 4095 terms, the same as the oracle's
    chain over every term"""
    c = mc.case("g:n=4095")
    assert c.tiles >= 2 and c.tiles * c.tile_len >= 3 * c.n // 4 - c.tile_len
    assert mc.expected96(c.name, oracle_port) == oracle_port.g1_msm(*c.pack(), 96, 8)
