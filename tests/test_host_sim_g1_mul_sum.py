"""CPU tests of the per-lane sum of k G1 products under one doubling chain (g1.hpp g1_scalar_mul_sum: k co-Z tables brought onto one
common Z, one Jacobian loop, complete fallback) under the bounds checker (tests/host_sim/g1_mul_sum.cpp, C12381_CHECK_BOUNDS: a bound
that fails aborts the process).  The pinned value of a lane is the oracle's `multiply` on every term followed by its `add`
(g1_mul_sum_cases.expected); the sim also reports the lanes that took the complete path."""
import ctypes
import os
import subprocess

import pytest

from g1_mul_sum_cases import INF, edge_lanes, expected, pack, related_lanes, seeded_lanes
from g1_torsion import X2, exceptional
from util import R

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t
KS = (1, 2, 3, 4)


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIM_DIR, "libsim_g1sum.so")
    src = os.path.join(SIM_DIR, "g1_mul_sum.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-pthread", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def run(sim, pts, sc, k):
    n = len(sc) // (32 * k)
    out = ctypes.create_string_buffer(max(96 * n, 1))
    comp = ctypes.create_string_buffer(max(n, 1))
    assert sim.sim_g1_mul_sum_batch(sz(n), ctypes.c_int(k), pts, sc, out, comp) == 0
    return out.raw[:96 * n], list(comp.raw[:n])


def differing(got, exp, n):
    return [i for i in range(n) if got[96 * i:96 * i + 96] != exp[96 * i:96 * i + 96]]


def trivial(term):
    return term[0] == INF or term[1] % R == 0


@pytest.mark.parametrize("k", KS)
def test_seeded_subgroup_lanes_never_fall_back(sim, oracle_port, k):
    """random points of G1 with random 256-bit scalars: the oracle's bytes, no bound assertion, and NO lane on the complete path"""
    n = 1500
    pts, sc = pack(seeded_lanes(oracle_port, k, n, 9700 + 10 * k), k)
    got, comp = run(sim, pts, sc, k)
    assert sum(comp) == 0
    assert differing(got, expected(oracle_port, pts, sc, k), n) == []


@pytest.mark.parametrize("k", KS)
def test_edge_scalars_and_special_points_in_every_term_position(sim, oracle_port, k):
    """edge scalars x {subgroup, infinity, order 3, order 11, G + T3, off-subgroup, eigenpoints} in every term position; a term on a point
    of order 3 or 11 with a scalar that is not 0 mod r has a degenerate table (Z_T = 0), so its lane must take the complete path; a
    subgroup or infinity term among random subgroup terms must not (alone, k = 1: exactly the lanes g1_torsion.exceptional predicts)"""
    lanes, tags = edge_lanes(oracle_port, k)
    pts, sc = pack(lanes, k)
    got, comp = run(sim, pts, sc, k)
    bad = differing(got, expected(oracle_port, pts, sc, k), len(lanes))
    assert bad == [], [tags[i] for i in bad[:8]]
    small = [i for i, (name, s, pos) in enumerate(tags) if name in ("o3", "o11") and s % R != 0]
    assert len(small) >= 100 and all(comp[i] for i in small)
    plain = [i for i, (name, s, pos) in enumerate(tags) if name in ("gen", "sub", "inf") and (k == 1 or i % 3 != 2)]
    want = [1 if k == 1 and tags[i][0] != "inf" and exceptional(tags[i][1], R, X2 % R) is not None else 0 for i in plain]
    assert [comp[i] for i in plain] == want, [tags[i] for i, w in zip(plain, want) if comp[i] != w][:8]


@pytest.mark.parametrize("k", KS[1:])
def test_related_lanes(sim, oracle_port, k):
    """Q = P, Q = -P, Q = 2P, Q = phi(P), all terms infinity, all scalars 0: the oracle's bytes; a lane whose result is infinity by
    cancellation is a complete-path lane, a lane whose terms are all trivial is not"""
    lanes, kinds = related_lanes(oracle_port, k)
    pts, sc = pack(lanes, k)
    got, comp = run(sim, pts, sc, k)
    exp = expected(oracle_port, pts, sc, k)
    bad = differing(got, exp, len(lanes))
    assert bad == [], [kinds[i] for i in bad[:8]]
    cancel = [i for i, kd in enumerate(kinds) if kd.startswith("cancel")]
    assert len(cancel) >= 20
    for i in cancel:
        assert exp[96 * i:96 * i + 96] == INF and not all(trivial(t) for t in lanes[i]) and comp[i] == 1, kinds[i]
    for i, kd in enumerate(kinds):
        if kd.startswith("all"):
            assert exp[96 * i:96 * i + 96] == INF and all(trivial(t) for t in lanes[i]) and comp[i] == 0, kd


def test_port_equals_reference_on_these_inputs_and_double_multiply_on_the_subgroup(oracle_port):
    """The port oracle the other cases compare with equals the compiled reference (`multiply` + `add`) on this suite's own edge and
    related inputs, and on subgroup lanes the pinned value equals the reference's fused g^x * h^y (double_multiply -> ECP_mul2), reached
    through sum_of_products with n = 2.  Where the compiled reference is not built, the same two statements are checked within the port."""
    from oracle.bindings import Oracle, have_reference
    ref = Oracle("reference") if have_reference() else oracle_port
    for k in (2, 3):
        for lanes in (edge_lanes(oracle_port, k)[0], related_lanes(oracle_port, k)[0]):
            pts, sc = pack(lanes, k)
            assert expected(ref, pts, sc, k, nthreads=1) == expected(oracle_port, pts, sc, k)
    n = 200
    lanes = seeded_lanes(oracle_port, 2, n, 9790)
    pts, sc = pack(lanes, 2)
    exp = expected(oracle_port, pts, sc, 2)
    for i in range(n):
        p2 = lanes[i][0][0] + lanes[i][1][0]
        s2 = (lanes[i][0][1] % (1 << 256)).to_bytes(32, "big") + (lanes[i][1][1] % (1 << 256)).to_bytes(32, "big")
        assert ref.g1_sum_of_products(p2, s2, 96) == exp[96 * i:96 * i + 96], i
