"""CPU tests of the per-lane sum over shared G2 bases (fixed_base.hpp g2_fixed_eval_sum: nb tables of multiples, one accumulator per lane
across all bases, the complete mixed addition g2_add_affine only) under the bounds checker (tests/host_sim/g2_fixed_sum.cpp, C12381_CHECK_BOUNDS: a bound that
fails aborts the process).  The pinned value of a lane is the oracle's `multiply` per column followed by its `add`, the addend last
(g2_fixed_sum_cases.expected).  The sim builds table entries lazily and keeps them per base, and the cases share one pool of bases."""
import ctypes
import os
import subprocess

import pytest

from g2_fixed_sum_cases import INF, addends, edge_case, edge_scalars, expected, related_cases, seeded, special_bases
from util import R

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t
NBS = (1, 2, 3, 5)


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIM_DIR, "libsim_g2fixedsum.so")
    src = os.path.join(SIM_DIR, "g2_fixed_sum.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-pthread", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    lib.sim_g2_fixed_sum_batch.argtypes = [sz, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    return lib


def run(sim, bases, sc, addend=None):
    nb = len(bases) // 192
    n = len(sc) // (32 * nb)
    out = ctypes.create_string_buffer(max(192 * n, 1))
    rc = sim.sim_g2_fixed_sum_batch(n, nb, bases, addend, sc, out)
    return rc, out.raw[:192 * n]


def differing(got, exp):
    return [i for i in range(len(exp) // 192) if got[192 * i:192 * i + 192] != exp[192 * i:192 * i + 192]]


def test_the_edge_scalars_the_cases_rely_on():
    ks = edge_scalars()
    assert all(k in ks for k in (0, R, R + 1, (1 << 256) - 1))


@pytest.mark.parametrize("nb", NBS)
def test_seeded_lanes(sim, oracle_port, nb):
    """random G2 bases with random 256-bit scalars: the oracle's bytes and no bound assertion"""
    bases, sc = seeded(oracle_port, nb, 300, 9750 + nb)
    rc, got = run(sim, bases, sc)
    assert rc == 0 and differing(got, expected(oracle_port, bases, sc)) == []


@pytest.mark.parametrize("nb", NBS)
def test_edge_scalars_in_every_base_position(sim, oracle_port, nb):
    """0, r, r + 1, 2^256 - 1, powers of |x| (zero GS digits), sparse windows: in every position"""
    for pos in range(nb):
        bases, sc = edge_case(oracle_port, nb, pos)
        rc, got = run(sim, bases, sc)
        assert rc == 0 and differing(got, expected(oracle_port, bases, sc)) == [], (nb, pos)


@pytest.mark.parametrize("nb", (2, 3))
def test_related_bases_and_cancellations(sim, oracle_port, nb):
    """H2 = H1, -H1, 2 H1, psi(H1): the complete addition needs no other path; lanes that cancel are the point at infinity"""
    for kind, bases, sc, cancel in related_cases(oracle_port, nb):
        rc, got = run(sim, bases, sc)
        exp = expected(oracle_port, bases, sc)
        assert len(cancel) >= 5 and all(exp[192 * j:192 * j + 192] == INF for j in cancel), kind      # the oracle: infinity there
        assert any(exp[192 * j:192 * j + 192] != INF for j in range(len(exp) // 192)), kind
        assert rc == 0 and differing(got, exp) == [], kind


@pytest.mark.parametrize("nb", (1, 3))
def test_addends(sim, oracle_port, nb):
    """absent, infinity, an element of G2, the negative of a lane's sum, a twist point of order 13 (outside G2)"""
    bases, sc = seeded(oracle_port, nb, 40, 9760 + nb)
    for name, addend in addends(oracle_port, bases, sc):
        rc, got = run(sim, bases, sc, addend)
        exp = expected(oracle_port, bases, sc, addend)
        assert rc == 0 and differing(got, exp) == [], name
        if name == "-sum0":
            assert exp[:192] == INF and exp[192:384] != INF


def test_bases_without_a_table_are_refused(sim, oracle_port):
    """the sim serves elements of G2 only, as the table kernel marks only those valid: anything else is the generic route's"""
    bases, sc = seeded(oracle_port, 3, 4, 9770)
    for name, pt in special_bases():
        for pos in range(3):
            assert run(sim, bases[:192 * pos] + pt + bases[192 * (pos + 1):], sc)[0] == -2, (name, pos)
