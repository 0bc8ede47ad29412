"""CPU tests of the device's Fp12 routines on ARBITRARY elements (gt_cases.py), under the bounds checker (tests/host_sim/sim.cpp,
C12381_CHECK_BOUNDS: every limb / value bound of fp.hpp is asserted on these sparse and non-canonical inputs too): the three-lane form of
pairing3.hpp (sim_gt3_op_batch, what gt3_op_kernel / gt3_is_unity_kernel / gt3_pow_queue_kernel run) and the one-lane form of fp12.hpp
(sim_gt_op_batch, the experiments build's gt_op_kernel).  Expected bytes: the Fp12 tower on Python integers for mul, conj, the final
exponentiation x^(3 (p^12 - 1) / r) and the is-unity verdict; the plain-C oracle for FP12_pow, which is a power only on the cyclotomic subgroup
(test_gt_cases.py holds the two references against each other).
  mul       all 144 products of basis elements (one coefficient-pair route of f12t_mul / f12t_combine each), sparse x sparse, x . 0 / 1 / -1,
            non-canonical operands on either side
  conj      every class
  is_unity  one, every single-coordinate miss of it, its p + 1 encodings and the misses hidden under them
  fexp      every class: inversion and Frobenius of elements of Fp, Fp2, Fp4 and of one-coefficient elements; zero
  pow       the route: exactly the members of the cyclotomic subgroup (of order r or not, + p encoded or not, zero, one) take the windows —
            a unitary element outside it, -1, a dense element and a Miller value take the reference's digit sequence"""
import ctypes
import os
import subprocess

import pytest

import gt_cases as gc

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t

FORMS = ("sim_gt3_op_batch", "sim_gt_op_batch")          # three lanes per element (pairing3.hpp) / one lane (fp12.hpp)
MUL, CONJ, POW, FEXP, UNITY = range(5)


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIM_DIR, "libsim.so")
    srcs = [os.path.join(SIM_DIR, "sim.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-pthread", "-o", so,
                        os.path.join(SIM_DIR, "sim.cpp")], check=True)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def el():
    return gc.elements()


def _op(sim, form, op, a, b=None):
    n = len(a) // 576
    out = ctypes.create_string_buffer(n if op == UNITY else 576 * n)
    assert getattr(sim, form)(op, sz(n), a, b, out) == 0
    return out.raw


@pytest.mark.parametrize("form", FORMS)
def test_sim_gt_mul_by_coefficient_route_and_on_sparse_operands(sim, form):
    pairs = gc.mul_pairs()
    labels = [p[0] for p in pairs]
    got = _op(sim, form, MUL, b"".join(p[1] for p in pairs), b"".join(p[2] for p in pairs))
    assert gc.differs(got, gc.mul_expected(pairs), 576, labels) == ""


@pytest.mark.parametrize("form", FORMS)
def test_sim_gt_conj_on_every_class(sim, el, form):
    labels = gc.all_labels()
    assert gc.differs(_op(sim, form, CONJ, b"".join(el[l] for l in labels)), gc.conj_expected(labels), 576, labels) == ""


@pytest.mark.parametrize("form", FORMS)
def test_sim_gt_is_unity_near_one(sim, form):
    items = gc.near_one()
    got = _op(sim, form, UNITY, b"".join(b for _, b in items))
    assert gc.differs(got, gc.unity_expected(items), 1, [l for l, _ in items]) == ""


@pytest.mark.parametrize("form", FORMS)
def test_sim_gt_fexp_on_every_class(sim, oracle_port, el, form):
    labels = gc.all_labels()
    tower = gc.fexp_tower()
    want = b"".join(tower[l] if l in tower else oracle_port.fexp(el[l]) for l in labels)       # zero: the oracle's bytes
    assert gc.differs(_op(sim, form, FEXP, b"".join(el[l] for l in labels)), want, 576, labels) == ""


def test_sim_gt_pow_route_is_membership_of_the_cyclotomic_subgroup(sim, oracle_port):
    """the kernel's choice (route 0) and the same choice in the work-queue kernel's five pieces (route 2): the oracle's bytes for every
    element, and the windows taken by exactly the members — counted per class, so a membership test degraded to "unitary" shows as
    unitary / minus_one in the windows (and in their bytes)"""
    try:
        labels, a, e = gc.pow_cases()
        want = oracle_port.gt_op("pow", a, e)
        ne = len(gc.POW_EXPS)
        for route in (0, 2):
            sim.sim_gt3_pow_route(route)
            took, bad = {}, []
            for k, l in enumerate(gc.POW_LABELS):
                got = _op(sim, "sim_gt3_op_batch", POW, a[576 * ne * k:576 * ne * (k + 1)], e[32 * ne * k:32 * ne * (k + 1)])
                took[l] = sim.sim_gt3_pow_route(route)
                bad.append(gc.differs(got, want[576 * ne * k:576 * ne * (k + 1)], 576, labels[ne * k:ne * (k + 1)]))
            assert "".join(bad) == "", (route, bad)
            assert took == {l: ne if l in gc.WINDOWED else 0 for l in gc.POW_LABELS}, route
    finally:
        sim.sim_gt3_pow_route(0)


def test_sim_gt_pow_membership_test_on_sparse_and_subfield_elements(sim, oracle_port, el):
    """f12t_is_cyclotomic (four Frobenius maps and a product) on elements of Fp, Fp2, Fp4, one-coefficient elements and basis elements: the
    verdict the tower gives (none is a member), the oracle's bytes"""
    labels, a, e = gc.pow_cases(gc.POW_SPARSE_EXPS, gc.POW_SPARSE_LABELS)
    members = sum(1 for l in gc.POW_SPARSE_LABELS if gc.is_cyclotomic(gc.dec(el[l])))
    assert members == 0
    sim.sim_gt3_pow_route(0)
    assert gc.differs(_op(sim, "sim_gt3_op_batch", POW, a, e), oracle_port.gt_op("pow", a, e), 576, labels) == ""
    assert sim.sim_gt3_pow_route(0) == members * len(gc.POW_SPARSE_EXPS)
    assert gc.differs(_op(sim, "sim_gt_op_batch", POW, a, e), oracle_port.gt_op("pow", a, e), 576, labels) == ""


def test_sim_gt_pow_one_lane(sim, oracle_port):
    """fp12_pow_generic, the one-lane kernel's power: the reference's digit sequence on every element"""
    labels, a, e = gc.pow_cases()
    assert gc.differs(_op(sim, "sim_gt_op_batch", POW, a, e), oracle_port.gt_op("pow", a, e), 576, labels) == ""
