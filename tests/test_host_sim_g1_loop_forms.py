"""CPU tests of the forms of the G1 window loop, under the bounds checker (tests/host_sim/g1_loop_forms.cpp, C12381_CHECK_BOUNDS).
- fp_sqr2 (fp.hpp: r = 2 a^2 / R from a square's columns): raw limbs EQUAL to fp_mul(a, fp_raw_dbl(a)) for random operands and for
  operands at the cap (limbs +-(2^28 + 8), signs mixed, the top limb at the largest value its value bound allows), the value against
  Python integers mod p; the checker stays silent at the cap and aborts the process where 28 LB^2 + 14 2^56 + 2^40 >= 2^63.
- g1j_dbl with G = 2Y^2 from fp_sqr2: raw limbs equal to the form it replaces (a copy kept in the harness) on the point list of
  test_host_sim_g1_dbl_fold.py with Z = 1, random Z, p - 1 and 0.
- g1j_madd (the mixed addition the doublings feed and are fed by) against plain affine integer arithmetic (g1_torsion.ec_add): random
  accumulators with Z = 1 and random Z, accumulator = +T and -T (Z3 = 0, and still 0 after a doubling and another addition), X1 = 0, the
  small-order points, and a chain of 125 doublings with two additions after every fifth."""
import ctypes
import math
import os
import subprocess
import sys

import pytest

from g1_torsion import ec_add, ec_mul, ec_neg, enc, generator
from test_host_sim_g1_dbl_fold import CAP, operand, points, value
from util import P, R, prng

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
SO = os.path.join(SIM_DIR, "libsim_g1_loop_forms.so")
sz = ctypes.c_size_t
NL, LB = 14, 28
RMONT = 1 << (NL * LB)


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(SIM_DIR, "g1_loop_forms.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-pthread", "-o", SO, src], check=True)
    return ctypes.CDLL(SO)


# ---------------------------------------------------------------- fp_sqr2 on raw limbs
def sqr2_cap_vectors(lb, declared=None):
    """operands with every low limb at +-lb (alternating, all positive, all negative, random signs) and the top limb, of either sign, the
    largest its value bound (2 and 4: a reduction output, a table record) allows"""
    vecs = []
    i = 0
    for pat in ("alt", "pos", "neg", "rnd"):
        for top_sign in (1, -1):
            for vb in (2, 4):
                for _ in range(4):                                  # four random sign patterns; the fixed ones repeat, which costs nothing
                    limbs, (l, v) = operand(9920 + i, lb, vb, top_sign, pat)
                    vecs.append((limbs, (float(declared) if declared is not None else l, v)))
                    i += 1
    return vecs


def sqr2_random_vectors(count):
    """reduction outputs as they come: limbs 0..12 in [0, 2^28), the value a random residue in [0, 2p)"""
    vecs = []
    for i in range(count):
        v = prng(9930, i) % (2 * P)
        vecs.append(([(v >> (LB * j)) & ((1 << LB) - 1) for j in range(NL - 1)] + [v >> (LB * (NL - 1))], (float(1 << LB), 2.0)))
    return vecs


def run_sqr2(lib, vecs):
    n = len(vecs)
    limbs = (ctypes.c_int32 * (NL * n))(*[l for v in vecs for l in v[0]])
    bnd = (ctypes.c_double * (2 * n))(*[x for v in vecs for x in v[1]])
    outs, outm = (ctypes.c_int32 * (NL * n))(), (ctypes.c_int32 * (NL * n))()
    ob = (ctypes.c_double * (4 * n))()
    assert lib.sim_lf_sqr2(sz(n), limbs, bnd, outs, outm, ob) == 0
    return ([list(outs[NL * i:NL * i + NL]) for i in range(n)], [list(outm[NL * i:NL * i + NL]) for i in range(n)],
            [tuple(ob[4 * i:4 * i + 4]) for i in range(n)])


@pytest.mark.parametrize("kind", ["random", "cap"])
def test_sqr2_raw_limbs_equal_the_general_product(sim, kind):
    vecs = sqr2_random_vectors(256) if kind == "random" else sqr2_cap_vectors(CAP)
    outs, outm, bounds = run_sqr2(sim, vecs)                  # the checker did not fire: the process is still here
    for (a, _), s, m, (slb, svb, mlb, mvb) in zip(vecs, outs, outm, bounds):
        assert s == m
        assert (slb, svb) == (mlb, mvb)                       # and it declares what fp_mul(a, 2a) declares
        va = value(a)
        assert (value(s) * RMONT - 2 * va * va) % P == 0
        assert all(0 <= l < (1 << LB) for l in s[:NL - 1])
        assert all(abs(l) <= slb for l in s) and abs(value(s)) <= svb * P
        assert svb <= 1.1 and slb == float(1 << 28)


# the smallest limb bound the column check refuses: 28 LB^2 + 14 2^56 + 2^40 >= 2^63 (+ 2: clear of the rounding of the checker's doubles)
LB_REFUSED = math.isqrt(((1 << 63) - 14 * (1 << 56) - (1 << 40)) // 28) + 2

FIRE_CODE = r"""
import sys
sys.path.insert(0, %r)
import ctypes
import test_host_sim_g1_loop_forms as t
lib = ctypes.CDLL(t.SO)
v = t.sqr2_cap_vectors(%d, %d)[:1]
print("calling", flush=True)
t.run_sqr2(lib, v)
print("returned", flush=True)
"""


def test_sqr2_checker_fires_past_the_column_bound(sim):
    """limbs at CAP declared at CAP: the call returns.  Declared at LB_REFUSED (2^29.05) and at 2^30, the limbs unchanged (the checker reads
    the declaration, and it must speak before a product is formed): the checker aborts the process."""
    assert 28 * LB_REFUSED ** 2 + 14 * (1 << 56) + (1 << 40) >= 1 << 63 > 28 * (LB_REFUSED - 4) ** 2 + 14 * (1 << 56) + (1 << 40)
    for declared, fires in ((CAP, False), (LB_REFUSED, True), (1 << 30, True)):
        code = FIRE_CODE % (HERE, CAP, declared)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
        assert "calling" in r.stdout
        if fires:
            assert r.returncode == -6 and "returned" not in r.stdout, (r.returncode, r.stderr[-500:])
            assert "C12381 bound violation: fp_sqr2" in r.stderr
        else:
            assert r.returncode == 0 and "returned" in r.stdout, r.stderr[-2000:]


# ---------------------------------------------------------------- the doubling: same limbs as the form it replaces
def test_doubling_raw_limbs_equal_the_parent_form(sim):
    pts = points()
    lanes = []
    for i, (name, pt) in enumerate(pts):
        lanes.append((name, pt, 1))
        for j in range(3):
            lanes.append((name, pt, prng(9702, 4 * i + j) % P or 1))
        lanes.append((name, pt, P - 1))
        lanes.append((name, pt, 0))
    n = len(lanes)
    P_ = b"".join(enc(pt) for _, pt, _ in lanes)
    Z_ = b"".join(z.to_bytes(48, "big") for _, _, z in lanes)
    new, old = (ctypes.c_int32 * (42 * n))(), (ctypes.c_int32 * (42 * n))()
    out = ctypes.create_string_buffer(96 * n)
    assert sim.sim_lf_dbl_cmp(sz(n), P_, Z_, new, old, out) == 0
    for i, (name, pt, z) in enumerate(lanes):
        assert list(new[42 * i:42 * i + 42]) == list(old[42 * i:42 * i + 42]), (name, z)
        assert out.raw[96 * i:96 * i + 96] == (bytes(96) if z == 0 else enc(ec_add(pt, pt))), (name, z)


# ---------------------------------------------------------------- the mixed addition against integers
def madd_lanes():
    """(name, acc, Z, q, q2): acc + q, then 2 (acc + q) + q2"""
    g = generator()
    rnd = lambda s, i: ec_mul(prng(s, i) % R or 1, g)
    lanes = []
    for i in range(24):                                            # random accumulators, Z = 1 and random Z
        a, q, q2 = rnd(9940, i), rnd(9941, i), rnd(9942, i)
        lanes.append(("rnd%d" % i, a, 1, q, q2))
        lanes.append(("rnd%d" % i, a, prng(9943, i) % P or 1, q, q2))
        lanes.append(("rnd%d" % i, a, P - 1, q, q2))
    for i in range(6):                                             # accumulator = +T and = -T
        t, q2 = rnd(9944, i), rnd(9945, i)
        for z in (1, prng(9946, i) % P or 1):
            lanes.append(("+T%d" % i, t, z, t, q2))
            lanes.append(("-T%d" % i, ec_neg(t), z, t, q2))
    tors = points()[41:]                                           # o3a, o3b, o11, g+t3, eig10177, eig859267
    assert [n for n, _ in tors][:2] == ["o3a", "o3b"] and tors[0][1][0] == 0
    for i, (name, t) in enumerate(tors):
        q, q2 = rnd(9947, i), rnd(9948, i)
        for z in (1, prng(9949, i) % P or 1):
            lanes.append((name + "+q", t, z, q, q2))               # X1 = 0 for the points of order 3
            lanes.append(("q+" + name, q, z, t, q2))
            lanes.append((name + "+" + name, t, z, t, q2))
            lanes.append((name + "-" + name, ec_neg(t), z, t, q2))
        for name2, t2 in tors:
            lanes.append((name + "+" + name2, t, prng(9950, i) % P or 1, t2, q2))
    return lanes


def test_madd_against_affine_integer_arithmetic(sim):
    lanes = madd_lanes()
    n = len(lanes)
    A_ = b"".join(enc(a) for _, a, _, _, _ in lanes)
    Z_ = b"".join(z.to_bytes(48, "big") for _, _, z, _, _ in lanes)
    Q_ = b"".join(enc(q) for _, _, _, q, _ in lanes)
    Q2_ = b"".join(enc(q2) for _, _, _, _, q2 in lanes)
    o1, o2 = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(96 * n)
    assert sim.sim_lf_madd(sz(n), A_, Z_, Q_, Q2_, o1, o2) == 0
    exceptional = regular = 0
    for i, (name, a, z, q, q2) in enumerate(lanes):
        got1, got2 = o1.raw[96 * i:96 * i + 96], o2.raw[96 * i:96 * i + 96]
        if a[0] == q[0]:                                           # acc = +-q: H = 0, Z3 = 0, and Z = 0 survives the doubling and the addition
            assert got1 == bytes(96) and got2 == bytes(96), (name, z)
            exceptional += 1
            continue
        s = ec_add(a, q)
        assert got1 == enc(s), (name, z)
        d = ec_add(s, s)
        # the second addition is exceptional in its own right where 2 (acc + q) = +-q2 or the doubling passed through infinity (order 2: none)
        assert got2 == (bytes(96) if d is None or d[0] == q2[0] else enc(ec_add(d, q2))), (name, z)
        regular += 1
    assert exceptional >= 2 * 12 + 2 * 12 and regular >= 72 + 24


def test_chain_of_125_doublings_two_additions_after_every_fifth(sim):
    """acc <- 32 acc + Q0 + Q1, 25 times, as the window loop runs them: the bounds checker follows the declared bounds through the loop"""
    g = generator()
    for i in range(4):
        p, q0, q1 = (ec_mul(prng(9960 + j, i) % R or 1, g) for j in range(3))
        out = ctypes.create_string_buffer(96)
        assert sim.sim_lf_chain(enc(p), enc(q0), enc(q1), 25, out) == 0
        s = p
        for _ in range(25):
            s = ec_add(ec_add(ec_mul(32, s), q0), q1)
        assert out.raw == enc(s), i
