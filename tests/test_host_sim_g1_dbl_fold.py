"""CPU tests of the folded Jacobian doubling (g1.hpp g1j_dbl: G = 2Y^2, D/2 = X G, Y3 = E (D - X3) - 2G^2 in ONE reduction) and of its
primitive fp_mul_msqr2 (fp.hpp), under the bounds checker (tests/host_sim/g1_dbl_fold.cpp, C12381_CHECK_BOUNDS).
- The doubling against the complete g1_dbl and against plain affine integer arithmetic (g1_torsion.ec_add), for Z = 1, random Z and
  Z = 0, on subgroup points, X = 0 (the points (0, +-2)), and the small-order points of g1_torsion.py.
- A chain of 125 doublings with a mixed addition after every fifth, as the window loop runs them, against integers.
- The primitive on raw limbs AT its declared caps (a, c: 2^28 + 8; b: 3 (2^28 + 8); signs mixed; top limbs at the largest value their
  value bounds allow) against Python integers mod p; the checker stays silent there and aborts the process with b at 2^31."""
import ctypes
import os
import subprocess
import sys

import pytest

from g1_torsion import ec_add, ec_mul, eigenpoint, enc, generator, point_of_order
from util import P, R, prng

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
SO = os.path.join(SIM_DIR, "libsim_g1_dbl_fold.so")
sz = ctypes.c_size_t
NL, LB = 14, 28
RMONT = 1 << (NL * LB)
CAP = (1 << 28) + 8                        # limb bound of a reduction output with its carry slack (G1_REC_LB, soa_load_fp)


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(SIM_DIR, "g1_dbl_fold.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-pthread", "-o", SO, src], check=True)
    return ctypes.CDLL(SO)


def points():
    """(name, affine point): subgroup points, X = 0, order 11, G + (0, 2), eigenpoints of order 10177 and 859267"""
    g = generator()
    out = [("gen", g)] + [("sub%d" % i, ec_mul(prng(9701, i) % R, g)) for i in range(40)]
    out += [("o3a", (0, 2)), ("o3b", (0, P - 2)), ("o11", point_of_order(11)), ("g+t3", ec_add(g, (0, 2)))]
    out += [("eig%d" % q, eigenpoint(q)[0]) for q in (10177, 859267)]
    return out


def test_doubling_equals_the_complete_formulas_and_integers(sim):
    pts = points()
    lanes = []                                            # (name, point, Z)
    for i, (name, pt) in enumerate(pts):
        lanes.append((name, pt, 1))
        for j in range(3):
            lanes.append((name, pt, prng(9702, 4 * i + j) % P or 1))
        lanes.append((name, pt, P - 1))
        lanes.append((name, pt, 0))
    n = len(lanes)
    P_ = b"".join(enc(pt) for _, pt, _ in lanes)
    Z_ = b"".join(z.to_bytes(48, "big") for _, _, z in lanes)
    oj, oc = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(96 * n)
    assert sim.sim_dblfold_cmp(sz(n), P_, Z_, oj, oc) == 0
    seen_zero = 0
    for i, (name, pt, z) in enumerate(lanes):
        j, c = oj.raw[96 * i:96 * i + 96], oc.raw[96 * i:96 * i + 96]
        want = enc(ec_add(pt, pt))
        assert c == want, (name, "complete")
        if z == 0:                                        # Z = 0 stays Z = 0
            assert j == bytes(96), (name, "Z = 0")
            seen_zero += 1
        else:
            assert j == want, (name, z)
    assert seen_zero == len(pts)
    assert enc(ec_add((0, 2), (0, 2))) == enc((0, P - 2))  # X = 0: 2 (0, 2) = (0, -2), through E = 0, D = 0, Y3 = -2 G^2 alone


def test_chain_of_125_doublings_between_mixed_additions(sim):
    """acc <- 32 acc + Q, 25 times: every doubling's operands are reduction outputs, every fifth one's are g1j_madd outputs; the
    bounds checker runs over the declared bounds as the window loop produces them"""
    g = generator()
    for i in range(4):
        p, q = ec_mul(prng(9703, i) % R or 1, g), ec_mul(prng(9704, i) % R or 1, g)
        out = ctypes.create_string_buffer(96)
        assert sim.sim_dblfold_chain(enc(p), enc(q), 25, out) == 0
        s = p
        for _ in range(25):
            s = ec_add(ec_mul(32, s), q)
        assert out.raw == enc(s), i


# ---------------------------------------------------------------- the primitive on raw limbs
def value(limbs):
    return sum(l << (LB * i) for i, l in enumerate(limbs))


def operand(seed, lb, vb, top_sign, pattern):
    """13 low limbs at +-lb (signs by `pattern`: 'alt', 'pos', 'neg', 'rnd'), the top limb the largest of sign top_sign whose VALUE stays
    within vb p; -> (limbs, declared (lb, vb))"""
    sign = {"alt": lambda i: 1 - 2 * (i & 1), "pos": lambda i: 1, "neg": lambda i: -1, "rnd": lambda i: 1 - 2 * (prng(seed, i) & 1)}[pattern]
    low = [sign(i) * lb for i in range(NL - 1)]
    lv = value(low)
    top = (vb * P - top_sign * lv) >> (LB * (NL - 1))     # top_sign * (top 2^364) + lv within [-vb p, vb p]
    top = min(top, lb)
    limbs = low + [top_sign * top]
    assert abs(value(limbs)) <= vb * P and top > vb * 100000
    return limbs, (float(lb), float(vb))


def msqr2_vectors(b_lb, b_declared=None):
    """a, c at the cap of a reduction output, b at b_lb (declared as b_declared where that differs); value bounds of the doubling's
    operands with room: E = 3A (4), D - X3 (16), G (2)"""
    vecs = []
    pats = ("alt", "pos", "neg", "rnd")
    i = 0
    for pa in pats:
        for pb in pats:
            for pc in pats:
                for sa, sb, sc in ((1, 1, 1), (1, -1, 1), (-1, 1, -1), (-1, -1, -1)):
                    vecs.append((operand(9710 + i, CAP, 4, sa, pa), operand(9810 + i, b_lb, 16, sb, pb), operand(9910 + i, CAP, 2, sc, pc)))
                    i += 1
    if b_declared is not None:
        vecs = [(a, (b[0], (float(b_declared), b[1][1])), c) for a, b, c in vecs]
    return vecs


def run_msqr2(lib, vecs):
    n = len(vecs)
    limbs = (ctypes.c_int32 * (3 * NL * n))(*[l for v in vecs for o in v for l in o[0]])
    bnd = (ctypes.c_double * (6 * n))(*[x for v in vecs for o in v for x in o[1]])
    out = (ctypes.c_int32 * (NL * n))()
    ob = (ctypes.c_double * (2 * n))()
    assert lib.sim_dblfold_msqr2(sz(n), limbs, bnd, out, ob) == 0
    return [list(out[NL * i:NL * i + NL]) for i in range(n)], [(ob[2 * i], ob[2 * i + 1]) for i in range(n)]


def test_msqr2_raw_limbs_at_the_declared_caps(sim):
    vecs = msqr2_vectors(3 * CAP)
    assert len(vecs) == 256
    outs, bounds = run_msqr2(sim, vecs)                   # the checker did not fire: the process is still here
    for (a, b, c), o, (lb, vb) in zip(vecs, outs, bounds):
        va, vb_, vc = value(a[0]), value(b[0]), value(c[0])
        assert (value(o) * RMONT - (va * vb_ - 2 * vc * vc)) % P == 0
        assert all(0 <= l < (1 << LB) for l in o[:NL - 1])
        assert all(abs(l) <= lb for l in o) and abs(value(o)) <= vb * P
        assert vb <= 1.1 and lb == float(1 << 28)        # what the next product of the doubling chain relies on


FIRE_CODE = r"""
import sys
sys.path.insert(0, %r)
import ctypes
import test_host_sim_g1_dbl_fold as t
lib = ctypes.CDLL(t.SO)
v = t.msqr2_vectors(%d, %d)[:1]
print("calling", flush=True)
t.run_msqr2(lib, v)
print("returned", flush=True)
"""


def test_msqr2_checker_fires_with_b_at_2_31(sim):
    """the same call with b at 2^31 (limbs 2^31 - 1, declared 2^31): 14 (2^59 + 2 2^56 + 2^56) > 2^63, the checker aborts the process.
    The control run, the same child with b at its cap, returns."""
    for b_lb, b_declared, fires in ((3 * CAP, 3 * CAP, False), ((1 << 31) - 1, 1 << 31, True)):      # limbs 2^31 - 1 fit int32
        code = FIRE_CODE % (HERE, b_lb, b_declared)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
        assert "calling" in r.stdout
        if fires:
            assert r.returncode == -6 and "returned" not in r.stdout, (r.returncode, r.stderr[-500:])
            assert "C12381 bound violation: fp_mul_msqr2" in r.stderr
        else:
            assert r.returncode == 0 and "returned" in r.stdout, r.stderr[-2000:]
