"""CPU tests of the leaner forms of the single G1 product (g1.hpp), through the stand-alone program tests/host_sim/g1_lean.cpp built with
C12381_CHECK_BOUNDS (it aborts on a violated bound):
- g1j_add_eis over the nine-reduction g1j_madd_eis against g1j_add_signed over g1j_madd, lane by lane as Jacobian classes mod p (and
  against affine integer arithmetic where the lane is a point): random accumulators and table points, operands with every limb at the
  bound its argument may carry, acc = +-T (Z3 = 0 in both forms or in neither), an accumulator at infinity, the digit of class 0;
- the table with beta^2 x = -(x + beta x) against the table built with products, every field of every entry mod p;
- the whole product on the golden vectors, the small-order points, a point outside G1 under scalars below x^2, and the edge scalars:
  the bytes of the stored rows and of the oracle."""
import os
import struct
import subprocess

import pytest

from g1_eisenstein_seed import exceptional_seeded
from g1_torsion import ec_add, ec_mul, ec_neg, eigenpoint, enc, generator, point_of_order
from test_host_sim_g1_dbl_fold import CAP, operand, value
from util import P, R, golden, prng

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
NL, LB = 14, 28
RMONT = 1 << (NL * LB)
RINV = pow(RMONT, -1, P)
NONE = 15


@pytest.fixture(scope="module")
def prog():
    exe = os.path.join(SIM_DIR, "g1_lean")
    src = os.path.join(SIM_DIR, "g1_lean.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-pthread", "-o", exe, src], check=True)
    return exe


def _run(prog, mode, data):
    r = subprocess.run([prog, mode], input=data, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


# ---------------------------------------------------------------- the mixed addition
def mont(v):
    """v -> (limbs of v R mod p, canonical; declared bounds of a reduction output)"""
    m = v * RMONT % P
    return [(m >> (LB * j)) & ((1 << LB) - 1) for j in range(NL - 1)] + [m >> (LB * (NL - 1))], (float(1 << LB), 1.0)


def jac(pt, z):
    """the affine point on the Jacobian Z = z"""
    return mont(pt[0] * z * z % P), mont(pt[1] * z * z * z % P), mont(z)


def add_lanes():
    """(name, X1, Y1, Z1, x2, y2, acc_inf, code, expected affine point or None); an operand is (limbs, (lb, vb))"""
    g = generator()
    rnd = lambda s, i: ec_mul(prng(s, i) % R or 1, g)
    lanes = []
    for i in range(24):                                            # random accumulators and table points, either sign of y
        a, t = rnd(9970, i), rnd(9971, i)
        for j, z in enumerate((1, prng(9972, i) % P or 1, P - 1)):
            neg = (i + j) & 1
            lanes.append(("rnd%d" % i, *jac(a, z), mont(t[0]), mont(t[1]), 0, neg << 4 | i % 11, ec_add(a, ec_neg(t) if neg else t)))
    for i in range(6):                                             # acc = +T and -T under either sign: H = 0, Z3 = 0; or the doubling case
        t = rnd(9973, i)
        for z in (1, prng(9974, i) % P or 1):
            for a in (t, ec_neg(t)):
                for neg in (0, 1):
                    lanes.append(("T%d" % i, *jac(a, z), mont(t[0]), mont(t[1]), 0, neg << 4, "zero"))
    for i in range(6):                                             # an accumulator at infinity: its coordinates are placeholders
        a, t = rnd(9975, i), rnd(9976, i)
        for neg in (0, 1):
            lanes.append(("inf%d" % i, *jac(a, prng(9977, i) % P or 1), mont(t[0]), mont(t[1]), 1, neg << 4 | 3, ec_neg(t) if neg else t))
            lanes.append(("inf1_%d" % i, mont(1), mont(1), mont(1), mont(t[0]), mont(t[1]), 1, neg << 4 | 3, ec_neg(t) if neg else t))
    for i in range(6):                                             # the digit of class 0 reads entry 0 and keeps the accumulator
        a, t = rnd(9978, i), rnd(9979, i)
        z = prng(9980, i) % P or 1
        for neg in (0, 1):
            lanes.append(("none%d" % i, *jac(a, z), mont(t[0]), mont(t[1]), 0, neg << 4 | NONE, a))
            lanes.append(("none+inf%d" % i, *jac(a, z), mont(t[0]), mont(t[1]), 1, neg << 4 | NONE, "inf"))
            lanes.append(("none+T%d" % i, *jac(t, z), mont(t[0]), mont(t[1]), 0, neg << 4 | NONE, t))
    # every limb at the bound its argument may carry: X1, Y1 a reduction output or a table field (value bound 4), Z1 a reduction output, 1
    # or the seed's carried x2 - x1 of two table fields (8), x2, y2 table fields (4, y under either sign)
    i = 0
    for pat in ("alt", "pos", "neg", "rnd"):
        for signs in range(32):
            sg = [1 - 2 * ((signs >> b) & 1) for b in range(5)]
            ops = [operand(9990 + 5 * i + b, CAP, vb, sg[b], pat if b % 2 == 0 else ("rnd" if pat != "rnd" else "alt"))
                   for b, vb in enumerate((4, 4, 8, 4, 4))]
            lanes.append(("cap%d" % i, *ops, 0, (i & 1) << 4 | i % 11, None))
            i += 1
    return lanes


def _val(limbs):
    return value(limbs) * RINV % P


def test_add_eis_equals_add_signed_as_jacobian_classes(prog):
    lanes = add_lanes()
    n = len(lanes)
    data = struct.pack("<Q", n)
    for ln in lanes:
        for limbs, (lb, vb) in ln[1:6]:
            assert all(abs(l) <= lb for l in limbs) and abs(value(limbs)) <= vb * P
            data += struct.pack("<14i2d", *limbs, lb, vb)
        data += struct.pack("<2I", ln[6], ln[7])
    out = _run(prog, "add", data)                               # the checker did not fire: the program returned 0
    assert len(out) == 4 * 86 * n
    w = struct.unpack("<%di" % (86 * n), out)
    zero = regular = 0
    for i, ln in enumerate(lanes):
        o = w[86 * i:86 * i + 86]
        xn, yn, zn = (_val(o[NL * j:NL * j + NL]) for j in range(3))
        xo, yo, zo = (_val(o[43 + NL * j:43 + NL * j + NL]) for j in range(3))
        name, want = ln[0], ln[8]
        assert o[42] == o[85], name                            # acc_inf afterwards
        assert (zn == 0) == (zo == 0), name                    # Z3 = 0 exactly where the old form has it
        assert (xn * zo * zo - xo * zn * zn) % P == 0 and (yn * zo ** 3 - yo * zn ** 3) % P == 0, name
        for l in o[:42]:
            assert abs(l) <= CAP
        if want == "zero":
            assert zn == 0, name
            zero += 1
        elif want == "inf":
            assert o[42] == 1, name
        elif want is not None:
            assert o[42] == 0 and zn != 0, name
            zi = pow(zn, -1, P)
            assert (xn * zi * zi % P, yn * zi ** 3 % P) == want, name
            regular += 1
    assert zero == 6 * 2 * 2 * 2 and regular >= 72 + 24 + 24


# ---------------------------------------------------------------- the table
def test_table_fields_equal_the_product_built_table_mod_p(prog):
    g = generator()
    pts = [("gen", g)] + [("sub%d" % i, ec_mul(prng(9985, i) % R or 1, g)) for i in range(24)]
    pts += [("o3a", (0, 2)), ("o3b", (0, P - 2)), ("o11", point_of_order(11)), ("eig10177", eigenpoint(10177)[0])]
    pts += [("off%d" % i, bytes.fromhex(p)) for i, p in enumerate(golden("g1")["offsubgroup_points"][:4])]
    n = len(pts)
    data = struct.pack("<Q", n) + b"".join(pt if isinstance(pt, bytes) else enc(pt) for _, pt in pts)
    out = _run(prog, "table", data)
    assert len(out) == 4 * 1260 * n
    w = struct.unpack("<%di" % (1260 * n), out)
    for i, (name, pt) in enumerate(pts):
        new, old = w[1260 * i:1260 * i + 630], w[1260 * i + 630:1260 * i + 1260]
        for f in range(45):                                    # 11 entries x (y, x, beta x, beta^2 x), then Z_T
            a, b = new[NL * f:NL * f + NL], old[NL * f:NL * f + NL]
            assert (value(a) - value(b)) % P == 0, (name, f // 4, f % 4)
            assert all(abs(l) <= CAP for l in a) and abs(value(a)) <= 4 * P, (name, f // 4, f % 4)
            if f < 44 and f % 4 != 3:
                assert a == b, (name, f // 4, f % 4)           # the fields the change does not touch keep their limbs
        if name.startswith("o3"):                              # beta x = x on the points of order 3: the first step has h = 0, Z_T = 0
            assert value(new[NL * 44:NL * 45]) % P == 0


# ---------------------------------------------------------------- the whole product
def _b32(k):
    return (k % (1 << 256)).to_bytes(32, "big")


def test_whole_product_bytes(prog, oracle_port):
    g = golden("g1")
    lanes = []                                                 # (point, scalar, stored row or None)
    for key in ("", "offsubgroup_", "offsubgroup_small_"):
        for p, s, m in zip(g[key + "points"], g[key + "scalars"], g[key + "mul96"]):
            lanes.append((bytes.fromhex(p), int(s, 16), bytes.fromhex(m)))
    stored = len(lanes)
    edge = [0, 1, R - 1, R, (1 << 256) - 1]
    small = [int(s, 16) for s in g["offsubgroup_small_scalars"][:3]]           # scalars below x^2
    te = eigenpoint(10177)[0]
    pts = [enc(generator()), bytes.fromhex(g["points"][3]), bytes(96), enc((0, 2)), enc((0, P - 2)), enc(point_of_order(11)), enc(te),
           bytes.fromhex(g["offsubgroup_points"][1])]
    for pb in pts:
        lanes += [(pb, k, None) for k in edge + small + [prng(9986, i) % (1 << 256) for i in range(4)]]
    n = len(lanes)
    P_ = b"".join(ln[0] for ln in lanes)
    S_ = b"".join(_b32(ln[1]) for ln in lanes)
    out = _run(prog, "mul", struct.pack("<Q", n) + P_ + S_)
    assert len(out) == 97 * n
    exp = oracle_port.g1_mul(P_, S_, 96, 8)
    for i, (pb, k, row) in enumerate(lanes):
        got = out[97 * i:97 * i + 96]
        assert got == exp[96 * i:96 * i + 96], (i, hex(k))
        if row is not None:
            assert got == row, (i, hex(k))
    assert stored >= 8
    comp = [out[97 * i + 96] for i in range(n)]
    per = len(edge) + len(small) + 4
    o3 = range(stored + 3 * per, stored + 5 * per)             # the points of order 3 take the complete path where the predictor says so
    assert [comp[i] for i in o3] == [0 if exceptional_seeded(lanes[i][1], 3, 2) is None else 1 for i in o3]
    assert sum(comp[i] for i in o3) >= per
    assert sum(comp[stored:stored + 2 * per]) == 0             # subgroup points never do
