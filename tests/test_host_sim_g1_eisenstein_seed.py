"""CPU tests of the seed of g1_scalar_mul_eis (g1.hpp: the accumulator starts from the top two digits, 42 windows follow) through the
stand-alone program tests/host_sim/g1_eisenstein_seed.cpp built with C12381_CHECK_BOUNDS: the program aborts
on a violated bound and on a pair of top digits the seed does not know.  Every one of the sixteen top values on each kind of point the
suite has, byte for byte against the oracle, the complete-path lanes against the predictor of the seeded schedule."""
import os
import struct
import subprocess

import pytest

from g1_eisenstein import DIGITS, code, recode, split
from g1_eisenstein_seed import SUMS, exact_digit, exceptional_seeded, occupied_scalars, one_scalar_per_top_value, top_value
from g1_torsion import X2, ec_mul, eigenpoint, enc, generator, point_of_order
from util import P, R, golden

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")


@pytest.fixture(scope="module")
def prog():
    exe = os.path.join(SIM_DIR, "g1_eisenstein_seed")
    src = os.path.join(SIM_DIR, "g1_eisenstein_seed.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-pthread", "-o", exe, src], check=True)
    return exe


def test_codes_of_the_seed_agree_with_python(prog):
    r = subprocess.run([prog, "codes"], capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr[-3000:]
    want = [code(*exact_digit(z)) for z in ((1, 0), (0, 1), (-5, 2), (3, -5), (2, 2), (2, 3))]
    assert [int(t, 16) for t in r.stdout.split()] == want
    assert [(2, 2), (2, 3)] == sorted(s for s, _, _ in SUMS.values())


def test_every_top_value_on_every_kind_of_point(prog, oracle_port):
    """the sixteen top values (one scalar each, then ten scalars of either value that occupies position 43) on the generator, a second
    subgroup point, an off-subgroup golden point, infinity, the two points of order 3, a point of order 11 and the eigenpoint of order 10177"""
    g = golden("g1")
    tops = one_scalar_per_top_value()
    ks = [tops[t] for t in sorted(tops)] + occupied_scalars(10)
    assert sum(1 for k in ks if len(recode(*split(k))) == DIGITS) >= 20 and {top_value(k) for k in ks if top_value(k) in SUMS} == set(SUMS)
    te, lam = eigenpoint(10177)
    pts = [(enc(generator()), (R, X2 % R)), (bytes.fromhex(g["points"][3]), (R, X2 % R)), (bytes.fromhex(g["offsubgroup_points"][1]), "off"),
           (bytes(96), "inf"), (enc((0, 2)), (3, 2)), (enc((0, P - 2)), (3, 2)), (enc(point_of_order(11)), (11, None)), (enc(te), (10177, lam))]
    lanes = [(pb, k, kind) for pb, kind in pts for k in ks]
    n = len(lanes)
    P_ = b"".join(ln[0] for ln in lanes)
    S_ = b"".join(ln[1].to_bytes(32, "big") for ln in lanes)
    r = subprocess.run([prog, "mul"], input=struct.pack("<Q", n) + P_ + S_, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout
    assert len(out) == 97 * n
    exp = oracle_port.g1_mul(P_, S_, 96, 8)
    bad = [i for i in range(n) if out[97 * i:97 * i + 96] != exp[96 * i:96 * i + 96]]
    assert bad == [], [(i, lanes[i][2], hex(lanes[i][1])) for i in bad[:8]]
    for i, (pb, k, kind) in enumerate(lanes):
        comp = out[97 * i + 96]
        if kind == "inf":
            want = 0
        elif kind == "off":                                    # a point whose order is not known here: bytes only
            want = comp
        else:
            want = 0 if exceptional_seeded(k, *kind) is None else 1
        assert comp == want, (i, kind, hex(k))
    comps = [out[97 * i + 96] for i in range(n)]
    assert sum(comps[4 * len(ks):6 * len(ks)]) >= 2 * (len(ks) - 2) and sum(comps[:2 * len(ks)]) == 0
    assert 0 < sum(comps[6 * len(ks):7 * len(ks)]) < len(ks)   # order 11: some lanes meet acc = +-T in the loop, not all


def test_generator_against_plain_integers(prog):
    """the sixteen top values on the generator against affine double-and-add on Python integers, a second reference"""
    g = generator()
    tops = one_scalar_per_top_value()
    ks = [tops[t] for t in sorted(tops)]
    P_ = enc(g) * len(ks)
    S_ = b"".join(k.to_bytes(32, "big") for k in ks)
    r = subprocess.run([prog, "mul"], input=struct.pack("<Q", len(ks)) + P_ + S_, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for i, k in enumerate(ks):
        assert r.stdout[97 * i:97 * i + 96] == enc(ec_mul(k % R, g)), hex(k)
