"""CPU tests of hash-to-G1 (h2c.hpp) and of the Zp / Fp helper entries on the degenerate inputs of h2c_zp_cases.py, under the bounds checker
(tests/host_sim/sim.cpp and tests/host_sim/h2c_zp.cpp, C12381_CHECK_BOUNDS): the zero SSWU denominator (u = 0 and u^2 = -1/11, for which
the reference returns a pair that is not on the curve), the u whose image on E' lies in the kernel of the 11-isogeny (infinity), the
sign boundary, unreduced inputs, every QR / sign class; cofactor clearing on points of small order and on the off-curve pair; the
21 x 21 edge grids of the Zp and Fp operations; the inner-product fold at its stage boundaries.
Expected values: the compiled reference for map_to_point and from_hash (the C port must agree on from_hash), Python integers for
everything else."""
import ctypes
import os
import subprocess

import pytest

import h2c_zp_cases as hz
from g1_torsion import dec, ec_mul, enc
from util import P

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t


def _build(so, src, opt):
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", opt, "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-pthread", "-o", so, src], check=True)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def sim():
    return _build(os.path.join(SIM_DIR, "libsim.so"), os.path.join(SIM_DIR, "sim.cpp"), "-O1")


@pytest.fixture(scope="module")
def unit():
    return _build(os.path.join(SIM_DIR, "libsim_h2c_zp.so"), os.path.join(SIM_DIR, "h2c_zp.cpp"), "-O2")


def _differs(got, want, w, labels):
    """the labels of the records that differ, as one string ("" when none does)"""
    assert len(got) == len(want) == w * len(labels)
    return "; ".join(str(labels[i]) for i in range(len(labels)) if got[w * i:w * i + w] != want[w * i:w * i + w])


def _map(unit, u48):
    n = len(u48) // 48
    out = ctypes.create_string_buffer(96 * n)
    assert unit.sim_h2c_map_to_point(sz(n), u48, out) == 0
    return out.raw


def _cofactor(unit, p96):
    n = len(p96) // 96
    out, bad = ctypes.create_string_buffer(96 * n), ctypes.c_int(7)
    assert unit.sim_h2c_clear_cofactor(sz(n), p96, out, ctypes.byref(bad)) == 0
    return out.raw, bad.value


def _from_hash(sim, d, fmt):
    n = len(d) // 64
    out = ctypes.create_string_buffer(fmt * n)
    assert sim.sim_g1_from_hash_batch(sz(n), d, out, fmt) == 0
    return out.raw


# ---------------------------------------------------------------- map_to_point
def test_map_to_point_on_every_branch(unit, oracle_ref):
    cases = hz.map_cases()
    labels = [(name, tag) for name, _, tag in cases]
    u48 = hz.map_bytes()
    want = oracle_ref.g1_map_to_point(u48)
    got = _map(unit, u48)
    assert _differs(got, want, 96, labels) == ""
    # what the reference does on the degenerate inputs, and the cases module's own arithmetic on all of them
    for i, (name, u, tag) in enumerate(cases):
        rec = want[96 * i:96 * i + 96]
        assert rec == enc(hz.map_to_point(u)), name
        if tag == "zero-den":
            assert rec == enc(hz.ZERO_DEN_PAIR) and not hz.on_curve(dec(rec)), name
        elif tag == "kernel":
            assert rec == bytes(96), name
        else:
            a = dec(got[96 * i:96 * i + 96])
            assert a is not None and (a[1] * a[1] - a[0] ** 3 - 4) % P == 0, name


def test_map_to_point_lanes_do_not_depend_on_their_batch(unit, oracle_ref):
    """the finish shares one inversion among the lanes of a batch: every case alone, and the batch reversed"""
    u48 = hz.map_bytes()
    want = oracle_ref.g1_map_to_point(u48)
    n = len(u48) // 48
    alone = b"".join(_map(unit, u48[48 * i:48 * i + 48]) for i in range(n))
    assert alone == want
    rev = b"".join(u48[48 * i:48 * i + 48] for i in reversed(range(n)))
    assert _map(unit, rev) == b"".join(want[96 * i:96 * i + 96] for i in reversed(range(n)))


# ---------------------------------------------------------------- from_hash
def test_from_hash_on_every_branch(sim, unit, oracle_ref, oracle_port):
    cases = hz.hash_cases()
    labels = [(name, tag) for name, _, tag in cases]
    d = hz.hash_bytes()
    for fmt in (96, 49):
        want = oracle_ref.g1_from_hash(d, fmt)
        assert want == oracle_port.g1_from_hash(d, fmt), fmt
        got = _from_hash(sim, d, fmt)
        assert _differs(got, want, fmt, labels) == "", fmt
        for i, (name, _, tag) in enumerate(cases):                      # degenerate digests hash to infinity
            assert (want[fmt * i:fmt * i + fmt] == bytes(fmt)) == (tag in ("zero-den", "kernel")), (name, fmt)
    # the plain multiple of the map's image, on Python integers
    want = oracle_ref.g1_from_hash(d, 96)
    for i, (name, dg, tag) in enumerate(cases):
        if tag not in ("zero-den", "kernel"):
            assert want[96 * i:96 * i + 96] == enc(ec_mul(hz.COFACTOR, hz.map_to_point(dg))), name


def test_clear_cofactor_of_map_to_point_is_from_hash(sim, unit, oracle_ref):
    """degenerate u included: the off-curve pair of a zero denominator is reported as a bad point by the cofactor entry, while from_hash,
    which feeds it to the same doubling chain unchecked, reaches infinity as the reference does"""
    cases = hz.map_cases()
    u48 = hz.map_bytes()
    d = b"".join(bytes(16) + u48[48 * i:48 * i + 48] for i in range(len(cases)))
    want = oracle_ref.g1_from_hash(d, 96)
    assert _from_hash(sim, d, 96) == want
    img = _map(unit, u48)
    got, bad = _cofactor(unit, img)
    assert bad == 1
    for i, (name, _, tag) in enumerate(cases):
        if tag == "zero-den":
            assert got[96 * i:96 * i + 96] == b"\xff" * 96 and want[96 * i:96 * i + 96] == bytes(96), name
        else:
            assert got[96 * i:96 * i + 96] == want[96 * i:96 * i + 96], name
    ok = [i for i, c in enumerate(cases) if c[2] != "zero-den"]
    got, bad = _cofactor(unit, b"".join(img[96 * i:96 * i + 96] for i in ok))
    assert bad == 0 and got == b"".join(want[96 * i:96 * i + 96] for i in ok)


# ---------------------------------------------------------------- cofactor clearing
def test_clear_cofactor_on_small_order_points(unit):
    cases = hz.cofactor_cases()
    labels = [c[0] for c in cases]
    assert sum(1 for c in cases if c[2] == hz.OFF_CURVE) == 1
    got, bad = _cofactor(unit, b"".join(c[1] for c in cases))
    assert bad == 1
    want = b"".join(b"\xff" * 96 if c[2] == hz.OFF_CURVE else c[2] for c in cases)
    assert _differs(got, want, 96, labels) == ""
    on = [c for c in cases if c[2] != hz.OFF_CURVE]
    got, bad = _cofactor(unit, b"".join(c[1] for c in on))
    assert bad == 0 and got == b"".join(c[2] for c in on)
    # 3, 11 and 10177 divide 1 - x: the small-order points go to infinity through the doubling chain, nothing else does
    small = ("infinity", "(0, 2)", "(0, -2)", "order 11", "order 11'", "o11 + o11'", "order 10177")
    assert all((c[2] == bytes(96)) == (c[0] in small) for c in on) and sum(c[0] in small for c in on) == len(small)


# ---------------------------------------------------------------- Zp
@pytest.mark.parametrize("op", range(5))
def test_zp_op_on_the_edge_grid(sim, op):
    a, b, pairs = hz.zp_grid()
    n = len(pairs)
    assert n == 441
    out = ctypes.create_string_buffer(32 * n)
    assert sim.sim_zp_op_batch(op, sz(n), a, b if op <= 2 else None, out) == 0
    assert _differs(out.raw, hz.zp_expected(hz.ZP_OPS[op], pairs), 32, [(hex(x), hex(y)) for x, y in pairs]) == ""


def test_zp_from_hash_on_edge_digests(sim):
    d = hz.zp_digest_bytes()
    n = len(d) // 64
    out = ctypes.create_string_buffer(32 * n)
    assert sim.sim_zp_from_hash_batch(sz(n), d, out) == 0
    assert _differs(out.raw, hz.zp_digest_expected(), 32, [hex(x) for x in hz.ZP_DIGESTS]) == ""


@pytest.mark.parametrize("n", hz.FOLD_SIZES)
def test_zp_inner_product_at_the_stage_boundaries(unit, n):
    a, b, dot, total = hz.fold_case(n)
    out, stages = ctypes.create_string_buffer(32), ctypes.c_int(0)
    assert unit.sim_zp_inner_product(sz(n), a, b, out, ctypes.byref(stages)) == 0
    assert out.raw == dot and stages.value == hz.fold_stages(n)
    assert unit.sim_zp_inner_product(sz(n), a, None, out, ctypes.byref(stages)) == 0
    assert out.raw == total and stages.value == hz.fold_stages(n)


# ---------------------------------------------------------------- Fp
@pytest.mark.parametrize("op", range(6))
def test_fp_op_on_the_edge_grid(sim, op):
    a, b, pairs = hz.fp_grid()
    n = len(pairs)
    assert n == 441
    out = ctypes.create_string_buffer(48 * n)
    assert sim.sim_fp_op_batch(op, sz(n), a, b if op <= 2 else None, out) == 0
    assert _differs(out.raw, hz.fp_expected(hz.FP_OPS[op], pairs), 48, [(hex(x), hex(y)) for x, y in pairs]) == ""
