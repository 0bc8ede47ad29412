"""CPU tests of the device's pairing routines on structured G1 arguments (g1_pairing_args.py), under the bounds checker
(tests/host_sim, C12381_CHECK_BOUNDS): (0, +-2) of order 3, whose px = 0 makes l2 = 3 X^2 px vanish in every line of the running-point
loop and leaves only the pass-through term in the product against a normalised table; G + T3, small-order points, the extreme x, the
three points that share a y, infinity and P beside -P.  The 63-lane pattern goes through the one-lane and three-lane loops and pair_eq;
the column patterns for K = 1, 2, 3, 8 go through the table-driven loop behind a restatement of the prep kernel's mask word and negation,
on raw and on normalised tables.  A declared bound that holds only for a generic px aborts the process here; every expected value is the
oracle's (pinned to the compiled reference on these inputs by test_g1_pairing_args.py)."""
import ctypes
import os
import subprocess

import pytest

import g1_pairing_args as ga

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t
ONE = ga.ONE


def _build(so, src, opt):
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", opt, "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-pthread", "-o", so, src], check=True)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def sim():
    return _build(os.path.join(SIM_DIR, "libsim.so"), os.path.join(SIM_DIR, "sim.cpp"), "-O1")


@pytest.fixture(scope="module")
def fk():
    return _build(os.path.join(SIM_DIR, "libsim_fixedk.so"), os.path.join(SIM_DIR, "fixed_k.cpp"), "-O2")


@pytest.fixture(scope="module")
def lanes(oracle_port):
    """the 63-lane pattern: (G1 bytes, G2 bytes, labels, oracle Miller values, oracle pairings)"""
    assert ga.self_check()
    pat = ga.pattern()
    p1, q2 = ga.lane_bytes(pat)
    return p1, q2, ["%s,%s" % l for l in pat], oracle_port.miller(p1, q2), oracle_port.pair(p1, q2, 8)


@pytest.fixture(scope="module")
def mils(oracle_port):
    return ga.Millers(oracle_port)


@pytest.mark.parametrize("entry,ref", (("sim_pair3_batch", "pair"), ("sim_miller3_batch", "miller"), ("sim_miller_batch", "miller"),
                                       ("sim_pair_batch", "pair")))
def test_sim_running_point_loops_on_the_pattern(sim, lanes, entry, ref):
    """the three-lane loop (miller3_dbl_step_sel forms l2 = 3 X^2 px and l0 = -2 Y Z (1 + i) py against a selected coordinate) and the
    one-lane loop: Miller values and pairings of all 63 lanes, the zero element of the px = 0 lane against G2 infinity among them"""
    p1, q2, labels, mil, gt = lanes
    n = len(labels)
    out = ctypes.create_string_buffer(576 * n)
    assert getattr(sim, entry)(sz(n), p1, q2, out) == 0
    assert ga.differs(out.raw, mil if ref == "miller" else gt, 576, labels) == ""


def test_sim_pair_eq_on_the_pattern(sim, oracle_port, lanes):
    """e(a1, a2) == e(b1, b2) as the kernels test it, e(a1, a2) e(-b1, b2) == 1: the degenerate classes on the a1 side and on the negated
    b1 side (py = 2 and py = p - 2 through the negation), a = b identical, both G1 arguments at infinity.  The one-lane loop on all
    lanes, the three-lane joint loop on the degenerate group."""
    p1, q2, labels, _, _ = lanes
    n = len(labels)
    b1, b2 = ga.rot(p1, 96, 2 * ga.TRI + 2), ga.rot(q2, 192, 2 * ga.TRI - 4)          # the degenerate group meets groups 0 and 1
    zero = bytes(96) * 4
    a1, a2 = zero + p1 + p1, q2[:192 * 4] + q2 + q2
    c1, c2 = zero + b1 + p1, q2[192 * 4:192 * 8] + b2 + q2
    want = oracle_port.pair_eq(a1, a2, c1, c2, 8)
    # identical sides are equal — but for the lane whose value is the zero element: 0 * conj(0) is not 1, here and in the reference
    assert set(want[:4]) == {1} and 0 in want[4:4 + n] and [i for i in range(n) if want[4 + n + i] != 1] == [2 * ga.TRI + 17]
    tail = list(range(n - ga.TRI + 2, 4 + n)) + list(range(4 + n + 2 * ga.TRI, len(want)))      # 23 unequal lanes, then group 2 against itself
    for entry, sel in (("sim_pair_eq_batch", list(range(len(want)))), ("sim_pair3_eq_batch", tail)):
        pick = lambda buf, w: b"".join(buf[w * i:w * i + w] for i in sel)
        ok = ctypes.create_string_buffer(len(sel))
        assert getattr(sim, entry)(sz(len(sel)), pick(a1, 96), pick(a2, 192), pick(c1, 96), pick(c2, 192), ok) == 0
        assert ok.raw == bytes(want[i] for i in sel), (entry, [i for j, i in enumerate(sel) if ok.raw[j] != want[i]])


def _run(fk, K, g1s, g2s, neg_mask, raw, step=16):
    n = len(g1s) // (96 * K)
    out = ctypes.create_string_buffer(576 * n)
    mask = (ctypes.c_uint32 * n)()
    assert fk.sim_fixedk_prep_miller(sz(n), K, g1s, g2s, ctypes.c_uint32(neg_mask), raw, step, out, mask) == 0
    return out.raw, list(mask)


def _check(K, twin, got, want, raw, oracle):
    """got against the oracle's products: the Miller value itself for raw tables, its final exponentiation for normalised ones; the
    claimed ones exactly.  An off-curve column is a skipped one whose record is not zero: the value is the product of the others."""
    pats = ga.column_patterns(K)
    bad = []
    fe, fw = oracle.fexp(got), oracle.fexp(b"".join(want))
    for i, (label, _, claims) in enumerate(pats):
        g, e = got[576 * i:576 * i + 576], fe[576 * i:576 * i + 576]
        if raw:
            ok = g == want[i] and (g == ONE) == ("one" in claims)
        else:
            ok = e == fw[576 * i:576 * i + 576]
        if ok and ("gt_one" in claims or "one" in claims or (twin and "gt_one_twin" in claims)):
            ok = e == ONE
        if not ok:
            bad.append(label)
    return bad


@pytest.mark.parametrize("K", ga.KS)
def test_sim_fixedk_column_patterns(fk, oracle_port, mils, K):
    """every column pattern as one element of a K-way batch, columns 0 and 1 on one G2 point.  Raw tables, in the queue's task ranges of
    16 iterations: the product of the oracle's Miller values, exactly 1 where every column is skipped.  Normalised tables (a skipped
    column multiplies by s, 69 times): the oracle's GT product after the final exponentiation, exactly 1 for all-infinity, all-order-3
    and the cancelling pair.  The mask words are the prep kernel's; an off-curve column (bit 31, which makes the entry write 0xff) is skipped like infinity
    though its record is not zero:
    the value is, byte for byte, that of the same element with infinity in that column."""
    g1s = ga.column_bytes(K)
    g2s = b"".join(ga.g2_points()[q] for q in ga.column_g2(K, True))
    want = mils.product(K, True)
    pats = ga.column_patterns(K)
    n = len(pats)
    off = [i for i, p in enumerate(pats) if "off" in p[2]]
    # the same batch with infinity where the off-curve records stand: a skipped column must not look at its record
    as_inf = b"".join(bytes(96) if cols[c] == ga.OFF_CURVE else ga.enc(cols[c]) for c in range(K) for _, cols, _ in pats)
    for raw, step in ((1, 16), (0, 64)):
        got, mask = _run(fk, K, g1s, g2s, 0, raw, step)
        assert mask == ga.column_mask_words(K)
        assert _check(K, True, got, want, raw, oracle_port) == [], (K, raw)
        # ... in the Miller value itself: on a normalised table the final exponentiation hides an l2 that was left standing
        alt, amask = _run(fk, K, as_inf, g2s, 0, raw, step)
        assert alt == got and [m & 0x7fffffff for m in mask] == amask and [i for i in range(n) if mask[i] != amask[i]] == off, (K, raw)


@pytest.mark.parametrize("K", ga.KS)
def test_sim_fixedk_negated_columns(fk, oracle_port, mils, K):
    """the prep step's negation (py <- p - py on py = 2, py = p - 2, ordinary py, and on the skipped records): columns handed over
    negated, with their bit in neg_mask, give what the plain columns give — every column (normalised tables), and for K < 8 the even
    ones (raw tables)"""
    g2s = b"".join(ga.g2_points()[q] for q in ga.column_g2(K, True))
    want = mils.product(K, True)
    full = (1 << K) - 1
    for neg, raw in ((full, 0), (0x55 & full, 1))[:1 if K in (1, 8) else 2]:
        got, mask = _run(fk, K, ga.column_bytes(K, neg), g2s, neg, raw, 16)
        assert mask == ga.column_mask_words(K)
        assert _check(K, True, got, want, raw, oracle_port) == [], (K, hex(neg), raw)


def test_sim_fixed_g2_single_table_on_every_point(fk, oracle_port, mils):
    """K = 1, every point of the builder as the G1 argument: against an ordinary G2 point (normalised: the GT value; raw: the Miller value),
    against G2 infinity (the table stays raw either way; px = 0 gives the zero element) and the order-13 twist point"""
    names = list(ga.points())
    g1s = b"".join(ga.enc(k) for k in names)
    for q in ("q1", "inf2", "t13"):
        want = mils.get([(k, q) for k in names])
        qb = ga.g2_points()[q]
        got, mask = _run(fk, 1, g1s, qb, 0, 1, 16)
        assert ga.differs(got, want, 576, names) == "" and mask == [1 if k == "inf" else 0 for k in names], q
        got, _ = _run(fk, 1, g1s, qb, 0, 0, 16)
        assert ga.differs(oracle_port.fexp(got), oracle_port.fexp(want), 576, names) == "", q
        if q == "inf2":
            assert got == want and [k for i, k in enumerate(names) if want[576 * i:576 * i + 576] == bytes(576)] == ["t3a", "t3b"]
