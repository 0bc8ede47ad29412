"""CPU tests of the device's G2 and pairing routines on structured inputs of the twist (g2_twist.py), under the bounds checker
(tests/host_sim/sim.cpp, C12381_CHECK_BOUNDS): points of order 13, whose Miller loop adds Q to T = -Q at i = 61, doubles infinity at
i = 60, 59, 58 and adds to infinity at i = 58 — the only non-zero inputs that send the line formulas of miller_dbl_step / miller_add_step,
the three-lane line products and the line tables of miller_lines_precompute through their degenerate cases — and whose 16-entry window table holds infinity at entry 13; points of order 23 and 2713 and G2gen + T13 as off-subgroup controls;
and compressed x coordinates with a real right-hand side, where fp2_sqrt has to take the sign-0 root of the norm as the reference does.
Expected values come from the oracle (pinned to the compiled reference on the same inputs by test_oracle_golden.py) and, for the
decoding, from Python integers."""
import ctypes
import os
import subprocess

import pytest

import g2_twist as tw
from util import prng

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


@pytest.fixture(scope="module")
def pts():
    p = tw.twist_points()
    assert tw.degenerate_steps(13) == [(61, tw.ADD_NEG), (60, tw.DBL_INF), (59, tw.DBL_INF), (58, tw.DBL_INF), (58, tw.ADD_INF)]
    assert all(tw.degenerate_steps(q) == [] for q in (23, 2713))
    assert all(tw.on_curve(v) for v in p.values()) and tw.ec_mul(13, p["t13a"]) is None and tw.ec_mul(13, p["t13b"]) is None
    return p


def _differs(got, want, w, labels):
    """the labels of the records that differ, as one string ("" when none does)"""
    assert len(got) == len(want) == w * len(labels)
    return "; ".join(str(labels[i]) for i in range(len(labels)) if got[w * i:w * i + w] != want[w * i:w * i + w])


def test_sim_g2_decompress_on_twist_edges(sim, oracle_port, pts):
    """the points' own encodings, the four classes of a real right-hand side under both sign tags and the imaginary controls: status 1
    everywhere, the bytes the reference's rule gives (worked out on Python integers) and the oracle's"""
    cases = [(k, tw.compress(v), tw.enc192(v)) for k, v in pts.items()] + tw.real_rhs_cases()
    assert sum(1 for c in cases if c[0].startswith("real")) == 8
    labels = [c[0] for c in cases]
    c97 = b"".join(c[1] for c in cases)
    n = len(cases)
    out, st = ctypes.create_string_buffer(192 * n), ctypes.create_string_buffer(n)
    assert sim.sim_g2_decompress_batch(sz(n), c97, out, st) == 0
    assert st.raw == b"\x01" * n
    bad = _differs(out.raw, b"".join(c[2] for c in cases), 192, labels)
    assert bad == "", bad
    assert (out.raw, st.raw) == oracle_port.g2_decompress(c97)


MUL_NAMES = ["inf", "t13a", "t13b", "5*t13a", "12*t13a", "t23", "t2713", "g+t13", "g"]


@pytest.mark.parametrize("form", ("sim_g2_mul_batch", "sim_g2h_mul_batch"))
def test_sim_g2_mul_on_small_order_bases(sim, oracle_port, pts, form):
    """an order-13 base puts infinity into entry 13 of the window table and wraps entries 14-16, an order-23 base leaves entry 16 = -7 Q;
    every base with the edge scalars, one lane per point and two lanes per point"""
    ks = tw.g2_edge_scalars() + [prng(9611, i) % (1 << 256) for i in range(4)]
    sb = b"".join(k.to_bytes(32, "big") for k in ks) * len(MUL_NAMES)
    pb = b"".join(tw.enc192(pts[k]) * len(ks) for k in MUL_NAMES)
    labels = [(k, hex(s)) for k in MUL_NAMES for s in ks]
    n = len(labels)
    for fmt in (192, 97):
        out = ctypes.create_string_buffer(fmt * n)
        assert getattr(sim, form)(sz(n), pb, sb, out, fmt) == 0
        assert _differs(out.raw, oracle_port.g2_mul(pb, sb, fmt, 4), fmt, labels) == "", fmt


def test_sim_g2_fixed_mul_refuses_bases_outside_g2(sim, oracle_port, pts):
    """the fixed-base table is for members of G2 only: every point of small order, and G2gen + T13, is sent to the generic route"""
    ks = tw.g2_edge_scalars()
    sb = b"".join(k.to_bytes(32, "big") for k in ks)
    out = ctypes.create_string_buffer(192 * len(ks))
    for k, v in pts.items():
        rc = sim.sim_g2_fixed_mul_batch(sz(len(ks)), tw.enc192(v), sb, out)
        if k in ("g", "5g"):
            assert rc == 0 and out.raw == oracle_port.g2_mul(tw.enc192(v) * len(ks), sb, 192, 4), k
        else:
            assert rc == -2, k


@pytest.fixture(scope="module")
def lanes(pts):
    """every point with an ordinary G1 argument, then T13 with the G1 argument at infinity"""
    g1 = tw.g1_ordinary(len(pts), 9612)
    labels = list(pts) + ["t13a, G1 infinity"]
    return b"".join(g1) + bytes(96), b"".join(tw.enc192(v) for v in pts.values()) + tw.enc192(pts["t13a"]), labels


@pytest.mark.parametrize("entry,ref", (("sim_pair_batch", "pair"), ("sim_pair3_batch", "pair"), ("sim_miller_batch", "miller"),
                                       ("sim_miller3_batch", "miller")))
def test_sim_miller_and_pairing_through_infinity(sim, oracle_port, lanes, entry, ref):
    p1, q2, labels = lanes
    n = len(labels)
    out = ctypes.create_string_buffer(576 * n)
    assert getattr(sim, entry)(sz(n), p1, q2, out) == 0
    assert _differs(out.raw, getattr(oracle_port, ref)(p1, q2), 576, labels) == ""


def test_sim_pair_eq_on_small_order_points(sim, oracle_port, lanes):
    p1, q2, labels = lanes
    n = len(labels)
    b1, b2 = p1[96 * 3:] + p1[:96 * 3], q2[192 * 5:] + q2[:192 * 5]
    e1, e2, f1, f2 = p1 + p1, q2 + q2, p1 + b1, q2 + b2
    want = oracle_port.pair_eq(e1, e2, f1, f2)
    assert set(want[:n]) == {1} and 0 in want[n:]
    for entry in ("sim_pair_eq_batch", "sim_pair3_eq_batch"):
        ok = ctypes.create_string_buffer(2 * n)
        assert getattr(sim, entry)(sz(2 * n), e1, e2, f1, f2, ok) == 0
        assert ok.raw == want, entry


def test_sim_fixed_g2_tables_of_small_order_points(sim, oracle_port, pts):
    """miller_lines_precompute on a point of order 13, whose lines include those of T + Q = infinity, of doubling infinity and of adding
    to infinity: the point in either slot of the two-table loop, in both, and the controls.  e(a, W) e(c, G) against the oracle's pair2"""
    g1 = tw.g1_ordinary(4, 9613)
    a, c = b"".join(g1[:3]) + bytes(96), g1[3] + b"".join(g1[:2]) + g1[2]          # one lane with a G1 argument at infinity
    n = 4
    special = ["t13a", "t13b", "5*t13a", "12*t13a", "t23", "t2713", "g+t13", "inf"]
    slots = [(s, "g") for s in special] + [("5g", s) for s in special] + [("t13a", "t13b"), ("t13a", "t13a"), ("t13b", "t23")]
    bad = []
    for w, q in slots:
        wb, qb = tw.enc192(pts[w]), tw.enc192(pts[q])
        out = ctypes.create_string_buffer(576 * n)
        assert sim.sim_pair2_fixed_batch(sz(n), a, wb, c, qb, out) == 0
        if out.raw != oracle_port.pair2(a, wb * n, c, qb * n):
            bad.append((w, q))
    assert bad == [], bad


@pytest.fixture(scope="module")
def fk():
    so = os.path.join(SIM_DIR, "libsim_fixedk.so")
    src = os.path.join(SIM_DIR, "fixed_k.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-pthread", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def test_sim_normalised_and_raw_line_tables(fk, oracle_port, pts):
    """miller_lines_precompute divides every line by its s-coefficient c1 unless one of them vanishes.  Measured here: the lines of a
    point of order 13 — the addition with T = -Q, the doublings of infinity and the addition to infinity among them — all have c1 != 0,
    so its table is normalised like the controls' (another Miller value in Fp12, the same GT value); only G2 infinity keeps a raw
    table, and the K-way loop then gives the reference's Miller value itself.  The GT value cannot tell a raw table from a wrongly
    normalised one (a table of zeros leaves powers of s, which the final exponentiation removes), so this compares Miller values.
    K = 1, and K = 2 with the raw table beside a normalised one in either order."""
    g1 = tw.g1_ordinary(3, 9614)
    col = b"".join(g1[:2]) + bytes(96)
    col2 = g1[2] + bytes(96) + g1[0]
    n = 3

    def run(g1s, g2s, k, raw, single=0):
        out = ctypes.create_string_buffer(576 * n)
        assert fk.sim_fixedk_miller(sz(n), k, g1s, g2s, raw, 16, single, out) == 0
        return out.raw
    inf = bytes(192)
    infm = oracle_port.miller_t(col2, inf * n)                               # lines (0, 0, -px): not 1 before the final exponentiation
    assert run(col2, inf, 1, raw=0) == infm and run(col2, inf, 1, raw=1) == infm and infm[:576] != infm[576:2 * 576]
    for k in ("t13a", "t13b", "5*t13a", "12*t13a", "t23", "t2713", "g+t13", "g"):
        q = tw.enc192(pts[k])
        want = oracle_port.miller_t(col, q * n)
        got = run(col, q, 1, raw=0)
        assert run(col, q, 1, raw=1) == want, k
        assert got[:576 * 2] != want[:576 * 2] and oracle_port.fexp_t(got) == oracle_port.pair(col, q * n), k
        # beside the raw table of infinity, in either order: the product of the two columns' own values
        both = oracle_port.gt_op("mul", got, infm)
        assert run(col2 + col, inf + q, 2, raw=0) == both and run(col + col2, q + inf, 2, raw=0) == both, k
