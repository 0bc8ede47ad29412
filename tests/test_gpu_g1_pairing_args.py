"""The pairing routes on the device, fed with structured G1 arguments (g1_pairing_args.py): (0, +-2) of order 3 — px = 0, so l2 vanishes
in every line of the running-point loop and only the pass-through term is left of the product against a normalised table — G + T3,
points of order 11 and 10177, the curve points with the smallest and the largest x, the three points that share a y, infinity, and P
beside -P.  What these tests vary is the route (running-point loop; fixed-G2 tables, normalised and raw), the lane placement (first in a
wavefront group of 21 pairings, last in it, alone in one; whole groups and queued ones in a batch tiled to 2049 groups) and, for the
K-way product, the column pattern behind the prep kernel's mask word.  Every input is computed on the CPU and every expected value is
the CPU oracle's (pinned to the compiled reference on these inputs by test_g1_pairing_args.py); all comparisons are byte-exact."""
import pytest

import g1_pairing_args as ga
import g2_twist as tw

pytestmark = pytest.mark.gpu

TRI, BIG = ga.TRI, ga.BIG
ONE = ga.ONE


@pytest.fixture(scope="module")
def ctx():
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pat(oracle_port):
    """the 63-lane pattern: (G1 bytes, G2 bytes, labels, oracle Miller values, oracle pairings) — computed once and shared"""
    assert ga.self_check()
    lanes = ga.pattern()
    p1, q2 = ga.lane_bytes(lanes)
    return p1, q2, ["%s,%s" % l for l in lanes], oracle_port.miller(p1, q2), oracle_port.pair(p1, q2, 16)


@pytest.fixture(scope="module")
def mils(oracle_port):
    return ga.Millers(oracle_port)


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(torch.device("cuda", 0))


def _sides(p1, q2):
    """the second pair of pair_eq and of the 2-way product: the pattern rotated so that the degenerate group meets groups 0 and 1"""
    return ga.rot(p1, 96, 2 * TRI + 2), ga.rot(q2, 192, 2 * TRI - 4)


# ---------------------------------------------------------------- the running-point loop
def test_pair_miller_and_product_on_the_pattern(ctx, oracle_port, pat):
    """pair, miller, fexp of the Miller values, pair_product(k = 2) with and without F_MILLER_ONLY"""
    from crypto12381_amd.capi import F_MILLER_ONLY
    p1, q2, labels, mil, gt = pat
    assert ga.differs(ctx.miller(p1, q2), mil, 576, labels) == ""
    assert ga.differs(ctx.pair(p1, q2), gt, 576, labels) == ""
    assert ga.differs(ctx.fexp(mil), gt, 576, labels) == ""
    assert gt[576 * (2 * TRI + 17):576 * (2 * TRI + 18)] == bytes(576)            # px = 0 against G2 infinity: the zero element
    b1, b2 = _sides(p1, q2)
    assert ga.differs(ctx.pair_product(p1 + b1, q2 + b2, 2), oracle_port.pair2(p1, q2, b1, b2), 576, labels) == ""
    m2 = oracle_port.gt_op("mul", mil, oracle_port.miller(b1, b2))
    assert ga.differs(ctx.pair_product(p1 + b1, q2 + b2, 2, F_MILLER_ONLY), m2, 576, labels) == ""


def _eq_lists(p1, q2):
    b1, b2 = _sides(p1, q2)
    zero = bytes(96) * 4
    return zero + p1 + p1, q2[:192 * 4] + q2 + q2, zero + b1 + p1, q2[192 * 4:192 * 8] + b2 + q2


def test_pair_eq_on_the_pattern(ctx, oracle_port, pat):
    """the degenerate classes on the a1 side and on the negated b1 side (py = 2 and py = p - 2 through fp_negate), a = b identical, both
    G1 arguments at infinity against different G2 points"""
    p1, q2, labels, _, _ = pat
    n = len(labels)
    a1, a2, c1, c2 = _eq_lists(p1, q2)
    want = oracle_port.pair_eq(a1, a2, c1, c2, 16)
    assert set(want[:4]) == {1} and 0 in want[4:4 + n] and [i for i in range(n) if want[4 + n + i] != 1] == [2 * TRI + 17]
    got = ctx.pair_eq(a1, a2, c1, c2)
    assert got == want, [i for i in range(len(want)) if got[i] != want[i]]


# ---------------------------------------------------------------- one fixed G2 point
def test_pair_fixed_g2_on_the_pattern(ctx, oracle_port, pat):
    """every G1 lane of the pattern against one G2 point (a normalised table) and against G2 infinity (the table stays raw; the px = 0
    lanes give the zero element): host form, _dev form, and the same call again from the cached table"""
    import torch
    p1, _, labels, _, _ = pat
    n = len(labels)
    g1names = [l.split(",")[0] for l in labels]
    for q in ("q3", "inf2"):
        qb = ga.g2_points()[q]
        want = oracle_port.pair(p1, qb * n, 16)
        got = ctx.pair_fixed_g2(p1, qb)
        assert ga.differs(got, want, 576, labels) == "", q
        assert ctx.pair_fixed_g2(p1, qb) == got, q
        out, da, db = torch.empty(576 * n, dtype=torch.uint8, device="cuda"), _dev(p1), _dev(qb)
        ctx.pair_fixed_g2_dev(n, da.data_ptr(), db.data_ptr(), out.data_ptr())
        assert ctx.sync() == 0 and bytes(out.cpu().numpy()) == got, q
        if q == "inf2":
            assert [i for i in range(n) if want[576 * i:576 * i + 576] == bytes(576)] == [i for i, k in enumerate(g1names) if k in ("t3a", "t3b")]


@pytest.mark.parametrize("name", ga.PLACED)
def test_every_class_first_last_and_alone(ctx, oracle_port, mils, name):
    """22 lanes: one point of the class first in a group, last in it and alone in the next — through the running-point loop, a
    normalised table, a raw table (F_MILLER_ONLY) and the raw table of G2 infinity"""
    from crypto12381_amd.capi import F_MILLER_ONLY
    lanes = ga.placement(name)
    labels = [l[0] for l in lanes]
    p1, q2 = ga.lane_bytes(lanes)
    mil = mils.get(lanes)
    assert ga.differs(ctx.miller(p1, q2), mil, 576, labels) == ""
    assert ga.differs(ctx.pair(p1, q2), oracle_port.fexp(mil), 576, labels) == ""
    m1 = mils.get([(a, "q1") for a in labels])
    qb = ga.g2_points()["q1"]
    assert ga.differs(ctx.pair_fixed_g2(p1, qb), oracle_port.fexp(m1), 576, labels) == ""
    assert ga.differs(ctx.pair_product_fixed_g2(p1, qb, 1, F_MILLER_ONLY), m1, 576, labels) == ""
    mi = mils.get([(a, "inf2") for a in labels])
    assert ga.differs(ctx.pair_fixed_g2(p1, bytes(192)), oracle_port.fexp(mi), 576, labels) == ""


@pytest.mark.parametrize("n", ga.RAGGED)
def test_ragged_batches_with_the_order_3_lane_last(ctx, oracle_port, mils, n):
    """n = 1, 20, 21, 22, 64: the px = 0 lane last — alone in the batch, short of a group, filling one, alone in the next"""
    from crypto12381_amd.capi import F_MILLER_ONLY
    lanes = ga.ragged(n)
    labels = [l[0] for l in lanes]
    p1, q2 = ga.lane_bytes(lanes)
    mil = mils.get(lanes)
    assert ga.differs(ctx.miller(p1, q2), mil, 576, labels) == ""
    assert ga.differs(ctx.pair(p1, q2), oracle_port.fexp(mil), 576, labels) == ""
    assert ctx.pair_eq(p1, q2, p1, q2) == b"\x01" * n
    m5 = mils.get([(a, "q5") for a in labels])
    qb = ga.g2_points()["q5"]
    assert ga.differs(ctx.pair_fixed_g2(p1, qb), oracle_port.fexp(m5), 576, labels) == ""
    assert ga.differs(ctx.pair_product_fixed_g2(p1, qb, 1, F_MILLER_ONLY), m5, 576, labels) == ""
    assert oracle_port.fexp(m5)[-576:] == ONE and m5[-576:] != ONE


# ---------------------------------------------------------------- K fixed G2 points: the column patterns
@pytest.mark.parametrize("K", ga.KS)
def test_pair_product_fixed_g2_column_patterns(ctx, oracle_port, mils, K):
    """element i of the batch is column pattern i: every single column at infinity, all, all but one, alternating, all of order 3,
    negated columns, the cancelling pair alone and beside live columns, an off-curve column beside infinity columns and beside live ones.  With distinct
    G2 points and with one point in columns 0 and 1; with F_MILLER_ONLY (raw tables: the product of the oracle's Miller values, exactly
    1 where every column is skipped) and without (the oracle's GT product; exactly 1 for all-infinity, all-order-3 and the cancelling
    pair).  A rejected element is 0xff, the status E_POINT, every other element as if it were not there; host form, _dev form and a
    second call on the cached tables return the same bytes."""
    import torch
    from crypto12381_amd.capi import C12381Error, E_POINT, F_MILLER_ONLY
    pats = ga.column_patterns(K)
    labels = [p[0] for p in pats]
    n = len(pats)
    g1s = ga.column_bytes(K)
    off = [i for i, p in enumerate(pats) if "off" in p[2]]
    assert len(off) == (1 if K == 1 else 2)
    for twin in (False, True):
        g2s = b"".join(ga.g2_points()[q] for q in ga.column_g2(K, twin))
        prod = mils.product(K, twin)
        wm = b"".join(b"\xff" * 576 if i in off else m for i, m in enumerate(prod))
        fe = oracle_port.fexp(b"".join(prod))
        wg = b"".join(b"\xff" * 576 if i in off else fe[576 * i:576 * i + 576] for i in range(n))
        for i, (label, _, claims) in enumerate(pats):                       # the claims, on the expected bytes
            if i in off:
                continue
            if "one" in claims:
                assert wm[576 * i:576 * i + 576] == ONE, label
            if "gt_one" in claims or "one" in claims or (twin and "gt_one_twin" in claims):
                assert wg[576 * i:576 * i + 576] == ONE, label
        for flags, want in ((F_MILLER_ONLY, wm), (0, wg)):
            got = ctx.pair_product_fixed_g2(g1s, g2s, K, flags, strict=False)
            assert ga.differs(got, want, 576, labels) == "", (K, twin, flags)
            assert ctx.pair_product_fixed_g2(g1s, g2s, K, flags, strict=False) == got, (K, twin, flags)
            with pytest.raises(C12381Error) as e:
                ctx.pair_product_fixed_g2(g1s, g2s, K, flags)
            assert e.value.code == E_POINT
            out, da, db = torch.zeros(576 * n, dtype=torch.uint8, device="cuda"), _dev(g1s), _dev(g2s)
            ctx.pair_product_fixed_g2_dev(n, K, da.data_ptr(), db.data_ptr(), out.data_ptr(), flags)
            assert ctx.sync() == E_POINT and bytes(out.cpu().numpy()) == got, (K, twin, flags)
        # without the rejected element the batch is clean and the others are unchanged
        keep = [i for i in range(n) if i not in off]
        clean = b"".join(g1s[96 * (c * n + i):96 * (c * n + i + 1)] for c in range(K) for i in keep)
        assert ctx.pair_product_fixed_g2(clean, g2s, K) == b"".join(wg[576 * i:576 * i + 576] for i in keep), (K, twin)


# ---------------------------------------------------------------- the work-queue kernels
def test_work_queue_kernels_on_the_tiled_pattern(ctx, oracle_port, pat):
    """the 63-lane pattern tiled to 2049 wavefront groups (1025 whole, 1024 through the queue, the last one a single lane — the first
    order-3 lane of the degenerate group): pair, miller, pair_eq and the final exponentiation of the tiled Miller values; the oracle's 63 values, tiled"""
    p1, q2, labels, mil, gt = pat
    assert (BIG + TRI - 1) // TRI == ga.QUEUE_WAVES + 1 and (BIG - 1) % 63 == 2 * TRI
    Pb, Qb = ga.tile(p1, 96, BIG), ga.tile(q2, 192, BIG)
    assert ga.differs(ctx.pair(Pb, Qb), ga.tile(gt, 576, BIG), 576, labels) == ""
    assert ga.differs(ctx.miller(Pb, Qb), ga.tile(mil, 576, BIG), 576, labels) == ""
    assert ga.differs(ctx.fexp(ga.tile(mil, 576, BIG)), ga.tile(gt, 576, BIG), 576, labels) == ""
    b1, b2 = _sides(p1, q2)
    want = oracle_port.pair_eq(p1, q2, b1, b2, 16)
    assert 0 in want and 1 in want
    got = ctx.pair_eq(Pb, Qb, ga.tile(b1, 96, BIG), ga.tile(b2, 192, BIG))
    assert ga.differs(got, ga.tile(want, 1, BIG), 1, labels) == ""


def test_fixed_g2_queue_kernels_on_the_tiled_pattern(ctx, oracle_port, pat, mils):
    """the same 2049 groups through pair_fixed_g2 and the 3-way fixed product with and without F_MILLER_ONLY; the product's columns are
    the pattern and two rotations of it, its middle G2 point is infinity (a raw table between two normalised ones)"""
    from crypto12381_amd.capi import F_MILLER_ONLY
    p1, _, labels, _, _ = pat
    n = len(labels)
    names = [l.split(",")[0] for l in labels]
    qb = ga.g2_points()
    Pb = ga.tile(p1, 96, BIG)
    assert ga.differs(ctx.pair_fixed_g2(Pb, qb["q2"]), ga.tile(oracle_port.fexp(mils.get([(a, "q2") for a in names])), 576, BIG), 576, labels) == ""
    shifts, qs = (0, 2 * TRI + 2, TRI + 5), ("q2", "inf2", "q6")
    m = None
    for s, q in zip(shifts, qs):
        col = mils.get([(names[(i + s) % n], q) for i in range(n)])
        m = col if m is None else oracle_port.gt_op("mul", m, col)
    g1s = b"".join(ga.tile(ga.rot(p1, 96, s), 96, BIG) for s in shifts)
    g2s = b"".join(qb[q] for q in qs)
    assert ga.differs(ctx.pair_product_fixed_g2(g1s, g2s, 3, F_MILLER_ONLY), ga.tile(m, 576, BIG), 576, labels) == ""
    assert ga.differs(ctx.pair_product_fixed_g2(g1s, g2s, 3), ga.tile(oracle_port.fexp(m), 576, BIG), 576, labels) == ""


# ---------------------------------------------------------------- compressed input
def test_compressed_order_3_and_extreme_x_arguments(ctx, oracle_port):
    """pair_flags(F_COMPRESSED_IN) on the 49-byte forms of (0, +-2) and of the smallest-x and largest-x points, the smallest x also as
    x + p (the decoder takes it mod p): the square root of 4, of small and of near-p right-hand sides, then the same pairing"""
    from crypto12381_amd.capi import F_COMPRESSED_IN
    names = ["t3a", "t3b", "xmin+", "xmin-", "xmax+", "xmax-", "inf", "g+t3", "m0"]
    c1 = b"".join(ga.compress(k) for k in names) + ga.compress("xmin+", add_p=True) + ga.compress("xmin-", add_p=True)
    names += ["xmin+", "xmin-"]
    p1 = b"".join(ga.enc(k) for k in names)
    assert oracle_port.g1_decompress(c1) == (p1, b"\x01" * len(names))
    qn = ["q%d" % (i % 8) for i in range(len(names))]
    q2 = b"".join(ga.g2_points()[q] for q in qn)
    c2 = b"".join(tw.compress(tw.dec192(ga.g2_points()[q])) for q in qn)
    want = oracle_port.pair(p1, q2, 8)
    assert want[:576] == ONE and want[576 * 2:576 * 3] != ONE
    assert ga.differs(ctx.pair_flags(c1, c2, F_COMPRESSED_IN), want, 576, names) == ""
    assert ctx.g1_decompress(c1) == (p1, b"\x01" * len(names))
