"""G2 and the pairing routes on the device, fed with structured inputs of the twist (g2_twist.py): points of order 13 — the Miller loop
adds Q to T = -Q at i = 61, doubles infinity at i = 60, 59, 58 and adds to infinity at i = 58; the 16-entry window table of a
multiplication holds infinity at entry 13 — points of order 23 and 2713 and G2gen + T13 as controls outside G2, infinity, and compressed
x coordinates whose right-hand side is real.  Lane placement is what these tests vary: a pairing takes three lanes (21 per wavefront), a
G2 multiplication two (32 per wavefront); a degenerate lane stands first in a group, last in a group and alone in one, one group is
degenerate throughout, and the 63-lane pattern is run once tiled to the smallest batch that takes the work-queue kernels.  Every input is
computed on the CPU and every expected value comes from the CPU oracle (pinned to the compiled reference on these inputs by
test_oracle_golden.py)."""
import pytest

import g2_twist as tw
from util import R, prng

pytestmark = pytest.mark.gpu

TRI = 21                                    # pairings per wavefront (TRI_PER_WAVE)
DUO = 32                                    # G2 multiplications per wavefront
QUEUE_WAVES = 2048                          # api_pair.hip PAIR_QUEUE_WAVES: more wavefront groups than this take the work queue
BIG = QUEUE_WAVES * TRI + 1                 # 2049 groups, the last one ragged: one lane alone


def _b32(k):
    return (k % (1 << 256)).to_bytes(32, "big")


def _differs(got, want, w, labels=None):
    assert len(got) == len(want) and len(got) % w == 0
    bad = [i for i in range(len(got) // w) if got[w * i:w * i + w] != want[w * i:w * i + w]]
    return [(i, labels[i % len(labels)]) if labels else i for i in bad[:12]]


@pytest.fixture(scope="module")
def ctx():
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pts():
    p = tw.twist_points()
    assert tw.degenerate_steps(13) == [(61, tw.ADD_NEG), (60, tw.DBL_INF), (59, tw.DBL_INF), (58, tw.DBL_INF), (58, tw.ADD_INF)]
    assert all(tw.degenerate_steps(q) == [] for q in (23, 2713))
    assert all(tw.on_curve(v) for v in p.values()) and tw.ec_mul(13, p["t13a"]) is None and tw.ec_mul(13, p["t13b"]) is None
    assert len(p) <= 40
    return p


ORDER13 = ["t13a", "t13b"] + ["%d*t13a" % j for j in range(2, 13)]


@pytest.fixture(scope="module")
def pattern(pts, oracle_port):
    """63 pairing lanes in three groups: an order-13 lane first in group 0 (infinity last), controls in the middle of group 1, a G1
    argument at infinity and an order-13 lane last in it, group 2 of order-13 points throughout.  (G1 bytes, G2 bytes, labels, oracle
    Miller values, oracle pairings) — computed once and shared."""
    g = tw.generator()
    ordinary = [tw.enc192(tw.ec_mul(prng(9701, i) % R, g)) for i in range(8)]
    names = []
    for i in range(3 * TRI):
        grp, pos = divmod(i, TRI)
        if grp == 0:
            names.append("t13a" if pos == 0 else "inf" if pos == TRI - 1 else None)
        elif grp == 1:
            names.append({9: "t23", 10: "t2713", 11: "g+t13", TRI - 1: "t13b"}.get(pos))
        else:
            names.append(ORDER13[pos % len(ORDER13)])
    g1 = tw.g1_ordinary(3 * TRI, 9702)
    g1[TRI + 3] = bytes(96)                                                   # an ordinary G2 point against G1 infinity
    g1[2 * TRI + 5] = bytes(96)                                               # and an order-13 one
    q = [tw.enc192(pts[k]) if k else ordinary[i % 8] for i, k in enumerate(names)]
    labels = [k or "ordinary" for k in names]
    assert labels[0] == "t13a" and labels[2 * TRI - 1] == "t13b" and all(k in ORDER13 for k in labels[2 * TRI:])
    p1, q2 = b"".join(g1), b"".join(q)
    return p1, q2, labels, oracle_port.miller(p1, q2), oracle_port.pair(p1, q2, 16)


def _tile(buf, w, n):
    reps = n // (len(buf) // w) + 1
    return (buf * reps)[:w * n]


# ---------------------------------------------------------------- decoding
def test_g2_decompress_real_rhs_and_small_order(ctx, oracle_port, pts):
    """host and _dev form: the points' own encodings, the four classes of a real right-hand side under both tags (two of them decode
    to y = (0, 0) as the reference does, two to the true root) and the imaginary controls; expected bytes from Python integers"""
    import torch
    cases = [(k, tw.compress(v), tw.enc192(v)) for k, v in pts.items()] + tw.real_rhs_cases()
    assert sum(1 for c in cases if c[0].startswith("real")) == 8
    labels = [c[0] for c in cases]
    n = len(cases)
    c97, want = b"".join(c[1] for c in cases), b"".join(c[2] for c in cases)
    assert (want, b"\x01" * n) == oracle_port.g2_decompress(c97)
    out, st = ctx.g2_decompress(c97)
    assert st == b"\x01" * n and _differs(out, want, 192, labels) == []
    # a ragged batch over several wavefronts, the special encodings at either end of each
    m = 4 * 64 + 7
    big = _tile(c97, 97, m)
    dev = torch.device("cuda", 0)
    din = torch.frombuffer(bytearray(big), dtype=torch.uint8).to(dev)
    dout = torch.empty(192 * m, dtype=torch.uint8, device=dev)
    dst = torch.empty(m, dtype=torch.uint8, device=dev)
    ctx.g2_decompress_dev(m, din.data_ptr(), dout.data_ptr(), dst.data_ptr())
    assert ctx.sync() == 0
    assert dst.cpu().numpy().tobytes() == b"\x01" * m
    assert _differs(dout.cpu().numpy().tobytes(), _tile(want, 192, m), 192, labels) == []


# ---------------------------------------------------------------- multiplication, addition, product
MUL_NAMES = ["inf", "t13a", "t13b", "5*t13a", "12*t13a", "t23", "t2713", "g+t13", "g"]


def test_g2_mul_edge_scalars_on_small_order_bases(ctx, oracle_port, pts):
    """every base with every edge scalar (0..16 reach each window entry; entry 13 of an order-13 base is infinity), at 97 and 192
    bytes, from 192-byte and from compressed input"""
    from crypto12381_amd.capi import F_COMPRESSED_IN
    ks = tw.g2_edge_scalars() + [prng(9711, i) % (1 << 256) for i in range(4)]
    sb = b"".join(_b32(k) for k in ks) * len(MUL_NAMES)
    pb = b"".join(tw.enc192(pts[k]) * len(ks) for k in MUL_NAMES)
    cb = b"".join(tw.compress(pts[k]) * len(ks) for k in MUL_NAMES)
    labels = [(k, hex(s)) for k in MUL_NAMES for s in ks]
    for fmt in (97, 192):
        want = oracle_port.g2_mul(pb, sb, fmt, 16)
        assert _differs(ctx.g2_mul(pb, sb, fmt), want, fmt, labels) == [], fmt
        assert _differs(ctx.g2_mul_flags(cb, sb, fmt, F_COMPRESSED_IN), want, fmt, labels) == [], fmt


def test_g2_mul_lane_placement(ctx, oracle_port, pts):
    """three groups of 32 points: a small-order base first, last, and throughout; then one such lane alone in the last group"""
    g = tw.generator()
    ordinary = [tw.enc192(tw.ec_mul(prng(9712, i) % R, g)) for i in range(8)]
    ks = tw.g2_edge_scalars()
    rows = []
    for i in range(3 * DUO + 1):
        grp, pos = divmod(i, DUO)
        name = ("t13a" if pos == 0 else None, "t23" if pos == DUO - 1 else None, ORDER13[pos % 13], "t13b")[grp]
        rows.append((tw.enc192(pts[name]) if name else ordinary[i % 8], ks[(5 * i + 13) % len(ks)] if name else prng(9713, i) % (1 << 256), name or "ordinary"))
    pb, sb, labels = b"".join(r[0] for r in rows), b"".join(_b32(r[1]) for r in rows), [r[2] for r in rows]
    want = oracle_port.g2_mul(pb, sb, 192, 16)
    assert _differs(ctx.g2_mul(pb, sb, 192), want, 192, labels) == []
    assert ctx.g2_mul(pb[:192], _b32(13), 192) == oracle_port.g2_mul(pb[:192], _b32(13), 192)                  # alone in a batch
    assert ctx.g2_mul(pb[:192], _b32(14), 97) == oracle_port.g2_mul(pb[:192], _b32(14), 97)


def test_g2_mul_fixed_takes_the_generic_route_outside_g2(ctx, oracle_port, pts):
    ks = tw.g2_edge_scalars() + [prng(9714, i) % (1 << 256) for i in range(40)]
    sb = b"".join(_b32(k) for k in ks)
    for name in ("t13a", "t23", "g+t13"):
        base = tw.enc192(pts[name])
        for fmt in (97, 192):
            assert _differs(ctx.g2_mul_fixed(base, sb, fmt), oracle_port.g2_mul(base * len(ks), sb, fmt, 16), fmt, [hex(k) for k in ks]) == [], (name, fmt)


def test_g2_add_and_product_with_small_order_terms(ctx, oracle_port, pts):
    names = ["inf", "t13a", "12*t13a", "2*t13a", "t13b", "t23", "g+t13", "g"]
    a = b"".join(tw.enc192(pts[p]) for p in names for _ in names)
    b = b"".join(tw.enc192(pts[q]) for _ in names for q in names)
    labels = [(p, q) for p in names for q in names]
    assert ctx.g2_add(a, b, 192) == b"".join(tw.enc192(tw.ec_add(pts[p], pts[q])) for p, q in labels)      # P + P, P + (-P), with infinity
    for fmt in (97, 192):
        assert _differs(ctx.g2_add(a, b, fmt), oracle_port.g2_add(a, b, fmt), fmt, labels) == [], fmt
    # the product: multiply each term, then the chain of additions; the order-13 terms alone sum to infinity on the way
    terms = ["t13a", "12*t13a", "g", "t13b", "t23", "inf", "g+t13", "5*t13a", "5g"]
    tp = b"".join(tw.enc192(pts[k]) for k in terms)
    assert ctx.g2_msm(tp[:384], None, 192) == bytes(192)
    for sc in (None, b"".join(_b32(k) for k in (1, 13, R - 1, 14, 23, 7, tw.X, 26, (1 << 256) - 1))):
        t = tp if sc is None else oracle_port.g2_mul(tp, sc, 192, 4)
        acc = bytes(192)
        for i in range(len(terms)):
            acc = oracle_port.g2_add(acc, t[192 * i:192 * i + 192], 192)
        assert ctx.g2_msm(tp, sc, 192) == acc
        assert ctx.g2_msm(tp, sc, 97) == oracle_port.g2_compress(acc)


# ---------------------------------------------------------------- pairings
def test_pair_miller_fexp_on_the_pattern(ctx, oracle_port, pattern):
    """the 63-lane pattern through pair, miller and fexp (with the all-zero element and one), from 192-byte and compressed input; a
    degenerate lane alone in a batch and alone in the last group"""
    from crypto12381_amd.capi import F_COMPRESSED_IN
    p1, q2, labels, mil, gt = pattern
    n = len(labels)
    assert _differs(ctx.miller(p1, q2), mil, 576, labels) == []
    assert _differs(ctx.pair(p1, q2), gt, 576, labels) == []
    one = bytes(575) + b"\x01"
    f = bytes(576) + one + mil
    assert oracle_port.fexp(mil) == gt
    assert _differs(ctx.fexp(f), oracle_port.fexp(bytes(576) + one) + gt, 576) == []
    c1, c2 = oracle_port.g1_compress(p1), b"".join(tw.compress(tw.dec192(q2[192 * i:192 * i + 192])) for i in range(n))
    assert _differs(ctx.pair_flags(c1, c2, F_COMPRESSED_IN), gt, 576, labels) == []
    assert ctx.pair(p1[:96], q2[:192]) == gt[:576] and ctx.miller(p1[:96], q2[:192]) == mil[:576]            # alone in a batch
    m = TRI + 1                                                                                                # alone in the last group
    pa, qa = p1[96:96 * (TRI + 1)] + p1[:96], q2[192:192 * (TRI + 1)] + q2[:192]
    assert ctx.pair(pa, qa) == gt[576:576 * m] + gt[:576]
    assert ctx.miller(pa, qa) == mil[576:576 * m] + mil[:576]


def test_pair_eq_and_products_on_the_pattern(ctx, oracle_port, pattern):
    """pair_eq, pair_product for k = 2, 3 with and without F_MILLER_ONLY: a degenerate point in one slot, in another, in all"""
    from crypto12381_amd.capi import F_MILLER_ONLY
    p1, q2, labels, mil, gt = pattern
    n = len(labels)
    rot = lambda buf, w, j: buf[w * j:] + buf[:w * j]
    b1, b2 = rot(p1, 96, 2 * TRI + 2), rot(q2, 192, 2 * TRI - 4)             # the all-degenerate group meets groups 0 and 1
    c1, c2 = rot(p1, 96, 7), rot(q2, 192, TRI)
    want_eq = oracle_port.pair_eq(p1 + p1, q2 + q2, p1 + b1, q2 + b2, 16)
    assert set(want_eq[:n]) == {1} and 0 in want_eq[n:]
    assert ctx.pair_eq(p1 + p1, q2 + q2, p1 + b1, q2 + b2) == want_eq
    want2 = oracle_port.pair2(p1, q2, b1, b2)
    assert _differs(ctx.pair_product(p1 + b1, q2 + b2, 2), want2, 576, labels) == []
    mul = lambda x, y: oracle_port.gt_op("mul", x, y)
    m2 = mul(mil, oracle_port.miller(b1, b2))
    assert _differs(ctx.pair_product(p1 + b1, q2 + b2, 2, F_MILLER_ONLY), m2, 576, labels) == []
    m3 = mul(m2, oracle_port.miller(c1, c2))
    assert _differs(ctx.pair_product(p1 + b1 + c1, q2 + b2 + c2, 3, F_MILLER_ONLY), m3, 576, labels) == []
    assert _differs(ctx.pair_product(p1 + b1 + c1, q2 + b2 + c2, 3), oracle_port.fexp(m3), 576, labels) == []


def test_fixed_g2_routes_with_small_order_arguments(ctx, oracle_port, pts, pattern):
    """pair_fixed_g2 with an order-13 and an order-23 argument equals pair; pair_product_fixed_g2 for k = 1, 2, 3, 8 with the order-13
    point in each position in turn, with and without F_MILLER_ONLY, against the product of the oracle's values"""
    from crypto12381_amd.capi import F_MILLER_ONLY
    p1 = pattern[0]
    n = TRI + 2
    g1 = [p1[96 * j:96 * (j + n)] for j in range(8)]                        # k columns of n G1 points; column j has infinity in lane TRI + 3 - j
    mul = lambda x, y: oracle_port.gt_op("mul", x, y)
    mils = {}

    def miller(name, col):
        if (name, col) not in mils:
            mils[name, col] = oracle_port.miller(g1[col], tw.enc192(pts[name]) * n)
        return mils[name, col]
    for name in ("t13a", "t23", "5*t13a"):
        q = tw.enc192(pts[name])
        assert _differs(ctx.pair_fixed_g2(g1[2], q), oracle_port.pair(g1[2], q * n, 16), 576) == [], name
    others = ["g", "5g", "t23", "g+t13", "t13b", "t2713", "inf"]
    for k in (1, 2, 3, 8):
        for at in range(k):
            names = others[:k - 1]
            names.insert(at, "t13a")
            g2s = b"".join(tw.enc192(pts[x]) for x in names)
            g1s = b"".join(g1[:k])
            m = None
            for col, x in enumerate(names):
                m = miller(x, col) if m is None else mul(m, miller(x, col))
            assert _differs(ctx.pair_product_fixed_g2(g1s, g2s, k, F_MILLER_ONLY), m, 576) == [], (k, at)
            assert _differs(ctx.pair_product_fixed_g2(g1s, g2s, k), oracle_port.fexp(m), 576) == [], (k, at)


def test_work_queue_kernels_on_the_tiled_pattern(ctx, oracle_port, pts, pattern):
    """the 63-lane pattern tiled to 2049 wavefront groups (one more than the plain grid serves, the last group a single lane): the
    work-queue kernels of pair, miller, pair_eq, the 2-way product, pair_fixed_g2 and the fixed 2-way product; the oracle's values
    of the pattern, tiled"""
    p1, q2, labels, mil, gt = pattern
    n = len(labels)
    assert (BIG + TRI - 1) // TRI == QUEUE_WAVES + 1
    P, Q = _tile(p1, 96, BIG), _tile(q2, 192, BIG)
    assert _differs(ctx.pair(P, Q), _tile(gt, 576, BIG), 576, labels) == []
    assert _differs(ctx.miller(P, Q), _tile(mil, 576, BIG), 576, labels) == []
    rot = lambda buf, w, j: buf[w * j:] + buf[:w * j]
    b1, b2 = rot(p1, 96, 2 * TRI + 2), rot(q2, 192, 2 * TRI - 4)
    B1, B2 = _tile(b1, 96, BIG), _tile(b2, 192, BIG)
    assert _differs(ctx.pair_product(P + B1, Q + B2, 2), _tile(oracle_port.pair2(p1, q2, b1, b2), 576, BIG), 576, labels) == []
    assert ctx.pair_eq(P, Q, B1, B2) == _tile(oracle_port.pair_eq(p1, q2, b1, b2, 16), 1, BIG)
    t13, t23 = tw.enc192(pts["t13a"]), tw.enc192(pts["t23"])
    f13, f23 = oracle_port.pair(p1, t13 * n, 16), oracle_port.pair(b1, t23 * n, 16)
    assert _differs(ctx.pair_fixed_g2(P, t13), _tile(f13, 576, BIG), 576) == []
    assert _differs(ctx.pair_product_fixed_g2(P + B1, t13 + t23, 2), _tile(oracle_port.gt_op("mul", f13, f23), 576, BIG), 576) == []


def test_split_and_miller_only_queue_kernels_on_the_tiled_pattern(ctx, oracle_port, pts, pattern):
    """the same 2049 groups (1025 whole, 1024 through the queue, the last one a single lane) for the two queue kernels the test above does not
    reach in this regime: the final exponentiation alone (six tasks per queued group, step 0 reads the input array) on the tiled Miller
    values, and the K-way fixed product with F_MILLER_ONLY (the last Miller task ends the group); the oracle's values of the pattern, tiled"""
    from crypto12381_amd.capi import F_MILLER_ONLY
    p1, q2, labels, mil, gt = pattern
    n = len(labels)
    assert _differs(ctx.fexp(_tile(mil, 576, BIG)), _tile(oracle_port.fexp(mil), 576, BIG), 576, labels) == []
    b1 = p1[96 * (2 * TRI + 2):] + p1[:96 * (2 * TRI + 2)]
    t13, t23 = tw.enc192(pts["t13a"]), tw.enc192(pts["t23"])
    m = oracle_port.gt_op("mul", oracle_port.miller(p1, t13 * n), oracle_port.miller(b1, t23 * n))
    got = ctx.pair_product_fixed_g2(_tile(p1, 96, BIG) + _tile(b1, 96, BIG), t13 + t23, 2, F_MILLER_ONLY)
    assert _differs(got, _tile(m, 576, BIG), 576) == []


# ---------------------------------------------------------------- verifiers with a fixed G2 argument of order 13
def test_ps_verify_with_an_order_13_key(ctx, oracle_port, pts):
    """ok[j] = [e(s1_j, X2 + sum m_ij Y2_i) == e(s2_j, g2)] with g2, X2 or Y2 of order 13: not in G2, so the generic route; verdicts
    against the oracle's pair_eq on W_j formed with the oracle's g2_mul / g2_add"""
    n = TRI + 2
    g = tw.generator()
    t13a, t13b, ordq = tw.enc192(pts["t13a"]), tw.enc192(pts["t13b"]), tw.enc192(tw.ec_mul(prng(9721, 0) % R, g))
    s1 = b"".join(tw.g1_ordinary(n, 9722))
    s2 = b"".join(tw.g1_ordinary(n, 9723))
    s2 = s1[:96 * 3] + s2[96 * 3:96 * (n - 1)] + bytes(96)                    # lanes 0..2: s2 = s1; the last lane: infinity
    for g2, X2, Y2 in ((t13a, ordq, b""), (tw.enc192(g), t13a, b""), (t13a, t13a, b""), (t13a, t13b, t13a), (tw.enc192(g), ordq, t13a + t13b)):
        nmsg = len(Y2) // 192
        ms = [[(0, 1, 12, 13, R - 1)[(j + i) % 5] if j < 10 else prng(9724, 7 * j + i) % (1 << 256) for i in range(nmsg)] for j in range(n)]
        m = b"".join(_b32(ms[j][i]) for i in range(nmsg) for j in range(n))
        W = X2 * n
        for i in range(nmsg):
            W = oracle_port.g2_add(W, oracle_port.g2_mul(Y2[192 * i:192 * i + 192] * n, m[32 * n * i:32 * n * (i + 1)], 192, 8), 192)
        want = oracle_port.pair_eq(s1, W, s2, g2 * n, 16)
        assert ctx.ps_verify(g2, X2, Y2, s1, s2, m) == want, (g2 == t13a, X2 == t13a, nmsg, list(want))
        if X2 == g2:
            assert set(want[:3]) == {1}                                     # e(s1, T) == e(s1, T)


def test_bbs_plus_verify_with_an_order_13_key(ctx, oracle_port, pts):
    """ok[j] = [e(A_j, w + x_j g2) == e(g1 + r_j h0 + sum m_ij h_i, g2)] with g2 or w of order 13 (the generic route): verdicts against
    the oracle's evaluation of the same equation"""
    import g1_torsion
    n, nmsg = TRI + 2, 2
    g = tw.generator()
    t13a, t13b = tw.enc192(pts["t13a"]), tw.enc192(pts["t13b"])
    G1 = g1_torsion.enc(g1_torsion.generator())
    hs = tw.g1_ordinary(nmsg + 1, 9731)
    h0, h = hs[0], b"".join(hs[1:])
    A = b"".join(tw.g1_ordinary(n, 9732))
    x = b"".join(_b32((0, 1, 12, 13, R - 1)[j % 5] if j < 10 else prng(9733, j)) for j in range(n))
    r = b"".join(_b32(prng(9734, j)) for j in range(n))
    m = b"".join(_b32(prng(9735, i * n + j)) for i in range(nmsg) for j in range(n))
    verdicts = set()
    for g2, w in ((t13a, tw.enc192(tw.ec_mul(5, g))), (tw.enc192(g), t13a), (t13a, t13b), (t13a, t13a)):
        want = oracle_port.bbs_plus_verify(G1, g2, h0, h, w, A, x, r, m, 16)
        assert ctx.bbs_plus_verify(G1, g2, h0, h, w, A, x, r, m) == want, (g2 == t13a, w == t13a, list(want))
        verdicts |= set(want)
    assert verdicts <= {0, 1}
