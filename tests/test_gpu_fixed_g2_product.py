"""c12381_pair_product_fixed_g2_batch: gt[i] = prod_{j < k} e(g1s[j*n + i], g2s[j]) over k line tables (k_pairk.hip), k = 1 .. 8.
Checked in bytes and status against c12381_pair_product_batch on replicated G2 points (k <= 3), against the GT product of k
c12381_pair_fixed_g2_batch results (every k) and against the CPU oracle on a sample; small batches run entirely through the work queue,
n = 2^16 + 5 runs whole groups, the queue and a ragged tail."""
import pytest

from util import R, cat, golden, prng

pytestmark = pytest.mark.gpu

OFF_CURVE = (1).to_bytes(48, "big") + (1).to_bytes(48, "big")


@pytest.fixture(scope="module")
def ctx():
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pts(ctx):
    """1000 G1 points (index 0 at infinity), 8 G2 points of G2, a twist point outside G2 and G2 infinity"""
    g1 = bytes.fromhex(golden("g1")["generator"])
    g2 = bytes.fromhex(golden("g2")["generator"])
    sc = b"".join((prng(7101, i) % R).to_bytes(32, "big") for i in range(1000))
    p = bytes(96) + ctx.g1_mul(g1 * 999, sc[32:], 96)
    q = ctx.g2_mul(g2 * 8, sc[:256], 192)
    off = cat(golden("g2")["offsubgroup_points"])[:192]
    return p, [q[192 * j:192 * j + 192] for j in range(8)], off


def _cols(p, n, k, shift=0):
    return [(p[96 * ((37 * j + shift) % 1000):] + p * (n // 1000 + 2))[:96 * n] for j in range(k)]


def _raw(ctx, name, n, k, g1s, g2s, flags=0):
    """(status, bytes) of a host entry called directly"""
    import ctypes
    from crypto12381_amd.capi import _p
    out = ctypes.create_string_buffer(576 * n)
    rc = getattr(ctx.lib, name)(ctx.h, n, k, _p(g1s), _p(g2s), _p(out), flags)
    return rc, out.raw


def _prod(ctx, vals):
    acc = vals[0]
    for v in vals[1:]:
        acc = ctx.gt_op("mul", acc, v)
    return acc


@pytest.mark.parametrize("n", [50, (1 << 16) + 5])
@pytest.mark.parametrize("k", range(1, 9))
def test_product_matches_single_tables(ctx, pts, k, n):
    p, q, _ = pts
    cols = _cols(p, n, k)
    got = ctx.pair_product_fixed_g2(b"".join(cols), b"".join(q[:k]), k)
    assert len(got) == 576 * n
    assert got == _prod(ctx, [ctx.pair_fixed_g2(cols[j], q[j]) for j in range(k)])
    if k <= 3:
        assert got == ctx.pair_product(b"".join(cols), b"".join(q[j] * n for j in range(k)), k)


def test_product_sample_vs_oracle(ctx, pts, oracle_port):
    p, q, off = pts
    n, k = 12, 5
    qs = [q[0], off, bytes(192), q[3], q[4]]                   # an element of G2, a twist point outside G2, infinity
    cols = _cols(p, n, k, 3)
    cols[2] = bytes(96) + cols[2][96:]
    got = ctx.pair_product_fixed_g2(b"".join(cols), b"".join(qs), k)
    want = oracle_port.pair(cols[0], qs[0] * n, 4)
    for j in range(1, k):
        want = oracle_port.gt_op("mul", want, oracle_port.pair(cols[j], qs[j] * n, 4))
    assert got == want


def test_product_miller_only(ctx, pts):
    from crypto12381_amd.capi import F_MILLER_ONLY
    p, q, off = pts
    n = 40
    for qs in ([q[1], q[2]], [q[0], bytes(192), off, q[5], q[6], q[7]]):
        k = len(qs)
        cols = _cols(p, n, k, 11)
        cols[0] = bytes(96) + cols[0][96:]                     # G1 infinity contributes 1 to the Miller value
        got = ctx.pair_product_fixed_g2(b"".join(cols), b"".join(qs), k, flags=F_MILLER_ONLY)
        assert got == _prod(ctx, [ctx.miller(cols[j], qs[j] * n) for j in range(k)])
        if k <= 3:
            assert got == ctx.pair_product(b"".join(cols), b"".join(x * n for x in qs), k, flags=F_MILLER_ONLY)
        # the GT product afterwards uses normalised tables again (rule change = rebuild)
        assert ctx.pair_product_fixed_g2(b"".join(cols), b"".join(qs), k) == _prod(ctx, [ctx.pair_fixed_g2(cols[j], qs[j]) for j in range(k)])


def test_product_off_subgroup_and_infinity(ctx, pts):
    p, q, off = pts
    n = 100
    qs = [off, bytes(192), q[2]]
    cols = _cols(p, n, 3, 5)
    got = ctx.pair_product_fixed_g2(b"".join(cols), b"".join(qs), 3)
    assert got == ctx.pair_product(b"".join(cols), b"".join(x * n for x in qs), 3)


def test_product_invalid_points(ctx, pts):
    from crypto12381_amd.capi import C12381Error
    p, q, _ = pts
    n, k = 30, 4
    cols = _cols(p, n, k, 9)
    bad_q = q[1][:191] + bytes([q[1][191] ^ 1])                # off the twist: every lane poisoned
    qs = [q[0], bad_q, q[2], q[3]]
    assert ctx.pair_product_fixed_g2(b"".join(cols), b"".join(qs), k, strict=False) == b"\xff" * (576 * n)
    with pytest.raises(C12381Error):
        ctx.pair_product_fixed_g2(b"".join(cols), b"".join(qs), k)
    # one G1 lane off the curve poisons only itself
    want = _prod(ctx, [ctx.pair_fixed_g2(cols[j], q[j]) for j in range(k)])
    cols[2] = cols[2][:96 * 7] + OFF_CURVE + cols[2][96 * 8:]
    got = ctx.pair_product_fixed_g2(b"".join(cols), b"".join(q[:k]), k, strict=False)
    assert got[576 * 7:576 * 8] == b"\xff" * 576
    assert got[:576 * 7] == want[:576 * 7] and got[576 * 8:] == want[576 * 8:]
    # k <= 3: bytes and status of pair_product_batch, poisoned lane included
    c3 = b"".join(cols[:3])
    assert _raw(ctx, "c12381_pair_product_fixed_g2_batch", n, 3, c3, b"".join(q[:3])) == \
        _raw(ctx, "c12381_pair_product_batch", n, 3, c3, b"".join(x * n for x in q[:3]))


def test_product_table_cache(ctx, pts):
    """consecutive calls with changed points: a table is rebuilt exactly when its point (or rule) changes"""
    p, q, off = pts
    n = 64
    cols = _cols(p, n, 3, 21)
    g1s = b"".join(cols)
    seq = [[q[0], q[1], q[2]], [q[0], q[5], q[2]], [q[0], q[5], q[2]], [q[4], q[5], off], [q[0], q[1], q[2]]]
    for qs in seq:
        got = ctx.pair_product_fixed_g2(g1s, b"".join(qs), 3)
        assert got == _prod(ctx, [ctx.pair_fixed_g2(cols[j], qs[j]) for j in range(3)])
        assert got == ctx.pair_product(g1s, b"".join(x * n for x in qs), 3)
