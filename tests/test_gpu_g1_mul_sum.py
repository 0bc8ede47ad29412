"""c12381_g1_mul_sum_batch on the device, through the C ABI: per-lane sums of k G1 products under one doubling chain (k_g1sum.hip).
The pinned value of a lane is the port oracle's `multiply` on every term followed by its `add` (g1_mul_sum_cases.expected; the port is
pinned to the compiled reference on these very inputs by tests/test_host_sim_g1_mul_sum.py).  Full-size batches are compared lane by
lane with the library's own composed route — c12381_g1_mul_batch per column and c12381_g1_add_batch — an independent code path that
tests/test_gpu_full_batch.py pins to the reference."""
import numpy as np
import pytest

from g1_mul_sum_cases import edge_lanes, expected, pack, related_lanes, seeded_lanes
from util import golden, prng

pytestmark = pytest.mark.gpu

KMAX = 4
OFF_CURVE = (1).to_bytes(48, "big") + (1).to_bytes(48, "big")


@pytest.fixture(scope="module")
def ctx():
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


def differing(got, exp, w):
    assert len(got) == len(exp)
    if got == exp:
        return []
    return [i for i in range(len(exp) // w) if got[w * i:w * i + w] != exp[w * i:w * i + w]]


def dev_call(ctx, pts, sc, k, fmt, flags=0):
    """the _dev form on torch tensors"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(sc) // (32 * k)
    dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).to(dev)
    ds = torch.frombuffer(bytearray(sc), dtype=torch.uint8).to(dev)
    out = torch.empty(fmt * n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ctx.g1_mul_sum_dev(n, k, dp.data_ptr(), ds.data_ptr(), out.data_ptr(), fmt, flags)
    rc = ctx.sync()
    return out.cpu().numpy().tobytes(), rc


def composed(ctx, pts, sc, k, fmt):
    """what a caller composes without this entry: one scalar-multiplication batch per column, then additions"""
    n = len(sc) // (32 * k)
    acc = ctx.g1_mul(pts[:96 * n], sc[:32 * n], fmt if k == 1 else 96)
    for j in range(1, k):
        col = ctx.g1_mul(pts[96 * n * j:96 * n * (j + 1)], sc[32 * n * j:32 * n * (j + 1)], 96)
        acc = ctx.g1_add(acc, col, fmt if j == k - 1 else 96)
    return acc


def random_columns(ctx, n, k, seed):
    """k columns of n subgroup points (multiples of the generator by the fixed-base path, the columns rotated against each other) and
    k n random 256-bit scalars"""
    g = bytes.fromhex(golden("g1")["generator"])
    rng = np.random.Generator(np.random.PCG64(seed))
    base = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    base[:, 0] &= 0x3f
    col = np.frombuffer(ctx.g1_mul_fixed(g, base.tobytes(), 96), dtype=np.uint8).reshape(n, 96)
    pts = b"".join(np.roll(col, 7919 * j, axis=0).tobytes() for j in range(k))
    sc = rng.integers(0, 256, size=(k * n, 32), dtype=np.uint8).tobytes()
    return pts, sc


@pytest.mark.parametrize("k", range(1, KMAX + 1))
def test_seeded_edge_and_related_lanes_against_the_oracle(ctx, oracle_port, k):
    """the three groups of the host-sim test in one batch, 49- and 96-byte outputs, host and _dev forms"""
    lanes = seeded_lanes(oracle_port, k, 300, 9800 + 10 * k) + edge_lanes(oracle_port, k)[0] + (related_lanes(oracle_port, k)[0] if k > 1 else [])
    pts, sc = pack(lanes, k)
    for fmt in (96, 49):
        exp = expected(oracle_port, pts, sc, k, fmt)
        got = ctx.g1_mul_sum(pts, sc, k, fmt)
        assert differing(got, exp, fmt)[:8] == []
        got, rc = dev_call(ctx, pts, sc, k, fmt)
        assert rc == 0 and differing(got, exp, fmt)[:8] == []


def test_every_lane_of_2_16_pairs_against_the_oracle(ctx, oracle_port):
    n = 1 << 16
    pts, sc = random_columns(ctx, n, 2, 9851)
    exp = expected(oracle_port, pts, sc, 2, 96, nthreads=8)
    assert differing(ctx.g1_mul_sum(pts, sc, 2, 96), exp, 96)[:8] == []


@pytest.mark.parametrize("k", (2, 4))
def test_every_lane_of_2_20_against_the_composed_route(ctx, k):
    """also several launches per call: 2 for k = 2, 4 for k = 4"""
    n = 1 << 20
    pts, sc = random_columns(ctx, n, k, 9860 + k)
    got = ctx.g1_mul_sum(pts, sc, k, 96)
    assert differing(got, composed(ctx, pts, sc, k, 96), 96)[:8] == []


def test_a_size_that_spans_two_launches_with_a_ragged_tail(ctx):
    """k = 3 runs 262 144 lanes per launch: 262 144 + 65 lanes are two launches, the second of one full wavefront and one lane"""
    n = (1 << 18) + 65
    pts, sc = random_columns(ctx, n, 3, 9870)
    for fmt in (49, 96):
        assert differing(ctx.g1_mul_sum(pts, sc, 3, fmt), composed(ctx, pts, sc, 3, fmt), fmt)[:8] == []


@pytest.mark.parametrize("n", (1, 63, 65, (1 << 16) + 1))
def test_odd_sizes(ctx, n):
    for k in (2, 3, 4):
        pts, sc = random_columns(ctx, n, k, 9880 + k)
        assert differing(ctx.g1_mul_sum(pts, sc, k, 49), composed(ctx, pts, sc, k, 49), 49)[:8] == []


def test_one_term_equals_g1_mul_batch_flags(ctx, oracle_port):
    from crypto12381_amd.capi import F_IN_SUBGROUP
    lanes = seeded_lanes(oracle_port, 1, 200, 9890) + edge_lanes(oracle_port, 1)[0]
    pts, sc = pack(lanes, 1)
    for fmt in (49, 96):
        assert ctx.g1_mul_sum(pts, sc, 1, fmt) == ctx.g1_mul_flags(pts, sc, fmt, 0)
    sub, ssc = pack(lanes[:200], 1)
    assert ctx.g1_mul_sum(sub, ssc, 1, 96, F_IN_SUBGROUP) == ctx.g1_mul_flags(sub, ssc, 96, F_IN_SUBGROUP)


def test_argument_checks(ctx, oracle_port):
    from crypto12381_amd.capi import C12381Error, E_ARG, F_COMPRESSED_IN, F_MILLER_ONLY, _p
    pts, sc = pack(seeded_lanes(oracle_port, 2, 4, 9900), 2)
    out = bytearray(96 * 4)
    lib, h = ctx.lib, ctx.h
    call = lambda n, k, p, s, o, fmt, flags: lib.c12381_g1_mul_sum_batch(h, n, k, _p(p), _p(s), _p(o), fmt, flags)
    import ctypes
    obuf = (ctypes.c_char * len(out)).from_buffer(out)
    assert call(4, 2, pts, sc, obuf, 96, 0) == 0
    for bad in ((4, 0, pts, sc, obuf, 96, 0), (4, KMAX + 1, pts, sc, obuf, 96, 0), (4, 2, pts, sc, obuf, 48, 0),
                (4, 2, pts, sc, obuf, 96, F_COMPRESSED_IN), (4, 2, pts, sc, obuf, 96, F_MILLER_ONLY), (4, 2, None, sc, obuf, 96, 0),
                (4, 2, pts, None, obuf, 96, 0), (4, 2, pts, sc, None, 96, 0), (0, 0, pts, sc, obuf, 96, 0)):
        assert call(*bad) == E_ARG, bad[:2] + bad[5:]
        assert lib.c12381_g1_mul_sum_batch_dev(h, bad[0], bad[1], None if bad[2] is None else _p(1 << 20), None if bad[3] is None else _p(1 << 20),
                                               None if bad[4] is None else _p(1 << 20), bad[5], bad[6]) == E_ARG
    with pytest.raises(C12381Error) as e:
        ctx.g1_mul_sum(pts, sc, 2, 96, F_COMPRESSED_IN)
    assert e.value.code == E_ARG
    # n = 0: OK, nothing touched — also with null pointers
    mark = bytes(out)
    assert call(0, 2, pts, sc, obuf, 96, 0) == 0 and call(0, 3, None, None, None, 49, 0) == 0 and bytes(out) == mark
    assert lib.c12381_g1_mul_sum_batch_dev(h, 0, 2, None, None, None, 96, 0) == 0
    assert ctx.g1_mul_sum(b"", b"", 2, 96) == b""


@pytest.mark.parametrize("k", (2, 3, 4))
def test_an_off_curve_point_poisons_its_lane_only(ctx, oracle_port, k):
    """one point off the curve in term 0 and one in term k - 1 (other lanes): those lanes are 0xff, every other lane is right, the call
    returns C12381_E_POINT, and the next call on the context is clean"""
    from crypto12381_amd.capi import C12381Error, E_POINT
    n = 130
    lanes = seeded_lanes(oracle_port, k, n, 9910 + k)
    good_pts, sc = pack(lanes, k)
    exp = expected(oracle_port, good_pts, sc, k, 96)
    lanes[5][0] = (OFF_CURVE, lanes[5][0][1])
    lanes[70][k - 1] = (OFF_CURVE, lanes[70][k - 1][1])
    pts, _ = pack(lanes, k)
    with pytest.raises(C12381Error) as e:
        ctx.g1_mul_sum(pts, sc, k, 96)
    assert e.value.code == E_POINT
    for fmt in (96, 49):
        got = ctx.g1_mul_sum(pts, sc, k, fmt, strict=False)
        want = expected(oracle_port, good_pts, sc, k, fmt)
        for i in range(n):
            assert got[fmt * i:fmt * i + fmt] == (b"\xff" * fmt if i in (5, 70) else want[fmt * i:fmt * i + fmt]), i
    got, rc = dev_call(ctx, pts, sc, k, 96)
    assert rc == E_POINT and got[96 * 5:96 * 6] == b"\xff" * 96 and got[96 * 6:96 * 70] == exp[96 * 6:96 * 70]
    assert ctx.g1_mul_sum(good_pts, sc, k, 96) == exp


def test_in_subgroup_flag_and_a_call_after_trim(ctx, oracle_port):
    """C12381_F_IN_SUBGROUP gives identical bytes on subgroup inputs, also for scalars below x^2 (whose [r]phi(P) terms it skips);
    c12381_trim releases the table slab and the next call rebuilds it"""
    from crypto12381_amd.capi import F_IN_SUBGROUP
    for k in (2, 4):
        lanes = seeded_lanes(oracle_port, k, 200, 9930 + k)
        for i in range(0, 200, 7):
            lanes[i][i % k] = (lanes[i][i % k][0], prng(9940, i) % (1 << 100))
        pts, sc = pack(lanes, k)
        exp = expected(oracle_port, pts, sc, k, 49)
        assert ctx.g1_mul_sum(pts, sc, k, 49) == exp
        assert ctx.g1_mul_sum(pts, sc, k, 49, F_IN_SUBGROUP) == exp
        ctx.trim()
        assert ctx.g1_mul_sum(pts, sc, k, 49) == exp
