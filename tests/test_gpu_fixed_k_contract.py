"""Argument contract of the two K-way fixed-G2 entry families (c12381_pair_product_fixed_g2_batch[_dev], c12381_ps_verify_batch[_dev]):
argument errors, the empty batch, host form equals _dev form, and the _dev status reported through c12381_sync."""
import ctypes

import pytest

from util import R, golden, prng

pytestmark = pytest.mark.gpu

G1 = bytes.fromhex(golden("g1")["generator"])
G2 = bytes.fromhex(golden("g2")["generator"])
OFF_CURVE = (1).to_bytes(48, "big") + (1).to_bytes(48, "big")


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pts(ctx):
    sc = b"".join((prng(7301, i) % R).to_bytes(32, "big") for i in range(40))
    return ctx.g1_mul(G1 * 32, sc[:32 * 32], 96), ctx.g2_mul(G2 * 8, sc[32 * 32:], 192)


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def test_product_argument_errors(ctx, pts):
    from crypto12381_amd.capi import E_ARG, _p
    p, q = pts
    out = ctypes.create_string_buffer(576 * 4)
    for name in ("c12381_pair_product_fixed_g2_batch", "c12381_pair_product_fixed_g2_batch_dev"):
        f = getattr(ctx.lib, name)
        assert f(ctx.h, 4, 0, _p(p), _p(q), _p(out), 0) == E_ARG                # k = 0
        assert f(ctx.h, 4, 9, _p(p), _p(q), _p(out), 0) == E_ARG                # k > C12381_FIXED_G2_MAX
        assert f(ctx.h, 4, 2, _p(p), _p(q), _p(out), 1) == E_ARG                # unknown flag bits
        assert f(ctx.h, 4, 2, _p(p), _p(q), _p(out), 4) == E_ARG
        assert f(ctx.h, 4, 2, None, _p(q), _p(out), 0) == E_ARG
        assert f(ctx.h, 4, 2, _p(p), None, _p(out), 0) == E_ARG
        assert f(ctx.h, 4, 2, _p(p), _p(q), None, 0) == E_ARG
        assert f(None, 4, 2, _p(p), _p(q), _p(out), 0) == E_ARG
        assert f(ctx.h, 0, 0, _p(p), _p(q), _p(out), 0) == E_ARG                # checks before the empty-batch rule


def test_ps_argument_errors(ctx, pts):
    from crypto12381_amd.capi import E_ARG, _p
    p, q = pts
    ok = ctypes.create_string_buffer(4)
    sc = b"\x01" * 128
    for name in ("c12381_ps_verify_batch", "c12381_ps_verify_batch_dev"):
        f = getattr(ctx.lib, name)
        args = [_p(q), _p(q), _p(q), _p(p), _p(p), _p(sc), _p(ok)]
        for i in range(7):
            a = list(args)
            a[i] = None
            want = 0 if i in (2, 5) else E_ARG
            rc = f(ctx.h, 0, 0, *a)                          # nmsg = 0: Y2 and m may be null
            assert rc == want, (name, i, rc)
            if i in (2, 5):
                assert f(ctx.h, 4, 1, *a) == E_ARG            # but not with messages
        assert f(None, 4, 1, *args) == E_ARG


def test_empty_batches_leave_outputs(ctx, pts):
    from crypto12381_amd.capi import _p
    p, q = pts
    out = ctypes.create_string_buffer(b"\xab" * 64, 64)
    assert ctx.lib.c12381_pair_product_fixed_g2_batch(ctx.h, 0, 3, _p(p), _p(q), _p(out), 0) == 0
    assert ctx.lib.c12381_pair_product_fixed_g2_batch_dev(ctx.h, 0, 3, _p(p), _p(q), _p(out), 0) == 0
    assert ctx.lib.c12381_ps_verify_batch(ctx.h, 0, 1, _p(q), _p(q), _p(q), _p(p), _p(p), _p(p), _p(out)) == 0
    assert ctx.lib.c12381_ps_verify_batch_dev(ctx.h, 0, 1, _p(q), _p(q), _p(q), _p(p), _p(p), _p(p), _p(out)) == 0
    assert out.raw == b"\xab" * 64
    assert ctx.sync() == 0


def test_product_host_equals_dev(ctx, pts):
    import torch
    from crypto12381_amd.capi import E_POINT, F_MILLER_ONLY
    p, q = pts
    n, k = 10, 3
    g1s = bytearray(p[:96 * n * k])
    g1s[96 * 4:96 * 5] = OFF_CURVE                          # one lane off the curve
    g1s = bytes(g1s)
    for flags in (0, F_MILLER_ONLY):
        host = ctx.pair_product_fixed_g2(g1s, q[:192 * k], k, flags=flags, strict=False)
        a, b = _dev(g1s), _dev(q[:192 * k])
        out = torch.zeros(576 * n, dtype=torch.uint8, device="cuda")
        ctx.pair_product_fixed_g2_dev(n, k, a.data_ptr(), b.data_ptr(), out.data_ptr(), flags)
        assert ctx.sync() == E_POINT
        assert bytes(out.cpu().numpy()) == host
        assert host[576 * 4:576 * 5] == b"\xff" * 576
    # a clean batch: status 0 through c12381_sync
    out = torch.zeros(576 * n, dtype=torch.uint8, device="cuda")
    a = _dev(p[:96 * n * k])
    ctx.pair_product_fixed_g2_dev(n, k, a.data_ptr(), _dev(q[:192 * k]).data_ptr(), out.data_ptr())
    assert ctx.sync() == 0
    assert bytes(out.cpu().numpy()) == ctx.pair_product_fixed_g2(p[:96 * n * k], q[:192 * k], k)


def test_ps_dev_status_through_sync(ctx, pts):
    import torch
    from crypto12381_amd.capi import E_POINT
    p, q = pts
    n = 6
    s1 = bytearray(p[:96 * n])
    s1[96 * 2:96 * 3] = OFF_CURVE
    s1 = bytes(s1)
    m = b"\x00" * 31 + b"\x05"
    m = m * n
    host = ctx.ps_verify(q[:192], q[192:384], q[384:576], s1, p[96 * n:192 * n], m, strict=False)
    assert host[2] == 0xff
    t = [_dev(b) for b in (q[:192], q[192:384], q[384:576], s1, p[96 * n:192 * n], m)]
    ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ctx.ps_verify_dev(n, 1, *[v.data_ptr() for v in t], ok.data_ptr())
    assert ctx.sync() == E_POINT
    assert bytes(ok.cpu().numpy()) == host
    assert ctx.sync() == 0                                  # the status was collected once
