"""c12381_ps_verify_aggregate: ONE verdict for a PS batch by a random linear combination,
  e(-sum rho_j σ2_j, g2) e(sum rho_j σ1_j, X2) prod_i e(sum_j (rho_j m_ij) σ1_j, Y2_i) == 1.
Signatures are made with Python integers and the CPU oracle's multiply (ps_cases.py), so which lanes are valid is known by construction; the
per-signature entry c12381_ps_verify_batch — itself tested against the oracle's pair_eq in test_gpu_ps_verify.py — gives the lane verdicts the
aggregate has to agree with.  rho: 128-bit values from the seeded prng, so every result is deterministic."""
import ctypes

import pytest

from g1_torsion import dec, ec_add, ec_neg, enc
from ps_cases import G1, T3, Keys, b32, rec, sign_points
from util import R, cat, golden, prng

pytestmark = pytest.mark.gpu

OFF_CURVE = (1).to_bytes(48, "big") + (1).to_bytes(48, "big")


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


_batches = {}


def batch(orc, nmsg, n):
    """(keys, s1, s2, m message-major) of n valid signatures, made once per shape"""
    if (nmsg, n) not in _batches:
        keys = Keys(orc, nmsg, 9900 + nmsg)
        ms = [[prng(9910 + nmsg, 100 * j + i, 32) for i in range(nmsg)] for j in range(n)]           # any value below 2^256, used as given
        s1, s2 = sign_points(orc, keys, ms, [1 + prng(9920, j) % (R - 1) for j in range(n)])
        m = b"".join(b32(ms[j][i]) for i in range(nmsg) for j in range(n))
        _batches[(nmsg, n)] = (keys, s1, s2, m)
    return _batches[(nmsg, n)]


def rhos(seed, n):
    return b"".join(b32(1 + prng(seed, j, 16)) for j in range(n))


def put(b, w, j, v):
    return b[:w * j] + v + b[w * (j + 1):]


def agree(ctx, keys, s1, s2, m, rho, want):
    """the verdict is `want` and equals all(ok == 1) of the per-signature entry"""
    ok = ctx.ps_verify(keys.g2, keys.X2, keys.Y2, s1, s2, m)
    assert all(v == 1 for v in ok) == want
    assert ctx.ps_verify_aggregate(keys.g2, keys.X2, keys.Y2, s1, s2, m, rho) == want


@pytest.mark.parametrize("n", [1, 65, 200])
@pytest.mark.parametrize("nmsg", [0, 1, 3, 6])
def test_valid_and_forged(ctx, oracle_port, nmsg, n):
    keys, s1, s2, m = batch(oracle_port, nmsg, n)
    rho = rhos(9930, n)
    agree(ctx, keys, s1, s2, m, rho, True)
    j = n // 2
    forged = put(s2, 96, j, rec(s1, 96, j))                        # σ2 = σ1: valid only for e = 1
    agree(ctx, keys, s1, forged, m, rho, False)
    if nmsg:
        agree(ctx, keys, s1, s2, put(m, 32, (nmsg - 1) * n + j, b32(5)), rho, False)                 # another message in the last column
    agree(ctx, keys, put(s1, 96, n - 1, rec(s2, 96, n - 1)), s2, m, rho, False)


def test_points_outside_g1_and_infinity(ctx, oracle_port):
    """lanes the per-signature entry accepts although a point lies outside G1 (an order-3 component pairs to 1 against G2) or both points are
    at infinity: the aggregate accepts them too, whatever the GLV form of the bucket products adds off the subgroup"""
    nmsg, n = 3, 65
    keys, s1, s2, m = batch(oracle_port, nmsg, n)
    s1 = put(s1, 96, 3, enc(ec_add(dec(rec(s1, 96, 3)), T3)))
    s2 = put(s2, 96, 4, enc(ec_add(dec(rec(s2, 96, 4)), T3)))
    s1, s2 = put(s1, 96, 5, bytes(96)), put(s2, 96, 5, bytes(96))
    agree(ctx, keys, s1, s2, m, rhos(9931, n), True)
    agree(ctx, keys, put(s1, 96, 6, bytes(96)), s2, m, rhos(9931, n), False)                         # σ1 at infinity alone


@pytest.mark.parametrize("nmsg", [0, 3])
def test_cancelling_tampers_need_distinct_rho(ctx, oracle_port, nmsg):
    """σ2_a + D and σ2_b - D: the plain product over the batch is unchanged, so rho = 1 everywhere accepts; distinct rho do not — rho enters"""
    n = 65
    keys, s1, s2, m = batch(oracle_port, nmsg, n)
    D = dec(oracle_port.g1_mul(G1, b32(prng(9940, 0) % R), 96, 1))
    a, b = 7, 40
    t = put(s2, 96, a, enc(ec_add(dec(rec(s2, 96, a)), D)))
    t = put(t, 96, b, enc(ec_add(dec(rec(t, 96, b)), ec_neg(D))))
    ok = ctx.ps_verify(keys.g2, keys.X2, keys.Y2, s1, t, m)
    assert [j for j in range(n) if ok[j] != 1] == [a, b]
    assert ctx.ps_verify_aggregate(keys.g2, keys.X2, keys.Y2, s1, t, m, b32(1) * n) is True
    assert ctx.ps_verify_aggregate(keys.g2, keys.X2, keys.Y2, s1, t, m, rhos(9941, n)) is False
    assert ctx.ps_verify_aggregate(keys.g2, keys.X2, keys.Y2, s1, s2, m, b32(1) * n) is True


@pytest.mark.parametrize("which", ["g2", "X2", "Y2", "Y2_inf"])
def test_key_outside_g2_gives_0(ctx, oracle_port, which):
    nmsg, n = 3, 65
    keys, s1, s2, m = batch(oracle_port, nmsg, n)
    off = cat(golden("g2")["offsubgroup_points"])[:192]
    g2, X2, Y2 = keys.g2, keys.X2, keys.Y2
    if which == "g2":
        g2 = off
    elif which == "X2":
        X2 = off
    else:
        Y2 = put(Y2, 192, 1, off if which == "Y2" else bytes(192))
    assert ctx.ps_verify_aggregate(g2, X2, Y2, s1, s2, m, rhos(9950, n)) is False
    assert ctx.ps_verify_aggregate(keys.g2, keys.X2, keys.Y2, s1, s2, m, rhos(9950, n)) is True      # the tables of the good keys come back


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("col", ["s1", "s2"])
def test_point_off_curve(ctx, oracle_port, n, col):
    from crypto12381_amd.capi import C12381Error, E_POINT
    nmsg = 1
    keys, s1, s2, m = batch(oracle_port, nmsg, n)
    if col == "s1":
        s1 = put(s1, 96, n - 1, OFF_CURVE)
    else:
        s2 = put(s2, 96, n - 1, OFF_CURVE)
    assert ctx.ps_verify_aggregate(keys.g2, keys.X2, keys.Y2, s1, s2, m, rhos(9960, n), strict=False) is False
    with pytest.raises(C12381Error) as e:
        ctx.ps_verify_aggregate(keys.g2, keys.X2, keys.Y2, s1, s2, m, rhos(9960, n))
    assert e.value.code == E_POINT


def test_off_curve_lane_cannot_hide(ctx, oracle_port):
    """σ1 off the curve beside σ2 at infinity: the bucket products leave the bad point out and what remains multiplies to 1 — the verdict is 0
    all the same, in the _dev form too"""
    import torch
    from crypto12381_amd.capi import E_POINT
    keys, s1, s2, m = batch(oracle_port, 0, 1)
    assert ctx.ps_verify_aggregate(keys.g2, keys.X2, b"", OFF_CURVE, bytes(96), b"", b32(3), strict=False) is False
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    t = [dev(b) for b in (keys.g2, keys.X2, OFF_CURVE, bytes(96), b32(3))]
    verdict = torch.full((1,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.ps_verify_aggregate_dev(1, 0, t[0].data_ptr(), t[1].data_ptr(), None, t[2].data_ptr(), t[3].data_ptr(), None, t[4].data_ptr(), verdict.data_ptr())
    assert ctx.sync() == E_POINT
    assert bytes(verdict.cpu().numpy()) == b"\x00"


def test_dev_equals_host(ctx, oracle_port):
    import torch
    nmsg, n = 6, 200
    keys, s1, s2, m = batch(oracle_port, nmsg, n)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    forged = put(s2, 96, 17, rec(s1, 96, 17))
    for col, want in ((s2, 1), (forged, 0)):
        t = [dev(b) for b in (keys.g2, keys.X2, keys.Y2, s1, col, m, rhos(9970, n))]
        verdict = torch.full((1,), 0x5a, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.ps_verify_aggregate_dev(n, nmsg, *[v.data_ptr() for v in t], verdict.data_ptr())
        assert ctx.sync() == 0
        assert bytes(verdict.cpu().numpy()) == bytes([want])


def test_arguments_and_empty_batch(ctx, oracle_port):
    from crypto12381_amd.capi import E_ARG
    n = 65
    keys, s1, s2, m = batch(oracle_port, 3, n)
    rho = rhos(9980, n)
    f = ctx.lib.c12381_ps_verify_aggregate
    out = ctypes.c_int(0x5a)
    k7 = Keys(oracle_port, 7, 9981)
    assert f(ctx.h, n, 7, k7.g2, k7.X2, k7.Y2, s1, s2, m + bytes(32 * 4 * n), rho, ctypes.byref(out)) == E_ARG       # nmsg + 2 > C12381_FIXED_G2_MAX
    assert f(ctx.h, 0, 7, k7.g2, k7.X2, k7.Y2, None, None, None, None, ctypes.byref(out)) == E_ARG
    good = [keys.g2, keys.X2, keys.Y2, s1, s2, m, rho]
    for i in range(7):
        a = list(good)
        a[i] = None
        assert f(ctx.h, n, 3, *a, ctypes.byref(out)) == E_ARG, i
    assert f(ctx.h, n, 3, *good, None) == E_ARG
    assert out.value == 0x5a
    assert f(ctx.h, 0, 3, keys.g2, keys.X2, keys.Y2, None, None, None, None, ctypes.byref(out)) == 0 and out.value == 1      # n = 0 gives 1
    assert ctx.ps_verify_aggregate(keys.g2, keys.X2, b"", b"", b"", b"", b"") is True
    assert f(ctx.h, n, 3, *good, ctypes.byref(out)) == 0 and out.value == 1
