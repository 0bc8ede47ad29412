"""c12381_ps_verify_batch with more messages than the K-way product takes (C12381_FIXED_G2_MAX - 2 < nmsg <= C12381_G2_FIXED_SUM_MAX):
W_j = X2 + sum_i m_ij Y2_i is one per-lane sum over the shared bases Y2 (c12381_g2_mul_fixed_sum_batch_dev: nmsg tables for keys in G2,
its generic columns for any other key), then the pair_eq kernels.  Signatures are made as examples/ps/src/ps.cpp signs them (s1 = h,
s2 = h^(x + sum y_i m_i)); every lane is compared with the CPU oracle's pair_eq(s1, W, s2, g2), W formed with the oracle's g2_mul / g2_add."""
import pytest

from g2_fixed_sum_cases import G2GEN, b32, special_bases
from util import R, golden, prng

pytestmark = pytest.mark.gpu

OFF_CURVE = (1).to_bytes(48, "big") + (1).to_bytes(48, "big")
G1 = bytes.fromhex(golden("g1")["generator"])
N = 20


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


def _keys(orc, nmsg, seed=8800):
    x = prng(seed, 0) % R
    y = [prng(seed, 1 + i) % R for i in range(nmsg)]
    return x, y, orc.g2_mul(G2GEN, b32(x), 192, 1), orc.g2_mul(G2GEN * nmsg, b"".join(b32(v) for v in y), 192, 8)


def _expected(orc, g2, X2, Y2, s1, s2, m, n, invalid=()):
    """oracle: pair_eq(s1, W, s2, g2) with W = X2 + sum m_i Y2_i; lanes in `invalid` (a point off the curve) are 0xff"""
    nmsg = len(Y2) // 192
    W = X2 * n
    for i in range(nmsg):
        W = orc.g2_add(W, orc.g2_mul(Y2[192 * i:192 * i + 192] * n, m[32 * n * i:32 * n * (i + 1)], 192, 8), 192)
    good = [j for j in range(n) if j not in invalid]
    pick = lambda b, w: b"".join(b[w * j:w * j + w] for j in good)
    got = orc.pair_eq(pick(s1, 96), pick(W, 192), pick(s2, 96), g2 * len(good), 8)
    out = bytearray(b"\xff" * n)
    for t, j in enumerate(good):
        out[j] = got[t]
    return bytes(out)


KINDS = ["valid"] * 10 + ["wrong_msg", "wrong_msg_last", "m_zero", "m_r", "m_max", "m_mixed_edges", "s1_inf", "off_curve", "valid", "valid"]
assert len(KINDS) == N


def _batch(orc, nmsg, x, y, seed):
    """20 mixed lanes, signed for the keys (x, y): (s1, s2, m message-major, invalid lanes).  The edge-message lanes are signed for those
    messages, so they verify; a wrong message is changed after signing"""
    edges = [0, R, (1 << 256) - 1]
    msgs = []
    for j, kind in enumerate(KINDS):
        if kind == "m_zero":
            msgs.append([0] * nmsg)
        elif kind == "m_r":
            msgs.append([R] * nmsg)
        elif kind == "m_max":
            msgs.append([(1 << 256) - 1] * nmsg)
        elif kind == "m_mixed_edges":
            msgs.append([edges[i % 3] if i % 2 else prng(seed, 100 * j + i) % (1 << 256) for i in range(nmsg)])
        else:
            msgs.append([prng(seed, 100 * j + i) % R for i in range(nmsg)])
    hs = orc.g1_mul(G1 * N, b"".join(b32(prng(seed, 9000 + j) % R or 1) for j in range(N)), 96, 8)
    s2s = orc.g1_mul(hs, b"".join(b32((x + sum(a * b for a, b in zip(y, ms))) % R) for ms in msgs), 96, 8)
    s1l = [hs[96 * j:96 * j + 96] for j in range(N)]
    invalid = []
    for j, kind in enumerate(KINDS):
        if kind == "wrong_msg":
            msgs[j][0] = (msgs[j][0] + 1) % R
        elif kind == "wrong_msg_last":
            msgs[j][nmsg - 1] = (msgs[j][nmsg - 1] + 1) % R
        elif kind == "s1_inf":
            s1l[j] = bytes(96)
        elif kind == "off_curve":
            s1l[j] = OFF_CURVE
            invalid.append(j)
    m = b"".join(b32(msgs[j][i]) for i in range(nmsg) for j in range(N))
    return b"".join(s1l), s2s, m, invalid


def _check(ctx, orc, X2, Y2, s1, s2, m, invalid, keys_in_g2):
    from crypto12381_amd.capi import C12381Error, E_POINT
    want = _expected(orc, G2GEN, X2, Y2, s1, s2, m, N, invalid)
    got = ctx.ps_verify(G2GEN, X2, Y2, s1, s2, m, strict=False)
    assert got == want, [(KINDS[j], got[j], want[j]) for j in range(N) if got[j] != want[j]]
    assert [got[j] for j in invalid] == [0xff] * len(invalid) and got.count(0xff) == len(invalid)      # 0xff in that lane only
    if keys_in_g2:
        for j, kind in enumerate(KINDS):
            if kind in ("valid", "m_zero", "m_r", "m_max", "m_mixed_edges"):
                assert got[j] == 1, (kind, j)
            elif kind.startswith("wrong_msg"):
                assert got[j] == 0, (kind, j)
    with pytest.raises(C12381Error) as e:
        ctx.ps_verify(G2GEN, X2, Y2, s1, s2, m)                 # the off-curve lane: C12381_E_POINT
    assert e.value.code == E_POINT
    return got


@pytest.mark.parametrize("nmsg", [8, 12])
def test_ps_verify_many_messages(ctx, oracle_port, nmsg):
    x, y, X2, Y2 = _keys(oracle_port, nmsg)
    s1, s2, m, invalid = _batch(oracle_port, nmsg, x, y, 8810 + nmsg)
    _check(ctx, oracle_port, X2, Y2, s1, s2, m, invalid, True)


@pytest.mark.parametrize("nmsg", [8, 12])
@pytest.mark.parametrize("case", ["Y2_off_g2", "X2_inf"])
def test_ps_verify_many_messages_generic_keys(ctx, oracle_port, nmsg, case):
    """one Y2 outside G2 (G + T13, a twist point of order 13 r) sends the sum through its generic columns; X2 at infinity is an addend like any
    other: the oracle's verdicts either way"""
    x, y, X2, Y2 = _keys(oracle_port, nmsg)
    s1, s2, m, invalid = _batch(oracle_port, nmsg, x, y, 8830 + nmsg)
    if case == "Y2_off_g2":
        pos = nmsg // 2
        Y2 = Y2[:192 * pos] + dict(special_bases())["g+t13"] + Y2[192 * (pos + 1):]
    else:
        X2 = bytes(192)
    got = _check(ctx, oracle_port, X2, Y2, s1, s2, m, invalid, False)
    assert 0 in got


def test_ps_verify_many_messages_key_off_twist(ctx, oracle_port):
    """an off-twist public point poisons every lane and returns C12381_E_POINT, as for few messages"""
    from crypto12381_amd.capi import C12381Error, E_POINT
    nmsg = 8
    x, y, X2, Y2 = _keys(oracle_port, nmsg)
    s1, s2, m, invalid = _batch(oracle_port, nmsg, x, y, 8850)
    flip = lambda b, at: b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]
    for X2b, Y2b in ((flip(X2, 191), Y2), (X2, flip(Y2, 191)), (X2, flip(Y2, 192 * nmsg - 1))):
        assert ctx.ps_verify(G2GEN, X2b, Y2b, s1, s2, m, strict=False) == b"\xff" * N
        with pytest.raises(C12381Error) as e:
            ctx.ps_verify(G2GEN, X2b, Y2b, s1, s2, m)
        assert e.value.code == E_POINT
    keep = [j for j in range(N) if j not in invalid]
    sub = lambda b, w: b"".join(b[w * j:w * j + w] for j in keep)
    msub = b"".join(m[32 * (i * N + j):32 * (i * N + j) + 32] for i in range(nmsg) for j in keep)
    want = _expected(oracle_port, G2GEN, X2, Y2, s1, s2, m, N, invalid)
    assert ctx.ps_verify(G2GEN, X2, Y2, sub(s1, 96), sub(s2, 96), msub) == bytes(want[j] for j in keep)      # the next clean call is right


@pytest.mark.parametrize("nmsg", [8, 12])
def test_ps_verify_many_messages_host_equals_dev(ctx, oracle_port, nmsg):
    import torch
    from crypto12381_amd.capi import E_POINT
    x, y, X2, Y2 = _keys(oracle_port, nmsg)
    s1, s2, m, invalid = _batch(oracle_port, nmsg, x, y, 8860 + nmsg)
    host = ctx.ps_verify(G2GEN, X2, Y2, s1, s2, m, strict=False)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    t = [dev(b) for b in (G2GEN, X2, Y2, s1, s2, m)]
    ok = torch.full((N,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.ps_verify_dev(N, nmsg, *[v.data_ptr() for v in t], ok.data_ptr())
    assert ctx.sync() == E_POINT
    assert bytes(ok.cpu().numpy()) == host
    assert host == _expected(oracle_port, G2GEN, X2, Y2, s1, s2, m, N, invalid)
