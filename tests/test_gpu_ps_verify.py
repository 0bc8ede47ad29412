"""c12381_ps_verify_batch: ok[j] = [ e(s1_j, X2 + sum_i m_ij Y2_i) == e(s2_j, g2) ] (the reference's examples/ps/src/ps.cpp:84-99).
Signatures are made as ps.cpp signs them (s1 = h, s2 = h^(x + sum y_i m_i)); every lane is compared with the CPU oracle's
pair_eq(s1, W, s2, g2), W formed with the oracle's g2_mul / g2_add.  The fast route (one (nmsg + 2)-way product over line tables) serves
nmsg = 0, 1, 3, 6 with keys in G2; nmsg = 7, keys outside G2 or at infinity take the generic route.  Edge lanes: signatures at infinity,
outside G1 (order-3 and eigenpoint components), scalars 0, r, r + 1, 2^256 - 1, W = infinity, a point off the curve."""
import pytest

from g1_torsion import dec, ec_add, eigenpoint, enc
from util import R, cat, golden, prng

pytestmark = pytest.mark.gpu

OFF_CURVE = (1).to_bytes(48, "big") + (1).to_bytes(48, "big")
G1 = bytes.fromhex(golden("g1")["generator"])
G2 = bytes.fromhex(golden("g2")["generator"])
T3 = (0, 2)                                        # a point of order 3


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


def _b(k):
    return (k % (1 << 256)).to_bytes(32, "big")


def _keys(orc, nmsg, seed=8100):
    x = prng(seed, 0) % R
    y = [prng(seed, 1 + i) % R for i in range(nmsg)]
    X2 = orc.g2_mul(G2, _b(x), 192, 1)
    Y2 = b"".join(orc.g2_mul(G2, _b(yi), 192, 1) for yi in y)
    return x, y, X2, Y2


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


def _batch(orc, nmsg, x, y, seed):
    """mixed lanes: (s1, s2, m message-major, kinds, invalid lanes)"""
    te, _ = eigenpoint(10177)
    rows = []                                                   # (kind, msgs, s1 point / bytes, exponent override / s2 bytes)
    n_valid = 8
    for j in range(n_valid):
        rows.append(("valid", [prng(seed, 100 * j + i) % R for i in range(nmsg)]))
    rows += [("wrong_msg", None), ("swapped", None), ("s2_twice", None), ("s1_inf", None), ("both_inf", None), ("s1_t3", None),
             ("s1_eigen", None), ("s2_t3", None), ("m_zero", [0] * nmsg), ("m_r", [R] * nmsg), ("m_r1", [R + 1] * nmsg),
             ("m_max", [(1 << 256) - 1] * nmsg), ("s1_t3_m_r1", [R + 1] * nmsg), ("off_curve", None)]
    if nmsg == 1:
        rows.append(("w_inf", [(-x * pow(y[0], -1, R)) % R]))
    n = len(rows)
    msgs = [r[1] if r[1] is not None else [prng(seed, 7000 + 10 * j + i) % R for i in range(nmsg)] for j, r in enumerate(rows)]
    hs = orc.g1_mul(G1 * n, b"".join(_b(prng(seed, 9000 + j) % R) for j in range(n)), 96, 8)
    exps = [(x + sum(yi * mi for yi, mi in zip(y, ms))) % R for ms in msgs]
    s2s = orc.g1_mul(hs, b"".join(_b(e) for e in exps), 96, 8)
    s1l = [hs[96 * j:96 * j + 96] for j in range(n)]
    s2l = [s2s[96 * j:96 * j + 96] for j in range(n)]
    invalid = []
    for j, (kind, _) in enumerate(rows):
        if kind == "wrong_msg":
            msgs[j] = [msgs[j][0] + 1] + msgs[j][1:] if nmsg else msgs[j]
            if not nmsg:
                s2l[j] = s1l[j]
        elif kind == "swapped":
            s1l[j], s2l[j] = s2l[j], s1l[j]
        elif kind == "s2_twice":
            s2l[j] = enc(ec_add(dec(s2l[j]), dec(s2l[j])))
        elif kind == "s1_inf":
            s1l[j] = bytes(96)
        elif kind == "both_inf":
            s1l[j] = s2l[j] = bytes(96)
        elif kind in ("s1_t3", "s1_t3_m_r1"):
            s1l[j] = enc(ec_add(dec(s1l[j]), T3))
        elif kind == "s1_eigen":
            s1l[j] = enc(ec_add(dec(s1l[j]), te))
        elif kind == "s2_t3":
            s2l[j] = enc(ec_add(dec(s2l[j]), T3))
        elif kind == "off_curve":
            s1l[j] = OFF_CURVE
            invalid.append(j)
    m = b"".join(_b(msgs[j][i]) for i in range(nmsg) for j in range(n))
    return b"".join(s1l), b"".join(s2l), m, [r[0] for r in rows], invalid


@pytest.mark.parametrize("nmsg", [0, 1, 3, 6, 7])
def test_ps_verify_mixed_lanes(ctx, oracle_port, nmsg):
    from crypto12381_amd.capi import C12381Error
    x, y, X2, Y2 = _keys(oracle_port, nmsg)
    s1, s2, m, kinds, invalid = _batch(oracle_port, nmsg, x, y, 8200 + nmsg)
    n = len(kinds)
    want = _expected(oracle_port, G2, X2, Y2, s1, s2, m, n, invalid)
    got = ctx.ps_verify(G2, X2, Y2, s1, s2, m, strict=False)
    assert got == want, [(kinds[j], got[j], want[j]) for j in range(n) if got[j] != want[j]]
    assert [got[j] for j in range(n) if kinds[j] == "valid"] == [1] * 8
    assert got[kinds.index("wrong_msg")] == 0 and got[kinds.index("off_curve")] == 0xff
    with pytest.raises(C12381Error):
        ctx.ps_verify(G2, X2, Y2, s1, s2, m)                   # the off-curve lane: C12381_E_POINT
    keep = [j for j in range(n) if j not in invalid]
    sub = lambda b, w: b"".join(b[w * j:w * j + w] for j in keep)
    msub = b"".join(m[32 * (i * n + j):32 * (i * n + j) + 32] for i in range(nmsg) for j in keep)
    assert ctx.ps_verify(G2, X2, Y2, sub(s1, 96), sub(s2, 96), msub) == bytes(want[j] for j in keep)


@pytest.mark.parametrize("case", ["X2_off_g2", "Y2_off_g2", "Y2_inf", "X2_inf", "g2_off_g2"])
def test_ps_verify_generic_keys(ctx, oracle_port, case):
    """public points outside G2 or at infinity: the generic route, same booleans as the oracle"""
    nmsg = 2
    x, y, X2, Y2 = _keys(oracle_port, nmsg, 8300)
    off = cat(golden("g2")["offsubgroup_points"])[:192]
    g2 = G2
    if case == "X2_off_g2":
        X2 = off
    elif case == "Y2_off_g2":
        Y2 = Y2[:192] + off
    elif case == "Y2_inf":
        Y2 = bytes(192) + Y2[192:]
    elif case == "X2_inf":
        X2 = bytes(192)
    else:
        g2 = off
    s1, s2, m, kinds, invalid = _batch(oracle_port, nmsg, x, y, 8400)
    n = len(kinds)
    assert ctx.ps_verify(g2, X2, Y2, s1, s2, m, strict=False) == _expected(oracle_port, g2, X2, Y2, s1, s2, m, n, invalid)


def test_ps_verify_key_off_twist(ctx, oracle_port):
    from crypto12381_amd.capi import C12381Error
    nmsg = 1
    x, y, X2, Y2 = _keys(oracle_port, nmsg)
    s1, s2, m, kinds, invalid = _batch(oracle_port, nmsg, x, y, 8500)
    n = len(kinds)
    for which in range(3):
        keys = [G2, X2, Y2]
        keys[which] = keys[which][:191] + bytes([keys[which][191] ^ 1])
        assert ctx.ps_verify(keys[0], keys[1], keys[2], s1, s2, m, strict=False) == b"\xff" * n
        with pytest.raises(C12381Error):
            ctx.ps_verify(keys[0], keys[1], keys[2], s1, s2, m)


@pytest.mark.parametrize("nmsg", [1, 7])
def test_ps_verify_host_equals_dev(ctx, oracle_port, nmsg):
    import torch
    from crypto12381_amd.capi import E_POINT
    x, y, X2, Y2 = _keys(oracle_port, nmsg)
    s1, s2, m, kinds, invalid = _batch(oracle_port, nmsg, x, y, 8600)
    n = len(kinds)
    host = ctx.ps_verify(G2, X2, Y2, s1, s2, m, strict=False)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    t = [dev(b) for b in (G2, X2, Y2, s1, s2, m)]
    ok = torch.full((n,), 0x5a, dtype=torch.uint8, device="cuda")
    ctx.ps_verify_dev(n, nmsg, *[v.data_ptr() for v in t], ok.data_ptr())
    assert ctx.sync() == E_POINT
    assert bytes(ok.cpu().numpy()) == host


def test_ps_verify_large_batch(ctx, oracle_port):
    """n = 2^16 valid signatures (made on the device): every lane 1, a seeded sample against the oracle"""
    n, nmsg = 1 << 16, 3
    x, y, X2, Y2 = _keys(oracle_port, nmsg, 8700)
    m = b"".join(_b(prng(8702, i * n + j) % (1 << 256)) for i in range(nmsg) for j in range(n))
    ints = [[int.from_bytes(m[32 * (i * n + j):32 * (i * n + j) + 32], "big") for i in range(nmsg)] for j in range(n)]
    hs = ctx.g1_mul(G1 * n, b"".join(_b(prng(8703, j) % R) for j in range(n)), 96)
    s2 = ctx.g1_mul(hs, b"".join(_b((x + sum(yi * mi for yi, mi in zip(y, ints[j]))) % R) for j in range(n)), 96)
    got = ctx.ps_verify(G2, X2, Y2, hs, s2, m)
    assert got == b"\x01" * n
    # a sample, with some lanes broken, against the oracle
    idx = sorted({prng(8704, i) % n for i in range(24)})
    s1s = b"".join(hs[96 * j:96 * j + 96] for j in idx)
    s2s = b"".join((s2 if t % 3 else hs)[96 * j:96 * j + 96] for t, j in enumerate(idx))
    msub = b"".join(m[32 * (i * n + j):32 * (i * n + j) + 32] for i in range(nmsg) for j in idx)
    want = _expected(oracle_port, G2, X2, Y2, s1s, s2s, msub, len(idx))
    assert ctx.ps_verify(G2, X2, Y2, s1s, s2s, msub) == want
    assert 0 in want and 1 in want
