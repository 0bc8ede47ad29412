"""c12381_ac_rps_pres_batch: presentations (the reference's examples/AC-rps/src/pres.cpp) from the wire formats with the caller's randomness, every
byte of every lane against tests/ac_rps_cases.expected_pres.  Lanes: valid, r = 0 (sigma1_ at infinity), t = 0, rho = 0, z = 0, randomness >= r and
2^256 - 1, h at infinity, h / sigma plus an order-3 point and an eigenpoint, tilde_H and tilde_M outside G2, a leading 0x00 with bytes behind it,
x >= p, malformed h, sigma, tilde_M (decoded though unused), tilde_H, z >= r, a disclosed and a hidden attribute >= r (0xff and a record of 0xff);
every shape pres takes — nI = 8 with its spilling tail and J = {8}, J empty, nattr = 10 — keys: another key and back, g or a Y outside G1,
tilde_g outside G2, an undecodable g / tilde_g / tilde_X / ANY Y record (every lane 0xff, C12381_E_POINT); one tiled run of 2^12 + 1 lanes in host
and _dev form."""
import pytest

import ac_rps_cases as rc
from g1_torsion import P as FP, enc as enc96, eigenpoint, point_of_order
from util import R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def op(oracle_port):
    return rc.Ops(oracle_port)


def L(kind, c, **kw):
    d = dict(attr=c.attr_all, sig=c.sig, cache=c.cache, usk=c.usk, rnd=c.rnd96)
    d.update(kw)
    return (kind, d)


def lanes_of(op, key, I, full=False):
    creds = [rc.Cred(op, key, I, 6200, i) for i in range(2)]
    b = creds[0]
    rnd = lambda r, t, rho: b"".join(v.to_bytes(32, "big") for v in (r, t, rho))
    out = [L("valid", c) for c in creds]
    out.append(L("r = 0", b, rnd=rnd(0, b.rnd[1], b.rnd[2])))
    out.append(L("t = 0, rho = r", b, rnd=rnd(b.rnd[0], 0, R)))
    out.append(L("hidden or disclosed a = r", b, attr=rc._field(b.attr_all, key.nattr - 1, R)))
    if not full:
        return out
    z0 = rc.Cred(op, key, I, 6200, 0, z=0)
    out.append(L("z = 0", z0))
    out.append(L("randomness 2^256 - 1, r + 5, r", b, rnd=rnd((1 << 256) - 1, R + 5, R)))
    out.append(L("h at infinity", b, sig=bytes(49) + b.sig[49:]))
    t3, te = enc96(point_of_order(3)), enc96(eigenpoint(10177)[0])
    h, sg = op.dec(b.sig[:49])[0], op.dec(b.sig[49:98])[0]
    out.append(L("h + order 3", b, sig=op.enc(op.add(h, t3)) + b.sig[49:]))
    out.append(L("sigma + eigenpoint", b, sig=b.sig[:49] + op.enc(op.add(sg, te)) + b.sig[98:]))
    out.append(L("tilde_H outside G2", b, cache=rc.g2enc(op, rc.g2_outside())))
    out.append(L("tilde_M outside G2", b, sig=b.sig[:98] + rc.g2enc(op, rc.g2_outside())))
    out.append(L("leading 00 + bytes", b, sig=b"\x00" + bytes(range(1, 49)) + b.sig[49:], cache=b"\x00" + bytes(range(3, 99))))
    x_big = int.from_bytes(b.sig[1:49], "big") + FP
    out.append(L("x >= p", b, sig=b.sig[:1] + x_big.to_bytes(48, "big") + b.sig[49:]))
    out.append(L("h bad tag", b, sig=b"\x05" + b.sig[1:]))
    out.append(L("sigma off curve", b, sig=b.sig[:49] + rc.off_curve_x() + b.sig[98:]))
    out.append(L("tilde_M tag 04", b, sig=b.sig[:98] + b"\x04" + b.sig[99:]))
    out.append(L("tilde_H tag 04", b, cache=b"\x04" + b.cache[1:]))
    out.append(L("z = r", b, usk=R.to_bytes(48, "big")))
    out.append(L("a_0 = 2^384 - 1", b, attr=rc._field(b.attr_all, 0, (1 << 384) - 1)))
    return out


def pack(lanes):
    return [b"".join(d[f] for _, d in lanes) for f in ("attr", "sig", "cache", "usk", "rnd")]


def want_of(op, key, I, lanes):
    return [rc.expected_pres(op, key.pk, key.Y49, key.nattr, I, d["attr"], d["sig"], d["cache"], d["usk"], d["rnd"]) for _, d in lanes]


def check(ctx, op, key, I, lanes, **kw):
    pres, st = ctx.ac_rps_pres(key.pk, key.Y49, I, *pack(lanes), **kw)
    want = want_of(op, key, I, lanes)
    bad = [(k, st[j], w[1]) for j, ((k, _), w) in enumerate(zip(lanes, want)) if (pres[389 * j:389 * j + 389], st[j]) != w]
    assert not bad, bad
    return {k: w[1] for (k, _), w in zip(lanes, want)}


def test_main_shape(ctx, op):
    key = rc.Key(op, 5000, rc.NATTR)
    by = check(ctx, op, key, rc.I_MAIN, lanes_of(op, key, rc.I_MAIN, full=True))
    bad = ("hidden or disclosed a = r", "h bad tag", "sigma off curve", "tilde_M tag 04", "tilde_H tag 04", "z = r", "a_0 = 2^384 - 1")
    assert all(v == (0xff if k in bad else 0) for k, v in by.items()), by


@pytest.mark.parametrize("nattr,I", rc.SHAPES)
def test_shapes(ctx, op, nattr, I):
    key = rc.Key(op, 5200 + nattr, nattr)
    by = check(ctx, op, key, I, lanes_of(op, key, I))
    assert by["valid"] == 0 and by["r = 0"] == 0 and by["hidden or disclosed a = r"] == 0xff


def test_second_key_and_back_and_dev(ctx, op):
    key, other = rc.Key(op, 5000, rc.NATTR), rc.Key(op, 5001, rc.NATTR)
    lanes = lanes_of(op, key, rc.I_MAIN)
    check(ctx, op, key, rc.I_MAIN, lanes)
    check(ctx, op, other, rc.I_MAIN, lanes)
    check(ctx, op, key, rc.I_MAIN, lanes)
    check(ctx, op, key, rc.I_MAIN, lanes, dev=True)


@pytest.mark.parametrize("kind", ["g outside G1", "a fixed Y outside G1", "a cross Y outside G1", "tilde_g outside G2"])
def test_generic_routes(ctx, op, kind):
    t3 = enc96(point_of_order(3))
    base = rc.Key(op, 5600, rc.NATTR)
    kw = {"g outside G1": dict(g=op.add(base.g, t3)), "a fixed Y outside G1": dict(Y={1: op.add(base.Y[1], t3)}),
          "a cross Y outside G1": dict(Y={7: op.add(base.Y[7], t3)}), "tilde_g outside G2": dict(tilde_g=rc.g2_outside())}[kind]
    key = rc.Key(op, 5600, rc.NATTR, **kw)
    check(ctx, op, key, rc.I_MAIN, lanes_of(op, key, rc.I_MAIN))


def test_undecodable_key_records(ctx, op):
    """pres materialises pk.Y: ANY record, used by the sum or not, fails the call"""
    from types import SimpleNamespace
    from crypto12381_amd.capi import C12381Error, E_POINT
    key = rc.Key(op, 5000, rc.NATTR)
    lanes = lanes_of(op, key, rc.I_MAIN)
    bad49 = rc.off_curve_x()
    put = lambda k: key.Y49[:49 * k] + bad49 + key.Y49[49 * (k + 1):]
    bads = [(b"\x05" + key.pk[1:], key.Y49), (key.pk[:49] + b"\x04" + key.pk[50:], key.Y49), (key.pk[:146] + b"\x04" + key.pk[147:], key.Y49)]
    bads += [(key.pk, put(k)) for k in (0, 5, 8)]                 # Y[5] and Y[8] are in neither part of the list for I = (0, 3)
    assert 5 not in [rc.NATTR - i for i in rc.I_MAIN] + [0] + [k for k, _ in rc.cross_terms(rc.NATTR, rc.I_MAIN, [1] * 4, [1] * 3)]
    for pk, Y in bads:
        bad = SimpleNamespace(pk=pk, Y49=Y, nattr=rc.NATTR)
        assert want_of(op, bad, rc.I_MAIN, lanes[:1]) == [None]
        pres, st = ctx.ac_rps_pres(pk, Y, rc.I_MAIN, *pack(lanes), strict=False)
        assert st == b"\xff" * len(lanes) and pres == b"\xff" * (389 * len(lanes))
        with pytest.raises(C12381Error) as e:
            ctx.ac_rps_pres(pk, Y, rc.I_MAIN, *pack(lanes))
        assert e.value.code == E_POINT
        check(ctx, op, key, rc.I_MAIN, lanes[:2])


def test_large_tiled_host_and_dev(ctx, op):
    key = rc.Key(op, 5000, rc.NATTR)
    lanes = lanes_of(op, key, rc.I_MAIN, full=True)
    want = want_of(op, key, rc.I_MAIN, lanes)
    n = (1 << 12) + 1
    idx = [(j * 37) % len(lanes) for j in range(n)]
    tiled = [lanes[i] for i in idx]
    want_p, want_s = b"".join(want[i][0] for i in idx), bytes(want[i][1] for i in idx)
    assert ctx.ac_rps_pres(key.pk, key.Y49, rc.I_MAIN, *pack(tiled)) == (want_p, want_s)
    assert ctx.ac_rps_pres(key.pk, key.Y49, rc.I_MAIN, *pack(tiled), dev=True) == (want_p, want_s)
