"""c12381_ac_rps_redact_batch: tilde_H = tilde_M / prod_I tilde_Y[i]^a_i (the reference's examples/AC-rps/src/redact.cpp) from the wire formats, every
lane against tests/ac_rps_cases.expected_redact.  Lanes: valid, tilde_M at infinity, tilde_M outside G2, a leading 0x00 with bytes behind it, h or
sigma malformed (decoded though unused: 0xff), tilde_M malformed, a disclosed value >= r (0xff), a HIDDEN value >= r (never read: no effect); every
shape, nI = 0 (tilde_M re-encoded) and nattr = 32 included; keys: another key and back, a used tilde_Y outside G2 or at infinity, an undecodable
used record (every lane 0xff, C12381_E_POINT), an undecodable unused record (no effect); one tiled run of 2^12 + 1 lanes in host and _dev form."""
import pytest

import ac_rps_cases as rc
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


def lanes_of(op, key, I):
    """(kind, attr_all, sig) per lane"""
    creds = [rc.Cred(op, key, I, 6100, i) for i in range(3)]
    b = creds[0]
    out = [("valid", c.attr_all, c.sig) for c in creds]
    out.append(("tilde_M at infinity", b.attr_all, b.sig[:98] + bytes(97)))
    out.append(("tilde_M outside G2", b.attr_all, b.sig[:98] + rc.g2enc(op, rc.g2_outside())))
    out.append(("leading 00 + bytes", b.attr_all, b.sig[:98] + b"\x00" + bytes(range(1, 97))))
    out.append(("h bad tag", b.attr_all, b"\x05" + b.sig[1:]))
    out.append(("sigma off curve", b.attr_all, b.sig[:49] + rc.off_curve_x() + b.sig[98:]))
    out.append(("tilde_M tag 04", b.attr_all, b.sig[:98] + b"\x04" + b.sig[99:]))
    J = rc.hidden(key.nattr, I)
    if I:
        out.append(("disclosed a = r", rc._field(b.attr_all, I[-1], R), b.sig))
        out.append(("disclosed a = 0", rc._field(b.attr_all, I[0], 0), b.sig))
    if J:
        out.append(("hidden a = 2^384 - 1", rc._field(b.attr_all, J[0], (1 << 384) - 1), b.sig))
    return out


def check(ctx, op, key, I, lanes, **kw):
    attr, sig = b"".join(a for _, a, _ in lanes), b"".join(s for _, _, s in lanes)
    cache, st = ctx.ac_rps_redact(key.tY97, I, attr, sig, **kw)
    want = [rc.expected_redact(op, key.tY97, key.nattr, I, a, s) for _, a, s in lanes]
    bad = [(k, st[j], w[1]) for j, ((k, _, _), w) in enumerate(zip(lanes, want)) if (cache[97 * j:97 * j + 97], st[j]) != w]
    assert not bad, bad
    return {k: w[1] for (k, _, _), w in zip(lanes, want)}


@pytest.mark.parametrize("nattr,I", rc.SHAPES + rc.BIG_SHAPES)
def test_shapes(ctx, op, nattr, I):
    key = rc.Key(op, 5200 + nattr, nattr)
    by = check(ctx, op, key, I, lanes_of(op, key, I))
    assert by["valid"] == 0 and by["tilde_M outside G2"] == 0 and by["h bad tag"] == by["sigma off curve"] == by["tilde_M tag 04"] == 0xff
    assert by.get("disclosed a = r", 0xff) == 0xff and by.get("hidden a = 2^384 - 1", 0) == 0


def test_second_key_and_back_and_dev(ctx, op):
    key, other = rc.Key(op, 5000, rc.NATTR), rc.Key(op, 5001, rc.NATTR)
    lanes = lanes_of(op, key, rc.I_MAIN)
    check(ctx, op, key, rc.I_MAIN, lanes)
    check(ctx, op, other, rc.I_MAIN, lanes)
    check(ctx, op, key, rc.I_MAIN, lanes)
    check(ctx, op, key, rc.I_MAIN, lanes, dev=True)


@pytest.mark.parametrize("kind", ["used tilde_Y outside G2", "used tilde_Y at infinity"])
def test_generic_routes(ctx, op, kind):
    kw = {"used tilde_Y outside G2": dict(tilde_Y={0: rc.g2_outside()}), "used tilde_Y at infinity": dict(tilde_Y={3: bytes(192)})}[kind]
    key = rc.Key(op, 5600, rc.NATTR, **kw)
    check(ctx, op, key, rc.I_MAIN, lanes_of(op, key, rc.I_MAIN))


def test_undecodable_key_records(ctx, op):
    from types import SimpleNamespace
    from crypto12381_amd.capi import C12381Error, E_POINT
    key = rc.Key(op, 5000, rc.NATTR)
    lanes = lanes_of(op, key, rc.I_MAIN)
    attr, sig = b"".join(a for _, a, _ in lanes), b"".join(s for _, _, s in lanes)
    bad97 = b"\x04" + key.tY97[1:97]
    put = lambda k: key.tY97[:97 * k] + bad97 + key.tY97[97 * (k + 1):]
    for k in rc.I_MAIN:
        assert rc.expected_redact(op, put(k), rc.NATTR, rc.I_MAIN, lanes[0][1], lanes[0][2]) is None
        cache, st = ctx.ac_rps_redact(put(k), rc.I_MAIN, attr, sig, strict=False)
        assert st == b"\xff" * len(lanes) and cache == b"\xff" * (97 * len(lanes))
        with pytest.raises(C12381Error) as e:
            ctx.ac_rps_redact(put(k), rc.I_MAIN, attr, sig)
        assert e.value.code == E_POINT
        check(ctx, op, key, rc.I_MAIN, lanes[:3])
    for k in (1, 2, rc.NATTR):                                    # never read
        check(ctx, op, SimpleNamespace(tY97=put(k), nattr=rc.NATTR), rc.I_MAIN, lanes)


def test_large_tiled_host_and_dev(ctx, op):
    key = rc.Key(op, 5000, rc.NATTR)
    lanes = lanes_of(op, key, rc.I_MAIN)
    want = [rc.expected_redact(op, key.tY97, rc.NATTR, rc.I_MAIN, a, s) for _, a, s in lanes]
    n = (1 << 12) + 1
    idx = [(j * 37) % len(lanes) for j in range(n)]
    attr, sig = b"".join(lanes[i][1] for i in idx), b"".join(lanes[i][2] for i in idx)
    want_c, want_s = b"".join(want[i][0] for i in idx), bytes(want[i][1] for i in idx)
    assert ctx.ac_rps_redact(key.tY97, rc.I_MAIN, attr, sig) == (want_c, want_s)
    assert ctx.ac_rps_redact(key.tY97, rc.I_MAIN, attr, sig, dev=True) == (want_c, want_s)
