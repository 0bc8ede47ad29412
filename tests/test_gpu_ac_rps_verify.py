"""c12381_ac_rps_verify_batch: AC-rps presentations (the reference's examples/AC-rps/src/verify.cpp) from the wire formats.  Keys, credentials, caches
and presentations are made by tests/ac_rps_cases.py as keygen, user_keygen, issue, redact and pres make them; the expected byte of every lane is
verify composed independently from the CPU oracle's primitives.  Lanes: valid, every field of PresInfo tampered, each equation and the c0 check
failing alone, a wrong c0 in front of a disclosed value >= r, sigma1_ at infinity (r = 0), t = 0, z = 0, a leading 0x00 with bytes behind it, x >= p,
order-3 and eigenpoint additions to sigma1_, sigma3_, C, tilde_sigma_ and tilde_H outside G2, malformed points and Zp fields >= r (0xff); shapes: I
empty, I = all, I unordered, nattr = 1, 2, 9 (nI = 8: the spilling tail), 10, 32; keys: another key and back, g / a used Y outside G1, tilde_g /
tilde_X / a used tilde_Y / tilde_Y[nattr] outside G2, an undecodable used record (every lane 0xff, C12381_E_POINT), an undecodable unused record
(no effect); the entries chained: redact -> pres -> verify; one tiled run of 2^12 + 1 lanes in host and _dev form."""
from types import SimpleNamespace

import pytest

import ac_rps_cases as rc
from g1_torsion import enc as enc96, point_of_order

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


@pytest.fixture(scope="module")
def main(op):
    key = rc.Key(op, 5000, rc.NATTR)
    lanes = rc.main_lanes(op, key)
    return key, lanes, rc.expect(op, key, rc.I_MAIN, lanes)


def run(ctx, key, I, lanes, **kw):
    pres, attr = rc.pack(lanes)
    return ctx.ac_rps_verify(key.pk, key.Y49, key.tY97, I, pres, attr, **kw)


def check(ctx, op, key, I, lanes):
    got, want = run(ctx, key, I, lanes), rc.expect(op, key, I, lanes)
    bad = [(ln.kind, g, w) for ln, g, w in zip(lanes, got, want) if g != w]
    assert not bad, bad
    return want


def test_main_shape(ctx, main):
    key, lanes, want = main
    got = run(ctx, key, rc.I_MAIN, lanes)
    bad = [(ln.kind, g, w) for ln, g, w in zip(lanes, got, want) if g != w]
    assert not bad, bad
    by = {ln.kind: w for ln, w in zip(lanes, want)}
    assert all(by[k] == 1 for k in rc.ONE_KINDS) and all(by[k] == 0 for k in rc.ZERO_KINDS) and all(by[k] == 0xff for k in rc.BAD_KINDS)
    assert by["c0 wrong and a = r"] == 0 and by["a = r"] == 0xff


@pytest.mark.parametrize("nattr,I", rc.SHAPES + rc.BIG_SHAPES)
def test_shapes(ctx, op, nattr, I):
    key = rc.Key(op, 5200 + nattr, nattr)
    lanes = rc.valid_lanes(op, key, I, 3, 5300)
    lanes.append(rc._with(lanes[0], "s0+1", pres389=rc._plus1(lanes[0].pres, 1, 293)))
    lanes.append(rc._with(lanes[1], "sigma2_ swapped", pres389=rc._pt(lanes[1].pres, "sigma2_", rc._get(lanes[2].pres, "sigma2_"))))
    if I:
        lanes.append(rc._with(lanes[1], "a+1", attr48=rc._plus1(lanes[1].attr, len(I) - 1)))
    want = check(ctx, op, key, I, lanes)
    assert want[:3] == b"\x01\x01\x01" and set(want[3:]) == {0}


def test_unordered_I_is_not_sorted(ctx, op):
    """attr_48 follows the order of idx, and so does the hashed prefix of the q_k"""
    key = rc.Key(op, 5204, 4)
    lanes = rc.valid_lanes(op, key, (3, 0), 2, 5300)
    assert run(ctx, key, (3, 0), lanes) == b"\x01\x01"
    assert run(ctx, key, (0, 3), lanes) == rc.expect(op, key, (0, 3), lanes) == b"\x00\x00"
    swapped = [rc._with(ln, "swapped", attr48=ln.attr[48:] + ln.attr[:48]) for ln in lanes]
    assert run(ctx, key, (0, 3), swapped) == rc.expect(op, key, (0, 3), swapped) == b"\x00\x00"      # W agrees, the q_k do not


def test_second_key_and_back(ctx, op, main):
    key, lanes, want = main
    other = rc.Key(op, 5001, rc.NATTR)
    assert set(check(ctx, op, other, rc.I_MAIN, lanes[:3])) == {0}
    assert run(ctx, key, rc.I_MAIN, lanes[:3]) == want[:3] == b"\x01" * 3


@pytest.mark.parametrize("kind", ["g outside G1", "used Y outside G1", "Y[0] outside G1", "tilde_g outside G2", "tilde_X outside G2",
                                  "used tilde_Y outside G2", "tilde_Y[nattr] outside G2", "used tilde_Y at infinity"])
def test_generic_routes(ctx, op, kind):
    """key points outside the subgroups: the fixed-base sums fall back to the generic kernels and the line tables serve any point of the twist; the
    credentials are made under that key with the oracle's multiply, and the verdicts are expected_verify's whatever they are"""
    t3 = enc96(point_of_order(3))
    base = rc.Key(op, 5600, rc.NATTR)
    kw = {"g outside G1": dict(g=op.add(base.g, t3)), "used Y outside G1": dict(Y={rc.NATTR: op.add(base.Y[rc.NATTR], t3)}),
          "Y[0] outside G1": dict(Y={0: op.add(base.Y[0], t3)}), "tilde_g outside G2": dict(tilde_g=rc.g2_outside()),
          "tilde_X outside G2": dict(tilde_X=rc.g2_outside()), "used tilde_Y outside G2": dict(tilde_Y={0: rc.g2_outside()}),
          "tilde_Y[nattr] outside G2": dict(tilde_Y={rc.NATTR: rc.g2_outside()}), "used tilde_Y at infinity": dict(tilde_Y={3: bytes(192)})}[kind]
    key = rc.Key(op, 5600, rc.NATTR, **kw)
    lanes = rc.valid_lanes(op, key, rc.I_MAIN, 3, 5700)
    lanes.append(rc._with(lanes[0], "sigma3_ swapped", pres389=rc._pt(lanes[0].pres, "sigma3_", rc._get(lanes[1].pres, "sigma3_"))))
    lanes.append(rc._with(lanes[1], "C swapped", pres389=rc._pt(lanes[1].pres, "C", rc._get(lanes[2].pres, "C"))))
    check(ctx, op, key, rc.I_MAIN, lanes)


def _put(b, k, rec):
    return b[:len(rec) * k] + rec + b[len(rec) * (k + 1):]


def test_undecodable_key_records(ctx, op, main):
    """a used record: every lane 0xff, C12381_E_POINT, the context usable afterwards; a record verify never reads: no effect"""
    from crypto12381_amd.capi import C12381Error, E_POINT
    key, lanes, want = main
    n = rc.NATTR
    bad49, bad97 = rc.off_curve_x(), b"\x04" + key.tY97[1:97]
    used = [(b"\x05" + key.pk[1:], key.Y49, key.tY97), (key.pk[:49] + b"\x04" + key.pk[50:], key.Y49, key.tY97),
            (key.pk[:146] + b"\x04" + key.pk[147:], key.Y49, key.tY97), (key.pk, _put(key.Y49, n - 3, bad49), key.tY97), (key.pk, _put(key.Y49, 0, bad49), key.tY97),
            (key.pk, key.Y49, _put(key.tY97, 0, bad97)), (key.pk, key.Y49, _put(key.tY97, n, bad97))]
    for pk, Y, tY in used:
        bad = SimpleNamespace(pk=pk, Y49=Y, tY97=tY)
        assert rc.expected_verify(op, pk, Y, tY, n, rc.I_MAIN, lanes[0].pres, lanes[0].attr) is None
        assert run(ctx, bad, rc.I_MAIN, lanes[:5], strict=False) == b"\xff" * 5
        with pytest.raises(C12381Error) as e:
            run(ctx, bad, rc.I_MAIN, lanes[:5])
        assert e.value.code == E_POINT
        assert run(ctx, key, rc.I_MAIN, lanes[:2]) == b"\x01\x01"
    Y, tY = key.Y49, key.tY97
    for k in (2, 3, 5, 6, 7, 8):                                  # used: Y[4], Y[1], Y[0]
        Y = _put(Y, k, bad49)
    for k in (1, 2):
        tY = _put(tY, k, bad97)
    unused = SimpleNamespace(pk=key.pk, Y49=Y, tY97=tY)
    assert run(ctx, unused, rc.I_MAIN, lanes) == want


@pytest.mark.parametrize("nattr,I", rc.SHAPES)
def test_chain_through_the_entries(ctx, op, nattr, I):
    """the entry's redact output feeds the entry's pres and that feeds the entry's verify: all 1"""
    key = rc.Key(op, 5900 + nattr, nattr)
    creds = [rc.Cred(op, key, I, 6000, i) for i in range(3)]
    cat = lambda f: b"".join(getattr(c, f) for c in creds)
    cache, st = ctx.ac_rps_redact(key.tY97, I, cat("attr_all"), cat("sig"))
    assert st == bytes(3) and cache == cat("cache")
    pres, st = ctx.ac_rps_pres(key.pk, key.Y49, I, cat("attr_all"), cat("sig"), cache, cat("usk"), cat("rnd96"))
    assert st == bytes(3)
    assert ctx.ac_rps_verify(key.pk, key.Y49, key.tY97, I, pres, cat("attr")) == b"\x01" * 3


def test_large_tiled_host_and_dev(ctx, main):
    key, lanes, want_d = main
    n = (1 << 12) + 1
    idx = [(j * 37) % len(lanes) for j in range(n)]
    tiled = [lanes[i] for i in idx]
    want = bytes(want_d[i] for i in idx)
    assert run(ctx, key, rc.I_MAIN, tiled) == want
    assert run(ctx, key, rc.I_MAIN, tiled, dev=True) == want
