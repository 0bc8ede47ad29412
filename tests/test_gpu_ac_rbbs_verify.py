"""c12381_ac_rbbs_verify_batch: AC-rbbs presentations (the reference's examples/AC-rbbs/src/verify.cpp) from the wire formats.  Keys, credentials,
caches and presentations are made by tests/ac_rbbs_cases.py as keygen, issue, redact and pres make them; the expected byte of every lane is verify
composed independently from the CPU oracle's primitives.  Lanes: valid, every field of PresInfo tampered, each of the three equations failing
alone, A at infinity, r = 0, a leading 0x00 with bytes behind it, x >= p, order-3 and eigenpoint additions to A_, C_J_, D_, malformed points and
Zp fields >= r (0xff); shapes: I empty, I = all, I unordered, nattr = 1, 2, 16, 32 with nI + 1 = 3, 8 (the product over line tables) and 9 (the
G2 sum and pair_eq); keys: another key and back, g / a used Y_i outside G1, tilde_g / tilde_X / a used tilde_Y outside G2 (the generic routes),
an undecodable used record (every lane 0xff, C12381_E_POINT), an undecodable unused record (no effect); the entries chained: redact -> pres ->
verify; one tiled run of 2^12 + 1 lanes in host and _dev form and a second chunk."""
from types import SimpleNamespace

import pytest

import ac_rbbs_cases as rc
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


def run(ctx, key, I, lanes, msg_len=rc.MSG_LEN, **kw):
    pres, attr, msgs = rc.pack(lanes)
    return ctx.ac_rbbs_verify(key.pk, key.Y49, key.tY97, I, pres, attr, msgs, msg_len, **kw)


def check(ctx, op, key, I, lanes, msg_len=rc.MSG_LEN):
    got, want = run(ctx, key, I, lanes, msg_len), rc.expect(op, key, I, lanes)
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
    assert by["A at infinity"] == 0


@pytest.mark.parametrize("nattr,I,msg_len", [(n, I, 32) for n, I in rc.SHAPES + rc.VERIFY_ONLY_SHAPES + [rc.SUM_SHAPE]] + [(4, (0, 3), 0), (4, (0, 3), 43)])
def test_shapes(ctx, op, nattr, I, msg_len):
    key = rc.Key(op, 5200 + nattr, nattr)
    lanes = rc.valid_lanes(op, key, I, 3, 5300, msg_len)
    lanes.append(rc._with(lanes[0], "s+1", pres341=rc._plus1(lanes[0].pres, 0, 245)))
    lanes.append(rc._with(lanes[1], "D_ swapped", pres341=rc._pt(lanes[1].pres, 3, lanes[2].pres[147:196])))
    if I:
        lanes.append(rc._with(lanes[1], "a+1", attr48=rc._plus1(lanes[1].attr, len(I) - 1)))
    want = check(ctx, op, key, I, lanes, msg_len)
    assert want[:4] == b"\x01\x01\x01\x00" and (want[4] == 0 or not I or len(I) == nattr) and set(want[5:]) <= {0}


def test_unordered_I_is_not_sorted(ctx, op):
    """attr_48 follows the order of idx, and so does the hashed prefix of the q_i"""
    key = rc.Key(op, 5204, 4)
    lanes = rc.valid_lanes(op, key, (3, 0), 2, 5300)
    assert run(ctx, key, (3, 0), lanes) == b"\x01\x01"
    assert run(ctx, key, (0, 3), lanes) == rc.expect(op, key, (0, 3), lanes) == b"\x00\x00"
    swapped = [rc._with(ln, "swapped", attr48=ln.attr[48:] + ln.attr[:48]) for ln in lanes]
    assert run(ctx, key, (0, 3), swapped) == rc.expect(op, key, (0, 3), swapped) == b"\x00\x00"      # K agrees, the q_i do not


def test_second_key_and_back(ctx, op, main):
    key, lanes, want = main
    other = rc.Key(op, 5001, rc.NATTR)
    assert set(check(ctx, op, other, rc.I_MAIN, lanes[:6])) == {0}
    assert run(ctx, key, rc.I_MAIN, lanes[:6]) == want[:6] == b"\x01" * 6


@pytest.mark.parametrize("kind", ["g outside G1", "used Y outside G1", "tilde_g outside G2", "tilde_X outside G2", "used tilde_Y outside G2",
                                  "used tilde_Y at infinity"])
def test_generic_routes(ctx, op, kind):
    """key points outside the subgroups: the fixed-base sum falls back to the generic kernel, each pairing equation to pair_eq; the credentials are
    made under that key with the oracle's multiply, and the verdicts are expected_verify's whatever they are"""
    t3 = enc96(point_of_order(3))
    base = rc.Key(op, 5600, rc.NATTR)
    kw = {"g outside G1": dict(g=op.add(base.g, t3)), "used Y outside G1": dict(Y={0: op.add(base.Y[0], t3)}),
          "tilde_g outside G2": dict(tilde_g=rc.g2_outside()), "tilde_X outside G2": dict(tilde_X=rc.g2_outside()),
          "used tilde_Y outside G2": dict(tilde_Y={0: rc.g2_outside()}), "used tilde_Y at infinity": dict(tilde_Y={3: bytes(192)})}[kind]
    key = rc.Key(op, 5600, rc.NATTR, **kw)
    lanes = rc.valid_lanes(op, key, rc.I_MAIN, 3, 5700)
    lanes.append(rc._with(lanes[0], "t+1", pres341=rc._plus1(lanes[0].pres, 1, 245)))
    lanes.append(rc._with(lanes[1], "C_J_ swapped", pres341=rc._pt(lanes[1].pres, 2, lanes[2].pres[98:147])))
    check(ctx, op, key, rc.I_MAIN, lanes)


def _put(b, k, rec):
    return b[:len(rec) * k] + rec + b[len(rec) * (k + 1):]


def test_undecodable_key_records(ctx, op, main):
    """a used record: every lane 0xff, C12381_E_POINT, the context usable afterwards; a record verify never reads: no effect"""
    from crypto12381_amd.capi import C12381Error, E_POINT
    key, lanes, want = main
    bad49, bad97 = rc.off_curve_x(), b"\x04" + key.tY97[1:97]
    used = [(b"\x05" + key.pk[1:], key.Y49, key.tY97), (key.pk[:49] + b"\x04" + key.pk[50:], key.Y49, key.tY97),
            (key.pk[:146] + b"\x04" + key.pk[147:], key.Y49, key.tY97), (key.pk, _put(key.Y49, 3, bad49), key.tY97), (key.pk, key.Y49, _put(key.tY97, 0, bad97))]
    for pk, Y, tY in used:
        bad = SimpleNamespace(pk=pk, Y49=Y, tY97=tY)
        assert rc.expected_verify(op, pk, Y, tY, rc.NATTR, rc.I_MAIN, lanes[0].pres, lanes[0].attr, lanes[0].msg) is None
        assert run(ctx, bad, rc.I_MAIN, lanes[:5], strict=False) == b"\xff" * 5
        with pytest.raises(C12381Error) as e:
            run(ctx, bad, rc.I_MAIN, lanes[:5])
        assert e.value.code == E_POINT
        assert run(ctx, key, rc.I_MAIN, lanes[:2]) == b"\x01\x01"
    Y, tY = key.Y49, key.tY97
    for k in (1, 2, 4, 5, 6, 7):
        Y = _put(Y, k, bad49)
    for k in (1, 2):
        tY = _put(tY, k, bad97)
    unused = SimpleNamespace(pk=key.pk, Y49=Y, tY97=tY)
    assert run(ctx, unused, rc.I_MAIN, lanes) == want


@pytest.mark.parametrize("nattr,I", [(4, (0, 3)), (4, (3, 0)), (4, ()), (4, (0, 1, 2, 3)), (16, (0, 3)), (1, (0,)), (2, (1,))])
def test_chain_through_the_entries(ctx, op, nattr, I):
    """the entry's redact output feeds the entry's pres and that feeds the entry's verify: all 1"""
    key = rc.Key(op, 5900 + nattr, nattr)
    creds = [rc.Cred(op, key, I, 6000, i) for i in range(3)]
    cache, st = ctx.ac_rbbs_redact(key.pk, key.Y49, I, b"".join(c.attr_all for c in creds), b"".join(c.sig for c in creds))
    assert st == bytes(3) and cache == b"".join(c.cache for c in creds)
    rnd = b"".join(v.to_bytes(32, "big") for c in creds for v in c.rnd)
    pres, st = ctx.ac_rbbs_pres(b"".join(c.sig for c in creds), cache, b"".join(c.msg for c in creds), rnd, rc.MSG_LEN)
    assert st == bytes(3)
    assert ctx.ac_rbbs_verify(key.pk, key.Y49, key.tY97, I, pres, b"".join(c.attr for c in creds), b"".join(c.msg for c in creds), rc.MSG_LEN) == b"\x01" * 3


def test_large_tiled_host_and_dev(ctx, op, main):
    import torch
    key, lanes, want_d = main
    n = (1 << 12) + 1
    idx = [(j * 37) % len(lanes) for j in range(n)]
    tiled = [lanes[i] for i in idx]
    want = bytes(want_d[i] for i in idx)
    pres, attr, msgs = rc.pack(tiled)
    host = ctx.ac_rbbs_verify(key.pk, key.Y49, key.tY97, rc.I_MAIN, pres, attr, msgs, rc.MSG_LEN)
    assert host == want
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    d = [dev(b) for b in (key.pk, key.Y49, key.tY97, pres, attr, msgs)]
    d_ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.ac_rbbs_verify_dev(n, rc.NATTR, rc.I_MAIN, rc.MSG_LEN, *(t.data_ptr() for t in d), d_ok.data_ptr())
    assert ctx.sync() == 0
    assert bytes(d_ok.cpu().numpy().tobytes()) == host


def test_second_chunk(ctx, main):
    """2^18 + 3 lanes: the batch runs in chunks of 2^18, and the second chunk reads and writes behind the first"""
    key, lanes, want_d = main
    n, m = (1 << 18) + 3, len(lanes)
    rep = lambda b, width: b * (n // m) + b[:width * (n % m)]
    pres, attr, msgs = rc.pack(lanes)
    got = ctx.ac_rbbs_verify(key.pk, key.Y49, key.tY97, rc.I_MAIN, rep(pres, 341), rep(attr, 96), rep(msgs, rc.MSG_LEN), rc.MSG_LEN)
    assert got == rep(want_d, 1)
