"""c12381_ac_bbs_verify_batch: AC-bbs presentations (the reference's examples/AC-bbs/src/verify.cpp) from the wire formats.  Keys, credentials and
presentations are made by tests/ac_bbs_cases.py as keygen, issue and pres make them; the expected byte of every lane is verify composed
independently from the CPU oracle's primitives, with multiply(B_, c) on the left side (the entry evaluates multiply(-B_, c) on the right).
Lanes: valid, tampered in every field, each half failing alone, A at infinity, r = 0, a leading 0x00 with bytes behind it, x >= p, points
outside G1 (order 3, eigenpoint), malformed points and Zp fields >= r (0xff); shapes: I empty, I = all, I unordered, nattr = 1, nattr = 32, empty
messages; keys: another key, g / Y_i outside G1 and tilde_X outside G2 (the generic routes), an undecodable key (every lane 0xff,
C12381_E_POINT); one tiled run of 2^12 + 1 lanes in host and _dev form."""
from types import SimpleNamespace

import pytest

import ac_bbs_cases as ac
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
    return ac.Ops(oracle_port)


@pytest.fixture(scope="module")
def main(op):
    key = ac.Key(op, 5000, ac.NATTR)
    lanes = ac.main_lanes(op, key)
    return key, lanes, ac.expect(op, key, ac.I_MAIN, lanes)


def run(ctx, key, I, lanes, msg_len=ac.MSG_LEN, **kw):
    pres, u, attr, msgs = ac.pack(lanes)
    return ctx.ac_bbs_verify(key.pk, key.Y49, I, pres, u, attr, msgs, msg_len, **kw)


def check(ctx, op, key, I, lanes, msg_len=ac.MSG_LEN):
    got, want = run(ctx, key, I, lanes, msg_len), ac.expect(op, key, I, lanes)
    bad = [(ln.kind, g, w) for ln, g, w in zip(lanes, got, want) if g != w]
    assert not bad, bad
    return want


def test_main_shape(ctx, main):
    key, lanes, want = main
    got = run(ctx, key, ac.I_MAIN, lanes)
    bad = [(ln.kind, g, w) for ln, g, w in zip(lanes, got, want) if g != w]
    assert not bad, bad
    by = {ln.kind: w for ln, w in zip(lanes, want)}
    assert sum(1 for ln, w in zip(lanes, want) if ln.kind == "valid" and w == 1) == 12
    assert all(by[k] == 0 for k in ac.ZERO_KINDS) and all(by[k] == 0xff for k in ac.BAD_KINDS)
    assert by["r = 0"] == by["leading 00 + bytes"] == by["x >= p"] == 1           # re-encoded points hash like the parsed ones
    assert by["B_ + order 3"] == by["A_ eigenpoint"] == by["A at infinity"] == 0


@pytest.mark.parametrize("nattr,I,msg_len", [(4, (), 32), (4, (0, 1, 2, 3), 32), (4, (3, 0), 32), (1, (), 32), (1, (0,), 32), (32, (0, 3), 32), (4, (0, 3), 0)])
def test_further_shapes(ctx, op, nattr, I, msg_len):
    key = ac.Key(op, 5200 + nattr, nattr)
    lanes = ac.valid_lanes(op, key, I, 3, 5300, msg_len)
    lanes.append(ac._with(lanes[0], "s+1", pres243=ac._plus1(lanes[0].pres, 0, 147)))
    if I:
        lanes.append(ac._with(lanes[1], "a+1", attr48=ac._plus1(lanes[1].attr, len(I) - 1)))
    if len(I) < nattr:
        lanes.append(ac._with(lanes[2], "u+1", u48=ac._plus1(lanes[2].u, nattr - len(I) - 1)))
    want = check(ctx, op, key, I, lanes, msg_len)
    assert want[:4] == b"\x01\x01\x01\x00" and set(want[4:]) <= {0}


def test_unordered_I_is_not_sorted(ctx, op):
    """attr_48 follows the order of idx: the values of I = (3, 0) offered under I = (0, 3) are the wrong way round"""
    key = ac.Key(op, 5204, 4)
    lanes = ac.valid_lanes(op, key, (3, 0), 2, 5300)
    assert run(ctx, key, (3, 0), lanes) == b"\x01\x01"
    assert run(ctx, key, (0, 3), lanes) == ac.expect(op, key, (0, 3), lanes) == b"\x00\x00"
    swapped = [ac._with(ln, "swapped", attr48=ln.attr[48:] + ln.attr[:48]) for ln in lanes]
    assert run(ctx, key, (0, 3), swapped) == b"\x01\x01"


def test_second_key_and_back(ctx, op, main):
    """every lane fails under another key; the first key's tables are rebuilt when it returns"""
    key, lanes, want = main
    other = ac.Key(op, 5001, ac.NATTR)
    assert set(check(ctx, op, other, ac.I_MAIN, lanes[:12])) == {0}
    assert run(ctx, key, ac.I_MAIN, lanes[:12]) == want[:12] == b"\x01" * 12


@pytest.mark.parametrize("kind", ["g outside G1", "disclosed Y outside G1", "hidden Y outside G1", "hidden Y at infinity", "tilde_X outside G2"])
def test_generic_routes(ctx, op, kind):
    """key points outside the subgroups: the fixed-base sums fall back to the generic kernel, the pairing half to the generic pairing; the
    presentations are made under that key with the oracle's multiply, and the verdicts are expected_verify's whatever they are"""
    t3 = enc96(point_of_order(3))
    base = ac.Key(op, 5600, ac.NATTR)
    kw = {"g outside G1": dict(g=op.add(base.g, t3)), "disclosed Y outside G1": dict(Y={0: op.add(base.Y[0], t3)}),
          "hidden Y outside G1": dict(Y={2: op.add(base.Y[2], t3)}), "hidden Y at infinity": dict(Y={1: bytes(96)}),
          "tilde_X outside G2": dict(tilde_X=ac.g2_outside())}[kind]
    key = ac.Key(op, 5600, ac.NATTR, **kw)
    lanes = ac.valid_lanes(op, key, ac.I_MAIN, 4, 5700)
    lanes.append(ac._with(lanes[0], "t+1", pres243=ac._plus1(lanes[0].pres, 1, 147)))
    lanes.append(ac._with(lanes[1], "u1+1", u48=ac._plus1(lanes[1].u, 1)))
    want = check(ctx, op, key, ac.I_MAIN, lanes)
    if kind == "hidden Y at infinity":
        assert want[:4] == b"\x01" * 4


def test_undecodable_key(ctx, op, main):
    from crypto12381_amd.capi import C12381Error, E_POINT
    key, lanes, want = main
    for pk, Y in ((b"\x05" + key.pk[1:], key.Y49), (key.pk[:49] + b"\x04" + key.pk[50:], key.Y49), (key.pk, key.Y49[:98] + ac.off_curve_x() + key.Y49[147:])):
        bad = SimpleNamespace(pk=pk, Y49=Y)
        assert ac.expected_verify(op, pk, Y, ac.I_MAIN, lanes[0].pres, lanes[0].u, lanes[0].attr, lanes[0].msg) is None
        assert run(ctx, bad, ac.I_MAIN, lanes[:5], strict=False) == b"\xff" * 5
        with pytest.raises(C12381Error) as e:
            run(ctx, bad, ac.I_MAIN, lanes[:5])
        assert e.value.code == E_POINT
        assert run(ctx, key, ac.I_MAIN, lanes[:2]) == b"\x01\x01"                  # the context recovers


def test_large_tiled_host_and_dev(ctx, op, main):
    import torch
    key, lanes, want_d = main
    distinct = list(lanes) + ac.valid_lanes(op, key, ac.I_MAIN, 64 - len(lanes), 5800)
    want_d = want_d + b"\x01" * (64 - len(lanes))
    assert ac.expect(op, key, ac.I_MAIN, distinct[len(lanes):]) == want_d[len(lanes):]
    n = (1 << 12) + 1
    idx = [(j * 37) % 64 for j in range(n)]
    tiled = [distinct[i] for i in idx]
    want = bytes(want_d[i] for i in idx)
    pres, u, attr, msgs = ac.pack(tiled)
    host = ctx.ac_bbs_verify(key.pk, key.Y49, ac.I_MAIN, pres, u, attr, msgs, ac.MSG_LEN)
    assert host == want
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    d = [dev(b) for b in (key.pk, key.Y49, pres, u, attr, msgs)]
    d_ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.ac_bbs_verify_dev(n, ac.NATTR, ac.I_MAIN, ac.MSG_LEN, *(t.data_ptr() for t in d), d_ok.data_ptr())
    assert ctx.sync() == 0
    assert bytes(d_ok.cpu().numpy().tobytes()) == host


def test_second_chunk(ctx, op, main):
    """2^18 + 3 lanes: the batch runs in chunks of 2^18, and the second chunk reads and writes behind the first"""
    key, lanes, want_d = main
    n, m = (1 << 18) + 3, len(lanes)
    rep = lambda b, width: b * (n // m) + b[:width * (n % m)]
    pres, u, attr, msgs = ac.pack(lanes)
    got = ctx.ac_bbs_verify(key.pk, key.Y49, ac.I_MAIN, rep(pres, 243), rep(u, 96), rep(attr, 96), rep(msgs, ac.MSG_LEN), ac.MSG_LEN)
    assert got == rep(want_d, 1)
