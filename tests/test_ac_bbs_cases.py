"""CPU test of the AC-bbs builders (tests/ac_bbs_cases.py) against themselves, so that the GPU tests cannot hide behind a wrong oracle: every
presentation `pres` makes verifies under `expected_verify` (which puts op.mul(B_, c) on the left side, as verify.cpp writes it), every tampered
lane is rejected, every malformed lane is where the reference would throw, on the main shape and on the further shapes of the GPU tests;
`expected_pres` marks what parse would refuse and agrees with `pres` elsewhere."""
import pytest

import ac_bbs_cases as ac
from util import R


@pytest.fixture(scope="module")
def op(oracle_port):
    return ac.Ops(oracle_port)


@pytest.fixture(scope="module")
def main(op):
    key = ac.Key(op, 5000, ac.NATTR)
    lanes = ac.main_lanes(op, key)
    return key, lanes, ac.expect(op, key, ac.I_MAIN, lanes)


def test_every_valid_lane_verifies(main):
    key, lanes, want = main
    got = [w for ln, w in zip(lanes, want) if ln.kind in ac.VALID_KINDS]
    assert len(got) == 12 and set(got) == {1}


def test_every_tampered_lane_is_rejected(main):
    key, lanes, want = main
    by = {ln.kind: w for ln, w in zip(lanes, want)}
    for kind in ac.ZERO_KINDS:
        assert by[kind] == 0, kind


def test_every_malformed_lane_throws(main):
    key, lanes, want = main
    by = {ln.kind: w for ln, w in zip(lanes, want)}
    for kind in ac.BAD_KINDS:
        assert by[kind] == 0xff, kind


def test_degenerate_lanes(main):
    """r = 0 makes A_ and B_ infinity: both halves hold trivially; a leading 0x00 with bytes behind it and an x >= p are the same points and
    hash alike; A at infinity fails the pairing half; the off-subgroup lanes are rejected"""
    key, lanes, want = main
    by = {ln.kind: w for ln, w in zip(lanes, want)}
    assert by["r = 0"] == 1 and by["leading 00 + bytes"] == 1 and by["x >= p"] == 1
    assert by["A at infinity"] == 0 and by["B_ + order 3"] == 0 and by["A_ eigenpoint"] == 0


def test_halves_fail_separately(op, main):
    """'A_ B_ scaled' keeps the pairing half, 'pairing only fails' keeps the Schnorr half"""
    key, lanes, _ = main
    _, tg, tX, _ = ac._parse_pk(op, key.pk, key.Y49)
    by = {ln.kind: ln for ln in lanes}
    pair_ok = lambda ln: op.o.pair(op.dec(ln.pres[:49])[0], tX) == op.o.pair(op.dec(ln.pres[49:98])[0], tg)
    assert pair_ok(by["A_ B_ scaled"]) and not pair_ok(by["pairing only fails"])


@pytest.mark.parametrize("nattr,I,msg_len", [(4, (), 32), (4, (0, 1, 2, 3), 32), (4, (3, 0), 32), (1, (), 32), (1, (0,), 32), (4, (0, 3), 0), (32, (0, 3), 32)])
def test_further_shapes(op, nattr, I, msg_len):
    key = ac.Key(op, 5200 + nattr, nattr)
    lanes = ac.valid_lanes(op, key, I, 2, 5300, msg_len)
    assert ac.expect(op, key, I, lanes) == b"\x01\x01"
    other = ac.Key(op, 5250 + nattr, nattr)
    assert ac.expect(op, other, I, lanes) == b"\x00\x00"


def test_undecodable_key(op, main):
    key, lanes, _ = main
    ln = lanes[0]
    for pk, Y in ((b"\x05" + key.pk[1:], key.Y49), (key.pk, key.Y49[:49] + ac.off_curve_x() + key.Y49[98:])):
        assert ac.expected_verify(op, pk, Y, ac.I_MAIN, ln.pres, ln.u, ln.attr, ln.msg) is None


def test_expected_pres(op):
    key = ac.Key(op, 5000, ac.NATTR)
    a = ac.attributes(5400, ac.NATTR)
    sig = ac.issue(op, key, a, 5401)
    attr = b"".join(ac.b48(v) for v in a)
    rnd = b"".join(v.to_bytes(32, "big") for v in (R, (1 << 256) - 1, 5, 0, R + 7))        # reduced mod r first
    msg = ac.message(5402, 0)
    p, u, st = ac.expected_pres(op, key, ac.I_MAIN, attr, sig, msg, rnd)
    assert st == 0 and len(p) == 243 and len(u) == 96
    assert ac.expected_verify(op, key.pk, key.Y49, ac.I_MAIN, p, u, ac.b48(a[0]) + ac.b48(a[3]), msg) == 1
    for bad_attr, bad_sig in ((attr[:48] + ac.b48(R) + attr[96:], sig), (attr, sig[:49] + ac.b48(R)), (attr, b"\x05" + sig[1:])):
        assert ac.expected_pres(op, key, ac.I_MAIN, bad_attr, bad_sig, msg, rnd) == (b"\xff" * 243, b"\xff" * 96, 0xff)
