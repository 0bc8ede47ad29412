"""CPU self-check of the AC-rps builders (tests/ac_rps_cases.py): the honest chain issue -> redact -> pres -> verify gives 1 for every shape of the
GPU tests; every tampered field of PresInfo gives 0; each equation, and the c0 check, fails alone where a lane says so; a wrong c0 hides a disclosed
value >= r (0, not 0xff); the expected kinds of the main lanes; the builders of pres and redact from wire bytes agree with the chain; the tail of
the q hash is 75 bytes at nI = 8 and 67 at nI = 4."""
import pytest

import ac_rps_cases as rc
from util import R


@pytest.fixture(scope="module")
def op(oracle_port):
    return rc.Ops(oracle_port)


@pytest.fixture(scope="module")
def main(op):
    key = rc.Key(op, 5000, rc.NATTR)
    lanes = rc.main_lanes(op, key)
    return key, lanes, rc.expect(op, key, rc.I_MAIN, lanes)


@pytest.mark.parametrize("nattr,I", rc.SHAPES + rc.BIG_SHAPES)
def test_honest_chain(op, nattr, I):
    key = rc.Key(op, 5200 + nattr, nattr)
    lanes = rc.valid_lanes(op, key, I, 1, 5300)
    assert rc.expect(op, key, I, lanes) == b"\x01"
    assert rc.checks(op, key, I, lanes[0].pres, lanes[0].attr) == (True, True, True)


def test_kinds(main):
    key, lanes, want = main
    by = {ln.kind: w for ln, w in zip(lanes, want)}
    assert len(by) == len(lanes) - 2                                            # three lanes are called valid
    assert [k for k in rc.ONE_KINDS if by[k] != 1] == []
    assert [k for k in rc.ZERO_KINDS if by[k] != 0] == []
    assert [k for k in rc.BAD_KINDS if by[k] != 0xff] == []
    assert by["tilde_H outside G2"] in (0, 1)


def test_each_check_fails_alone(op, main):
    key, lanes, _ = main
    by = {ln.kind: ln for ln in lanes}
    ck = lambda kind: rc.checks(op, key, rc.I_MAIN, by[kind].pres, by[kind].attr)
    assert ck("eq1 only fails") == (True, False, True)
    assert ck("eq2 only fails") == (True, True, False)
    # s0 is in neither equation: the Schnorr check alone fails
    assert rc.checks(op, key, rc.I_MAIN, by["s0+1"].pres, by["s0+1"].attr, past_c0=True) == (False, True, True)


def test_c0_before_attributes(op, main):
    key, lanes, want = main
    by = {ln.kind: w for ln, w in zip(lanes, want)}
    assert by["c0 wrong and a = r"] == 0 and by["a = r"] == 0xff


def test_q_tail_lengths():
    assert rc.q_tail_bytes(8) == 75 and rc.q_tail_bytes(4) == 67
    assert [(195 + 56 * nI) % 72 for nI in range(9)] == [51, 35, 19, 3, 59, 43, 27, 11, 67]


def test_wire_builders_agree_with_the_chain(op):
    key = rc.Key(op, 5000, rc.NATTR)
    cr = rc.Cred(op, key, rc.I_MAIN, 5100, 0)
    assert rc.expected_redact(op, key.tY97, rc.NATTR, rc.I_MAIN, cr.attr_all, cr.sig) == (cr.cache, 0)
    p, st = rc.expected_pres(op, key.pk, key.Y49, rc.NATTR, rc.I_MAIN, cr.attr_all, cr.sig, cr.cache, cr.usk, cr.rnd96)
    assert st == 0 and p == rc.pres(op, key, cr.a, cr.sig, cr.cache, cr.z, rc.I_MAIN, cr.rnd)
    assert rc.expected_verify(op, key.pk, key.Y49, key.tY97, rc.NATTR, rc.I_MAIN, p, cr.attr) == 1
    # a hidden attribute >= r: redact does not read it, pres throws
    big = rc._field(cr.attr_all, 1, R)
    assert rc.expected_redact(op, key.tY97, rc.NATTR, rc.I_MAIN, big, cr.sig) == (cr.cache, 0)
    assert rc.expected_pres(op, key.pk, key.Y49, rc.NATTR, rc.I_MAIN, big, cr.sig, cr.cache, cr.usk, cr.rnd96) == (b"\xff" * 389, 0xff)
    # nI = 0: tilde_M re-encoded
    assert rc.expected_redact(op, key.tY97, rc.NATTR, (), cr.attr_all, cr.sig) == (cr.sig[98:], 0)
