"""CPU test of the expected functions of the AC issuance entries (tests/ac_issue_cases.py), so that the GPU tests cannot hide behind a vacuous oracle:
on valid inputs they return the bytes of the existing builders (ac_bbs_cases.issue, ac_rbbs_cases.issue, ac_rps_cases.issue, ac_rps_cases.user_keygen,
which restate the reference with their own grouping); the builders' chain on those records — (redact,) pres, verify — ends in 1; every constructed
lane has the status its list claims, and the degenerate lanes are degenerate where they say; key failures are where the reference throws."""
import pytest

import ac_bbs_cases as ab
import ac_issue_cases as ai
import ac_rbbs_cases as arb
import ac_rps_cases as arp
from ac_bbs_cases import b48
from g1_torsion import enc as enc96, point_of_order
from util import R, prng

SHAPES = [(1, ()), (2, (1,)), (4, (0, 3))]


@pytest.fixture(scope="module")
def op(oracle_port):
    return ab.Ops(oracle_port)


@pytest.mark.parametrize("nattr,I", SHAPES)
def test_bbs_equals_the_builder_and_verifies(op, nattr, I):
    key = ai.bbs_key(op, 7100 + nattr, nattr)
    for i in range(2):
        a = ab.attributes(7200 + i, nattr)
        w = prng(7300, i) % (R - 1) + 1
        sig, st = ai.expected_bbs_issue(op, key.sk, key.pk, key.Y49, nattr, ai.span(a), ai.b32raw(w))
        assert st == 0 and sig == ab.issue(op, key, a, 0, w=w)
        msg = ab.message(7400, i)
        p, u = ab.pres(op, key, msg, a, op.dec(sig[:49])[0], w, I, ab.draw(7500 + i, nattr - len(I)))
        assert ab.expected_verify(op, key.pk, key.Y49, I, p, u, b"".join(b48(a[k]) for k in I), msg) == 1


@pytest.mark.parametrize("nattr,I", SHAPES)
def test_rbbs_equals_the_builder_and_verifies(op, nattr, I):
    key = ai.rbbs_key(op, 7110 + nattr, nattr)
    for i in range(2):
        a = ab.attributes(7210 + i, nattr)
        w = prng(7310, i) % (R - 1) + 1
        sig, st = ai.expected_rbbs_issue(op, key.sk, key.pk, key.Y49, nattr, ai.span(a), ai.b32raw(w))
        assert st == 0 and sig == arb.issue(op, key, a, 0, w=w)
        msg = ab.message(7410, i)
        pres = arb.pres(op, msg, sig, arb.redact(op, key, a, sig, I), arb.draw(7510 + i))
        assert arb.expected_verify(op, key.pk, key.Y49, key.tY97, nattr, I, pres, b"".join(b48(a[k]) for k in I), msg) == 1


@pytest.mark.parametrize("nattr,I", SHAPES)
def test_rps_equals_the_builders_and_verifies(op, nattr, I):
    key = ai.rps_key(op, 7120 + nattr, nattr)
    for i in range(2):
        a = ab.attributes(7220 + i, nattr)
        z, upk = arp.user_keygen(op, key, 7620 + i)
        (usk48, upk49), st = ai.expected_user_keygen(op, key.pk, ai.b32raw(z))
        assert st == 0 and usk48 == b48(z) and upk49 == op.enc(upk)
        alpha = prng(7320 + i, 0) % (R - 1) + 1                                              # what ac_rps_cases.issue draws from this seed
        sig, st = ai.expected_rps_issue(op, key.sk, key.pk, key.tY97, nattr, upk49, ai.span(a), ai.b32raw(alpha))
        assert st == 0 and sig == arp.issue(op, key, upk, a, 7320 + i)
        pres = arp.pres(op, key, a, sig, arp.redact(op, key, a, sig, I), z, I, arp.draw(7520 + i))
        assert arp.expected_verify(op, key.pk, key.Y49, key.tY97, nattr, I, pres, b"".join(b48(a[k]) for k in I)) == 1


@pytest.mark.parametrize("nattr", [1, 2, 4])
@pytest.mark.parametrize("scheme", ["bbs", "rbbs"])
def test_bbs_lanes_have_the_status_they_claim(op, scheme, nattr):
    key = (ai.bbs_key if scheme == "bbs" else ai.rbbs_key)(op, 7130 + nattr, nattr)
    dlog = (ai.bbs_dlog if scheme == "bbs" else ai.rbbs_dlog)(key)
    lanes = ai.bbs_lanes(key.x, dlog, nattr, 7700)
    kinds = [ln.kind for ln in lanes]
    assert len(set(kinds) - {"valid"}) == len(kinds) - 3 and kinds.count("valid") == 3
    rows = [ai.expected_bbs_issue(op, key.sk, key.pk, key.Y49, nattr, ln.attr, ln.rnd) for ln in lanes]
    for ln, (rec, st) in zip(lanes, rows):
        assert st == ln.status and len(rec) == 97 and (rec == b"\xff" * 97) == (st == 0xff), ln.kind
    by = dict(zip(kinds, rows))
    assert by["w = r - x"][0][:49] == bytes(49) and by["sum at infinity"][0][:49] == bytes(49)       # inverse(0) = 0 on a point of G1; the empty sum
    assert by["w = 0"][0][49:] == bytes(48) == by["rnd = r"][0][49:] and by["w = 0"][0][:49] != bytes(49)
    assert by["rnd = 2^256 - 1"][0][49:] == b48(((1 << 256) - 1) % R)
    assert sum(1 for _, st in rows if st == 0xff) == 2


@pytest.mark.parametrize("nattr", [1, 2, 4])
def test_rps_lanes_have_the_status_they_claim(op, nattr):
    key = ai.rps_key(op, 7140 + nattr, nattr)
    lanes = ai.rps_lanes(op, key.g, key.x, key.y, nattr, 7800)
    rows = [ai.expected_rps_issue(op, key.sk, key.pk, key.tY97, nattr, ln.upk, ln.attr, ln.rnd) for ln in lanes]
    for ln, (rec, st) in zip(lanes, rows):
        assert st == ln.status and len(rec) == 195 and (rec == b"\xff" * 195) == (st == 0xff), ln.kind
    by = {ln.kind: r[0] for ln, r in zip(lanes, rows)}
    assert by["alpha = 0"][:98] == bytes(98) == by["rnd = r"][:98]                                    # h and sigma at infinity
    assert by["all a = 0"][98:] == bytes(97) and by["all a = 0"][:49] != bytes(49)                    # tilde_M the empty product
    assert by["sigma at infinity"][49:98] == bytes(49) and by["sigma at infinity"][:49] != bytes(49)
    ln = next(l for l in lanes if l.kind == "x + ym = 0")
    alpha = int.from_bytes(ln.rnd, "big") % R
    assert by["x + ym = 0"][49:98] == op.enc(op.mul(op.dec(ln.upk)[0], alpha * pow(key.y, nattr + 1, R) % R))
    assert sum(1 for _, st in rows if st == 0xff) == 3
    # a leading 0x00 is infinity whatever follows
    a, b = (next(l for l in lanes if l.kind == k) for k in ("upk at infinity", "upk leading 00 + bytes"))
    assert ai.expected_rps_issue(op, key.sk, key.pk, key.tY97, nattr, b.upk, a.attr, a.rnd) == (by["upk at infinity"], 0)


def test_a_merged_exponent_is_another_point_outside_g1(op):
    """h^(x + ym) for g outside G1 is not g^(alpha (x + ym)): the lane the GPU tests rely on to catch a merged exponent"""
    g = op.add(op.mul(ab.G1GEN, 77), enc96(point_of_order(3)))
    key = ai.rps_key(op, 7150, 2, g=g)
    ln = ai.rps_lanes(op, key.g, key.x, key.y, 2, 7900)[0]
    rec, st = ai.expected_rps_issue(op, key.sk, key.pk, key.tY97, 2, ln.upk, ln.attr, ln.rnd)
    a = ab._fields(ln.attr, 2)
    alpha = int.from_bytes(ln.rnd, "big") % R
    e1 = (key.x + a[0] * key.y + a[1] * key.y * key.y) % R
    merged = op.add(op.mul(g, alpha * e1 % R), op.mul(op.dec(ln.upk)[0], alpha * pow(key.y, 3, R) % R))
    assert st == 0 and rec[49:98] != op.enc(merged)


def test_key_failures_are_where_the_reference_throws(op):
    nattr = 2
    kb, kr, kp = ai.bbs_key(op, 7160, nattr), ai.rbbs_key(op, 7161, nattr), ai.rps_key(op, 7162, nattr)
    ln = ai.bbs_lanes(kb.x, None, nattr, 7950)[0]
    lp = ai.rps_lanes(op, kp.g, kp.x, kp.y, nattr, 7960)[0]
    bad49 = ab.off_curve_x()
    assert ai.expected_bbs_issue(op, kb.sk, kb.pk, kb.Y49[:49] + bad49, nattr, ln.attr, ln.rnd) is None
    assert ai.expected_bbs_issue(op, kb.sk, bad49 + kb.pk[49:], kb.Y49, nattr, ln.attr, ln.rnd) is None
    assert ai.expected_bbs_issue(op, kb.sk, kb.pk[:146] + ai.bad_g2(kb.pk[146:]), kb.Y49, nattr, ln.attr, ln.rnd) is None
    assert ai.expected_bbs_issue(op, b48(R), kb.pk, kb.Y49, nattr, ln.attr, ln.rnd) is None
    assert ai.key_failure(op, "bbs", b48(R), bad49 + kb.pk[49:], kb.Y49, nattr) == "arg"
    # AC-rbbs: y is checked though unused; a record behind the first nattr is never read
    assert ai.expected_rbbs_issue(op, kr.sk[:48] + b48(R), kr.pk, kr.Y49, nattr, ln.attr, ln.rnd) is None
    good = ai.expected_rbbs_issue(op, kr.sk, kr.pk, kr.Y49, nattr, ln.attr, ln.rnd)
    assert good[1] == 0 and ai.expected_rbbs_issue(op, kr.sk, kr.pk, kr.Y49[:49 * (nattr + 1)] + bad49, nattr, ln.attr, ln.rnd) == good
    assert ai.expected_rbbs_issue(op, kr.sk, kr.pk, kr.Y49[:49] + bad49 + kr.Y49[98:], nattr, ln.attr, ln.rnd) is None
    # AC-rps: tilde_Y[nattr] is never read, tilde_Y[0] is
    good = ai.expected_rps_issue(op, kp.sk, kp.pk, kp.tY97, nattr, lp.upk, lp.attr, lp.rnd)
    assert good[1] == 0
    assert ai.expected_rps_issue(op, kp.sk, kp.pk, kp.tY97[:97 * nattr] + ai.bad_g2(kp.tY97[97 * nattr:]), nattr, lp.upk, lp.attr, lp.rnd) == good
    assert ai.expected_rps_issue(op, kp.sk, kp.pk, ai.bad_g2(kp.tY97[:97]) + kp.tY97[97:], nattr, lp.upk, lp.attr, lp.rnd) is None
    assert ai.expected_rps_issue(op, b48(R) + kp.sk[48:], kp.pk, kp.tY97, nattr, lp.upk, lp.attr, lp.rnd) is None
    assert ai.expected_user_keygen(op, kp.pk[:49] + ai.bad_g2(kp.pk[49:146]) + kp.pk[146:], ai.b32raw(5)) is None
    assert ai.key_failure(op, "keygen", None, kp.pk[:49] + ai.bad_g2(kp.pk[49:146]) + kp.pk[146:], None, 0) == "point"
