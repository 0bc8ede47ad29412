"""CPU test of the BBS+ builders (tests/bbs_cases.py), so that the GPU tests cannot hide behind a wrong builder: for every variant of the public
parameters and every number of message blocks the oracle's evaluation of the verification equation gives 1 on every ACCEPT lane, 0 on every REJECT
lane and 0xff on every THROWS lane, the named corner lanes are where the issue's table puts them, no constant output passes, the compiled
reference — where it is built — returns the same bytes, and the signing expectation from the logs equals g1_mul(g1_msm(..), 1 / (gamma + x))."""
import pytest

import bbs_cases as bc
from util import R

CASES = [(v, k) for v in bc.VARIANTS + bc.OFF_G2_VARIANTS for k in bc.NMSGS if bc.applicable(v, k)]
WIRE_LENS = (0, 1, 31, 32, 62)


@pytest.fixture(scope="module")
def reference():
    from oracle.bindings import Oracle, have_reference
    return Oracle("reference") if have_reference() else None


@pytest.mark.parametrize("variant,nmsg", CASES)
def test_labels_hold_under_the_oracle(oracle_port, reference, variant, nmsg):
    p = bc.Params(oracle_port, 9100, nmsg, variant)
    ls = bc.lanes(p)
    got = bc.expect(p, ls)
    if p.in_g2:
        for ln, b in zip(ls, got):
            assert b == ln.tag, (ln.kind, b)
        assert sum(b == 1 for b in got) >= 12 and sum(b == 0 for b in got) >= 12
    else:                                               # a key outside G2: the oracle alone decides; what does not depend on w or g2 stays
        by = {ln.kind: b for ln, b in zip(ls, got)}
        assert by["A inf, B inf"] == 1 and by["A not on the curve"] == 0xff
        assert by["A inf, B != inf"] == 0 and by["A valid, B inf"] == 0
        assert {0, 1} <= set(got)
    if reference is not None:
        assert reference.bbs_plus_verify(*p.public(), *bc.pack(ls), 8) == got


def test_named_corners(oracle_port):
    """the first table of the issue, by name, on the standard parameters"""
    p = bc.Params(oracle_port, 9100, 5)
    ls = bc.lanes(p)
    by = {ln.kind: b for ln, b in zip(ls, bc.expect(p, ls))}
    for kind in ("valid", "A inf, B inf", "x = -gamma, B inf", "x = 2R - gamma, B inf", "x = gamma", "x = 0", "x = R + 13", "r = R + 11, m_1 = R + 5",
                 "r = 0, m = 0", "r h0 = m_1 h_1", "r h0 = -m_1 h_1", "sum = g1", "m_1 h_1 = -m_last h_last", "m_4 h_4 = -m_5 h_5", "x = R - 1",
                 "x = 2^256 - 1", "A + cofactor component"):
        assert by[kind] == 1, kind
    for kind in ("A inf, B != inf", "A valid, B inf", "x = -gamma, B != inf", "A = B / x", "-A", "wrong message", "wrong x", "A outside G1"):
        assert by[kind] == 0, kind
    assert by["A not on the curve"] == 0xff
    # the lanes are where their names say: points at infinity, scalars unreduced
    L = {ln.kind: ln for ln in ls}
    assert L["A inf, B inf"].A == bytes(96) and p.b_log(L["A inf, B inf"].r, L["A inf, B inf"].m) == 0
    assert L["A valid, B inf"].A != bytes(96) and p.b_log(L["A valid, B inf"].r, L["A valid, B inf"].m) == 0
    assert (L["x = -gamma, B inf"].x + p.gamma) % R == 0 and L["x = 2R - gamma, B inf"].x > R
    k = L["A = B / x"]
    assert k.a * k.x % R == p.b_log(k.r, k.m)
    k = L["sum = g1"]
    assert (p.b_log(k.r, k.m) - p.t[0]) % R == p.t[0]
    k = L["m_1 h_1 = -m_last h_last"]
    assert (k.m[0] * p.t[1] + k.m[4] * p.t[5]) % R == 0


@pytest.mark.parametrize("variant,nmsg", [(v, k) for v, k in CASES if v in bc.VARIANTS])
def test_sign_expectation(oracle_port, variant, nmsg):
    """A = [b / (gamma + x)]G from the logs == multiply(g1 * h0^r * prod h_i^m_i, inverse(gamma + x)) by the oracle, on every lane"""
    orc = oracle_port
    p = bc.Params(orc, 9100, nmsg, variant)
    ls = bc.lanes(p)
    want = bc.sign_expect(p, ls)
    for j, ln in enumerate(ls):
        B = orc.g1_msm(p.g1 + p.h0 + p.h, bc.b32(1) + bc.b32(ln.r) + b"".join(bc.b32(v) for v in ln.m), 96, 1)
        assert orc.g1_mul(B, bc.b32(bc.inv(p.gamma + ln.x)), 96) == want[96 * j:96 * j + 96], ln.kind
    by = {ln.kind: want[96 * j:96 * j + 96] for j, ln in enumerate(ls)}
    assert by["x = -gamma, B != inf"] == bytes(96) and by["A inf, B inf"] == bytes(96)        # inverse(0) = 0; B at infinity


@pytest.mark.parametrize("setting", ["standard", "spare entry undecodable", "h_k at infinity", "w at infinity"])
@pytest.mark.parametrize("msg_len", WIRE_LENS)
def test_wire_labels_hold_under_the_oracle(oracle_port, reference, msg_len, setting):
    nblk = (msg_len + 30) // 31
    spare = setting == "spare entry undecodable"
    variant = "standard" if spare else setting
    nh = nblk + 1 if spare or variant == "standard" else nblk
    if not bc.applicable(variant, nh):
        nh = nblk + 1                                     # h_k at infinity without a used entry: the spare one
    p = bc.Params(oracle_port, 9200 + msg_len, nh, variant)
    wl = bc.wire_lanes(p, msg_len)
    got = bc.wire_expect(p, wl, msg_len, spare_tag=5 if spare else None)
    for ln, b in zip(wl, got):
        assert b == ln.tag, (ln.kind, b)
    assert {0, 1, 0xff} == set(got)
    if reference is not None:
        assert bc.wire_expect(p, wl, msg_len, reference, 5 if spare else None) == got
    by = {ln.kind: b for ln, b in zip(wl, got)}
    assert by["x = r"] == 0xff and by["padding byte in x"] == 0xff and by["tag flipped"] == 0 and by["A.x + p"] == 1
    assert by["x = r - 1"] == 1 and by["r-field = r - 1"] == 1 and by["r-field = 0"] == 1 and by["x = 1"] == 1
    assert by["tag 00, tail in place"] == 0 and by["x = -gamma on a valid signature"] == 0
