"""CPU test of the MHAC-bbs builders (tests/mhac_bbs_cases.py) against themselves, so that the GPU tests cannot hide behind a wrong oracle: the
honest chain iss_setup .. cred_pres of the reference's test.cpp verifies under `expected_verify`, tampered lanes are rejected, malformed ones are
where the reference would throw; `expected_pres` (one flat term loop, merged Zp sums) agrees with `cred_pres` (the reference's grouping) byte for
byte; and the shapes on which the reference's formulas do NOT verify an honest presentation are pinned."""
import pytest

import mhac_bbs_cases as mh
from util import R


@pytest.fixture(scope="module")
def op(oracle_port):
    return mh.Ops(oracle_port)


@pytest.fixture(scope="module")
def world(op):
    return mh.World(op, 6000, mh.M_MAIN)


def test_the_honest_chain_of_the_small_world_verifies(op, world):
    lanes = mh.valid_lanes(op, world, mh.PRV_MAIN, mh.REV_MAIN, mh.T_MAIN, 3, 6100)
    assert mh.expect(op, world, mh.PRV_MAIN, mh.REV_MAIN, lanes) == b"\x01\x01\x01"
    assert all(len(ln.fixed) == 242 and len(ln.z) == 96 and len(ln.zhp) == 48 and len(ln.rev) == 48 for ln in lanes)
    other = mh.World(op, 6001, mh.M_MAIN)
    assert mh.expect(op, other, mh.PRV_MAIN, mh.REV_MAIN, lanes) == b"\x00\x00\x00"


def test_tampered_and_malformed_lanes(op, world):
    ln = mh.valid_lanes(op, world, mh.PRV_MAIN, mh.REV_MAIN, mh.T_MAIN, 1, 6100)[0]
    exp = lambda l: mh.expect(op, world, mh.PRV_MAIN, mh.REV_MAIN, [l])[0]
    for k in range(3):
        assert exp(mh.with_(ln, "f+1", fixed=mh.plus1(ln.fixed, k, 98))) == 0
        assert exp(mh.with_(ln, "f=r", fixed=mh.field(ln.fixed, k, R, 98))) == 0xff
    assert exp(mh.with_(ln, "z1+1", z=mh.plus1(ln.z, 1))) == 0 and exp(mh.with_(ln, "zhp+1", zhp=mh.plus1(ln.zhp, 0))) == 0
    assert exp(mh.with_(ln, "rev+1", rev=mh.plus1(ln.rev, 0))) == 0 and exp(mh.with_(ln, "rev=r", rev=mh.b48(R))) == 0xff
    assert exp(mh.with_(ln, "crev bad", crev=mh.off_curve_x())) == 0xff
    assert mh.expected_verify(op, b"\x05" + world.pp[1:], world.h49, world.pk, mh.PRV_MAIN, mh.REV_MAIN, ln.crev, ln.fixed, ln.z, ln.zhp, ln.rev) is None
    # h[1] is revealed: verify never reads it
    h49 = world.h49[:49] + mh.off_curve_x() + world.h49[98:]
    assert mh.expected_verify(op, world.pp, h49, world.pk, mh.PRV_MAIN, mh.REV_MAIN, ln.crev, ln.fixed, ln.z, ln.zhp, ln.rev) == 1


@pytest.mark.parametrize("Prv,Rev,want", [((0, 2), (1,), 1), ((0, 2), (), 0), ((2, 0), (1,), 0), ((0, 1), (), 1), ((), (), 1), ((), (0, 1, 2, 3), 1),
                                          ((0, 1, 2, 3), (), 1), ((0, 2), (1, 3), 1), ((1,), (0,), 1), ((3, 2, 1, 0), (), 0)])
def test_honest_presentations_verify_only_when_hid_starts_with_prv(op, world, Prv, Rev, want):
    """cred_pres.cpp:89 adds beta_share_j[ii] into z[ii], which verify_pres.cpp:39-42 puts on h[Prv[ii]], while U carries beta_share_j[ii] on
    h[Hid[ii]] (cred_pres.cpp:76): an honest presentation verifies exactly when Hid[ii] = Prv[ii] for every ii < nPrv.  The builders show it:
    (m = 4, Prv = (0, 2), Rev = (1)) — the reference's test.cpp — verifies; (Prv = (0, 2), Rev = ()) has Hid = (0, 1, 2, 3), Hid[1] = 1 != 2, and
    Prv = (2, 0) has Hid[0] = 0 != 2: both are rejected (and so is every other order or gap).  The entries reproduce the formulas either way."""
    Hid = mh.sets(4, Prv, Rev)[1]
    assert want == (1 if all(Hid[ii] == Prv[ii] for ii in range(len(Prv))) else 0)
    lanes = mh.valid_lanes(op, world, Prv, Rev, 3, 1, 6200)
    assert mh.expect(op, world, Prv, Rev, lanes) == bytes([want])


@pytest.mark.parametrize("m,Prv,Rev,t", [(4, (0, 2), (1,), 3), (4, (0, 2), (1,), 1), (4, (0, 1), (3,), 4), (4, (2, 0), (), 2), (1, (), (), 1), (4, (0, 1, 2, 3), (), 8)])
def test_expected_pres_agrees_with_cred_pres(op, m, Prv, Rev, t):
    wd = mh.World(op, 6300 + m, m)
    hd = mh.Holder(op, wd, Prv, Rev, t, 6400)
    vals = [R, (1 << 256) - 1, 5, 0, R + 7] + mh.draw(6500, 64)                    # reduced mod r first
    vals = vals[:mh.rnd_count(m, Prv, Rev, t)]
    got = mh.expected_pres(op, wd.pp, wd.h49, Prv, Rev, t, **hd.pres_inputs(op, vals))
    assert got == hd.present(op, wd, vals) + (0,)
    nhp = len(mh.sets(m, Prv, Rev)[2])
    assert (len(got[0]), len(got[1]), len(got[2])) == (242, 48 * len(Prv), 48 * nhp)


def test_expected_pres_marks_what_parse_refuses(op, world):
    hd = mh.Holder(op, world, mh.PRV_MAIN, mh.REV_MAIN, 3, 6400)
    ins = hd.pres_inputs(op, mh.draw(6500, mh.rnd_count(4, mh.PRV_MAIN, mh.REV_MAIN, 3)))
    bad = (b"\xff" * 242, b"\xff" * 96, b"\xff" * 48, 0xff)
    for name in ("A49", "D49", "crev49", "cpub49"):
        assert mh.expected_pres(op, world.pp, world.h49, mh.PRV_MAIN, mh.REV_MAIN, 3, **dict(ins, **{name: b"\x05" + ins[name][1:]})) == bad
    for name, count in (("lam48", 3), ("es48", 3), ("as48", 6), ("pub48", 2)):
        for i in (0, count - 1):
            assert mh.expected_pres(op, world.pp, world.h49, mh.PRV_MAIN, mh.REV_MAIN, 3, **dict(ins, **{name: mh.field(ins[name], i, R)})) == bad
    assert mh.expected_pres(op, world.pp[:49] + b"\x04" + world.pp[50:], world.h49, mh.PRV_MAIN, mh.REV_MAIN, 3, **ins) is None
    # h[1] is revealed: pres never reads it; h[3] is hidden: it does
    assert mh.expected_pres(op, world.pp, world.h49[:49] + mh.off_curve_x() + world.h49[98:], mh.PRV_MAIN, mh.REV_MAIN, 3, **ins)[3] == 0
    assert mh.expected_pres(op, world.pp, world.h49[:147] + mh.off_curve_x(), mh.PRV_MAIN, mh.REV_MAIN, 3, **ins) is None


def test_main_lanes(op, world):
    """the lanes of the GPU verify test: what is valid verifies, what is tampered is rejected, what is malformed throws; r = 0 (A_ = B_ = infinity) holds
    both halves trivially, a leading 0x00 with bytes behind it and an x >= p are the same points and hash alike; each half fails alone"""
    lanes = mh.main_lanes(op, world)
    want = mh.expect(op, world, mh.PRV_MAIN, mh.REV_MAIN, lanes)
    by = {ln.kind: (ln, w) for ln, w in zip(lanes, want)}
    assert [w for ln, w in zip(lanes, want) if ln.kind == "valid"] == [1] * 8
    assert all(by[k][1] == 0 for k in mh.ZERO_KINDS), [k for k in mh.ZERO_KINDS if by[k][1] != 0]
    assert all(by[k][1] == 0xff for k in mh.BAD_KINDS)
    assert by["r = 0"][1] == by["leading 00 + bytes"][1] == by["x >= p"][1] == 1
    assert by["C_rev + order 3"][1] == 1                                # multiply(C_rev + T, zr) = multiply(C_rev, zr) for this zr: the formulas accept it
    g2, w = op.g2dec(world.pp[49:])[0], op.g2dec(world.pk)[0]
    pair_ok = lambda ln: op.o.pair(op.dec(ln.fixed[:49])[0], w) == op.o.pair(op.dec(ln.fixed[49:98])[0], g2)
    assert pair_ok(by["A_ B_ scaled"][0]) and not pair_ok(by["pairing only fails"][0])
    hash_only = mh.World(op, 6000, mh.M_MAIN, w=op.g2mul(world.g2, world.gamma + 1))        # the other issuer key: the hash half held all along
    ln = by["pairing only fails"][0]
    assert mh.expect(op, hash_only, mh.PRV_MAIN, mh.REV_MAIN, [ln]) == b"\x01"
