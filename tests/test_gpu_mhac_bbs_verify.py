"""c12381_mhac_bbs_verify_batch: MHAC-bbs presentations (the reference's examples/MHAC-bbs/src/verify_pres.cpp) from the wire formats.  Worlds,
credentials and presentations are made by tests/mhac_bbs_cases.py as iss_setup .. cred_pres make them; the expected byte of every lane is
verify_pres composed independently from the CPU oracle's primitives.  Lanes of the small world (m = 4, Prv = (0, 2), Rev = (1), t = 3): valid,
every field tampered, each half failing alone, A_ = B_ = infinity, a leading 0x00 with bytes behind it, x >= p, A_ / B_ / C_rev plus an order-3
point or an eigenpoint, ch = 0, malformed points and Zp fields >= r (0xff); shapes: Prv empty, Prv = all (pub_48 NULL), Rev empty, Rev = all of
Pub, Prv unordered, m = 1, m = 32; keys: another key, an h record outside G1 at a used position (generic route) and an undecodable one at an unused
position (not read), w outside G2, an undecodable pp / used h / pk (every lane 0xff, C12381_E_POINT); one tiled run of 2^12 + 1 lanes in host and
_dev form."""
import pytest

import mhac_bbs_cases as mh
from g1_torsion import enc as enc96, point_of_order

pytestmark = pytest.mark.gpu
PRV, REV, T = mh.PRV_MAIN, mh.REV_MAIN, mh.T_MAIN


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
    return mh.Ops(oracle_port)


@pytest.fixture(scope="module")
def main(op):
    wd = mh.World(op, 6000, mh.M_MAIN)
    lanes = mh.main_lanes(op, wd)
    return wd, lanes, mh.expect(op, wd, PRV, REV, lanes)


def run(ctx, wd, Prv, Rev, lanes, **kw):
    return ctx.mhac_bbs_verify(wd.pp, wd.h49, wd.pk, Prv, Rev, *mh.pack(lanes), **kw)


def check(ctx, op, wd, Prv, Rev, lanes):
    got, want = run(ctx, wd, Prv, Rev, lanes), mh.expect(op, wd, Prv, Rev, lanes)
    bad = [(ln.kind, g, w) for ln, g, w in zip(lanes, got, want) if g != w]
    assert not bad, bad
    return want


def test_main_shape(ctx, main):
    wd, lanes, want = main
    got = run(ctx, wd, PRV, REV, lanes)
    bad = [(ln.kind, g, w) for ln, g, w in zip(lanes, got, want) if g != w]
    assert not bad, bad
    by = {ln.kind: w for ln, w in zip(lanes, want)}
    assert sum(1 for ln, w in zip(lanes, want) if ln.kind == "valid" and w == 1) == 8
    assert all(by[k] == 0 for k in mh.ZERO_KINDS) and all(by[k] == 0xff for k in mh.BAD_KINDS)
    assert by["r = 0"] == by["leading 00 + bytes"] == by["x >= p"] == by["C_rev + order 3"] == 1


@pytest.mark.parametrize("m,Prv,Rev", [(4, (), (1,)), (4, (0, 1, 2, 3), ()), (4, (0, 1), ()), (4, (0, 2), ()), (4, (0, 2), (1, 3)), (4, (2, 0), (1,)), (1, (), ()),
                                       (1, (0,), ()), (1, (), (0,)), (32, (0, 2), (1,)), (32, (0, 1), (5, 31, 17))])
def test_further_shapes(ctx, op, m, Prv, Rev):
    """honest presentations — which the reference's formulas accept exactly when Hid starts with Prv — and one tampered field of every kind the
    shape has; (4, (0, 2), ()) and (4, (2, 0), (1)) are shapes whose honest presentations are rejected"""
    wd = mh.World(op, 6600 + m, m)
    lanes = mh.valid_lanes(op, wd, Prv, Rev, T, 3, 6700)
    lanes.append(mh.with_(lanes[0], "zr+1", fixed=mh.plus1(lanes[0].fixed, 1, 98)))
    if Prv:
        lanes.append(mh.with_(lanes[1], "z+1", z=mh.plus1(lanes[1].z, len(Prv) - 1)))
    if lanes[0].zhp:
        lanes.append(mh.with_(lanes[2], "zhp+1", zhp=mh.plus1(lanes[2].zhp, len(lanes[2].zhp) // 48 - 1)))
    if lanes[0].rev:
        lanes.append(mh.with_(lanes[0], "rev+1", rev=mh.plus1(lanes[0].rev, len(lanes[0].rev) // 48 - 1)))
        lanes.append(mh.with_(lanes[0], "rev = r", rev=mh.field(lanes[0].rev, 0, mh.R)))
    want = check(ctx, op, wd, Prv, Rev, lanes)
    Hid = mh.sets(m, Prv, Rev)[1]
    honest = 1 if all(Hid[ii] == Prv[ii] for ii in range(len(Prv))) else 0
    assert want[:4] == bytes([honest] * 3 + [0]) and set(want[4:]) <= {0, 0xff}


def test_unordered_prv_is_not_sorted(ctx, op):
    """z[ii] belongs to h[prv[ii]]: the fields of Prv = (0, 2) offered under (2, 0) are the wrong way round, and swapped back they verify"""
    wd = mh.World(op, 6604, 4)
    lanes = mh.valid_lanes(op, wd, (0, 2), (1,), T, 2, 6700)
    assert run(ctx, wd, (0, 2), (1,), lanes) == b"\x01\x01"
    assert run(ctx, wd, (2, 0), (1,), lanes) == mh.expect(op, wd, (2, 0), (1,), lanes) == b"\x00\x00"
    swapped = [mh.with_(ln, "swapped", z=ln.z[48:] + ln.z[:48]) for ln in lanes]
    assert run(ctx, wd, (2, 0), (1,), swapped) == mh.expect(op, wd, (2, 0), (1,), swapped) == b"\x01\x01"


def test_second_key_and_back(ctx, op, main):
    """every lane fails under another world; the first world's tables are rebuilt when it returns"""
    wd, lanes, want = main
    other = mh.World(op, 6001, mh.M_MAIN)
    assert set(check(ctx, op, other, PRV, REV, lanes[:8])) == {0}
    assert run(ctx, wd, PRV, REV, lanes[:8]) == want[:8] == b"\x01" * 8


@pytest.mark.parametrize("kind", ["private h outside G1", "hidden public h outside G1", "hidden h at infinity", "w outside G2"])
def test_generic_routes(ctx, op, kind):
    """public points outside the subgroups: the fixed-base sum falls back to the generic kernel, the pairing half to the generic pairing; the
    presentations are made under that world with the oracle's multiply, and the verdicts are expected_verify's whatever they are"""
    t3 = enc96(point_of_order(3))
    base = mh.World(op, 6800, mh.M_MAIN)
    kw = {"private h outside G1": dict(h={2: op.add(base.h[2], t3)}), "hidden public h outside G1": dict(h={3: op.add(base.h[3], t3)}),
          "hidden h at infinity": dict(h={3: bytes(96)}), "w outside G2": dict(w=mh.g2_outside())}[kind]
    wd = mh.World(op, 6800, mh.M_MAIN, **kw)
    lanes = mh.valid_lanes(op, wd, PRV, REV, T, 4, 6900)
    lanes.append(mh.with_(lanes[0], "ze+1", fixed=mh.plus1(lanes[0].fixed, 2, 98)))
    lanes.append(mh.with_(lanes[1], "z1+1", z=mh.plus1(lanes[1].z, 1)))
    lanes.append(mh.with_(lanes[2], "zhp+1", zhp=mh.plus1(lanes[2].zhp, 0)))
    want = check(ctx, op, wd, PRV, REV, lanes)
    if kind == "hidden h at infinity":
        assert want[:4] == b"\x01" * 4


def test_an_unused_h_record_is_not_read(ctx, op, main):
    """h[1] is revealed: its value sits in C_rev, and verify neither reads nor decodes the record"""
    from types import SimpleNamespace
    wd, lanes, want = main
    for rec in (mh.off_curve_x(), b"\x05" + bytes(48)):
        odd = SimpleNamespace(pp=wd.pp, h49=wd.h49[:49] + rec + wd.h49[98:], pk=wd.pk)
        assert run(ctx, odd, PRV, REV, lanes) == want


def test_undecodable_public_records(ctx, op, main):
    from types import SimpleNamespace
    from crypto12381_amd.capi import C12381Error, E_POINT
    wd, lanes, want = main
    ln = lanes[0]
    for pp, h49, pk in ((b"\x05" + wd.pp[1:], wd.h49, wd.pk), (wd.pp[:49] + b"\x04" + wd.pp[50:], wd.h49, wd.pk), (wd.pp, wd.h49, b"\x04" + wd.pk[1:]),
                        (wd.pp, mh.off_curve_x() + wd.h49[49:], wd.pk), (wd.pp, wd.h49[:147] + mh.off_curve_x(), wd.pk)):
        bad = SimpleNamespace(pp=pp, h49=h49, pk=pk)
        assert mh.expected_verify(op, pp, h49, pk, PRV, REV, ln.crev, ln.fixed, ln.z, ln.zhp, ln.rev) is None
        assert run(ctx, bad, PRV, REV, lanes[:5], strict=False) == b"\xff" * 5
        with pytest.raises(C12381Error) as e:
            run(ctx, bad, PRV, REV, lanes[:5])
        assert e.value.code == E_POINT
        assert run(ctx, wd, PRV, REV, lanes[:2]) == b"\x01\x01"                      # the context recovers


def test_large_tiled_host_and_dev(ctx, op, main):
    wd, lanes, want_d = main
    distinct = list(lanes) + mh.valid_lanes(op, wd, PRV, REV, T, 48 - len(lanes), 7300)
    want_d = want_d + b"\x01" * (48 - len(lanes))
    assert mh.expect(op, wd, PRV, REV, distinct[len(lanes):]) == want_d[len(lanes):]
    n = (1 << 12) + 1
    idx = [(j * 37) % 48 for j in range(n)]
    tiled = [distinct[i] for i in idx]
    want = bytes(want_d[i] for i in idx)
    assert run(ctx, wd, PRV, REV, tiled) == want
    assert run(ctx, wd, PRV, REV, tiled, dev=True) == want
