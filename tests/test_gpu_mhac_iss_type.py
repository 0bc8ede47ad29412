"""c12381_mhac_bbs_type_batch: make_pres_type of the reference's examples/MHAC-bbs from the wire formats.  C_rev, C_pub and the status of the host and the
_dev form equal tests/mhac_iss_cases.py's expected_type: the reference's world; nothing revealed (C_rev = g1) and every public attribute revealed
(C_pub = C_rev); nPrv = 0 and nPrv = m (no public value at all: both are g1); a public value 0; an h record outside G1 or at infinity; values = r
and 2^384 - 1 beside good lanes; public records that do not decode; more than one block."""
import pytest

import mhac_bbs_cases as mh
import mhac_iss_cases as mi
from g1_torsion import enc as enc96, eigenpoint, point_of_order
from util import R, prng

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = mi.ctx_fixture()
    yield c
    c.close()


@pytest.fixture(scope="module")
def op(oracle_port):
    return mh.Ops(oracle_port)


def spans(seed, nPub, count):
    return [b"".join(mh.b48(prng(seed + j, k) % R) for k in range(nPub)) for j in range(count)]


def check(ctx, op, wd, Prv, Rev, pubs):
    want = mi.want_type(op, wd, Prv, Rev, pubs)
    mi.both(lambda dev: ctx.mhac_bbs_type(wd.pp, wd.h49, Prv, Rev, b"".join(pubs), n=len(pubs), dev=dev), want)
    return want


@pytest.mark.parametrize("m,Prv,Rev", [(4, (0, 2), (1,)), (4, (0, 2), ()), (4, (0, 2), (3, 1)), (4, (), (1,)), (4, (), (0, 1, 2, 3)), (4, (0, 1, 2, 3), ()),
                                       (4, (2, 0), (1,)), (1, (), ()), (1, (), (0,)), (32, (0, 2), (5, 31, 17)), (5, (1, 3), (4, 0))])
def test_shapes(ctx, op, m, Prv, Rev):
    wd = mh.World(op, 6000 + m, m)
    nPub = m - len(Prv)
    crev, cpub, st = check(ctx, op, wd, Prv, Rev, spans(9500 + m, nPub, 4))
    assert st == bytes(4)
    g1 = op.enc(wd.g1)
    if all(i in Prv for i in Rev):
        assert crev == g1 * 4
    if all(i in Rev or i in Prv for i in range(m)):
        assert cpub == crev


def test_degenerate_and_bad_lanes(ctx, op):
    wd = mh.World(op, 6004, 4)
    Prv, Rev = (0, 2), (1,)
    pubs = spans(9600, 2, 3)
    pubs.insert(1, mh.field(pubs[0], 0, 0))                      # the revealed value 0: C_rev = g1
    pubs.insert(2, mh.field(pubs[0], 1, 0))
    pubs.append(bytes(96))
    pubs.insert(1, mh.field(pubs[0], 0, R))
    pubs.insert(3, mh.field(pubs[0], 1, R))
    pubs.append(mh.field(pubs[0], 0, (1 << 384) - 1))
    pubs.append(mh.field(pubs[0], 1, 1 << 256))
    crev, cpub, st = check(ctx, op, wd, Prv, Rev, pubs)
    assert st.count(0xff) == 4 and st.count(0) == 6
    assert crev[49 * 2:49 * 3] == op.enc(wd.g1) and cpub[49 * 7:49 * 8] == op.enc(wd.g1)


@pytest.mark.parametrize("kind", ["revealed h + order 3", "hidden h eigenpoint", "hidden h at infinity"])
def test_h_outside_g1(ctx, op, kind):
    base = mh.World(op, 6004, 4)
    h = {"revealed h + order 3": {1: op.add(base.h[1], enc96(point_of_order(3)))}, "hidden h eigenpoint": {3: enc96(eigenpoint(10177)[0])},
         "hidden h at infinity": {3: bytes(96)}}[kind]
    wd = mh.World(op, 6004, 4, h=h)
    check(ctx, op, wd, (0, 2), (1,), spans(9700, 2, 3))


def test_public_records(ctx, op):
    """an undecodable pp or Pub record of h: every byte 0xff and C12381_E_POINT; a private record is not read"""
    from types import SimpleNamespace
    from crypto12381_amd.capi import C12381Error, E_POINT
    wd = mh.World(op, 6004, 4)
    Prv, Rev = (0, 2), (1,)
    pubs = spans(9800, 2, 3)
    good = check(ctx, op, wd, Prv, Rev, pubs)
    run = lambda w, **kw: ctx.mhac_bbs_type(w.pp, w.h49, Prv, Rev, b"".join(pubs), **kw)
    unread = SimpleNamespace(pp=wd.pp, h49=mh.off_curve_x() + wd.h49[49:])
    assert run(unread) == good and run(unread, dev=True) == good
    for pp, h49 in ((b"\x05" + wd.pp[1:], wd.h49), (wd.pp[:49] + b"\x04" + wd.pp[50:], wd.h49), (wd.pp, wd.h49[:49] + mh.off_curve_x() + wd.h49[98:]),
                    (wd.pp, wd.h49[:147] + mh.off_curve_x())):
        bad = SimpleNamespace(pp=pp, h49=h49)
        assert mi.expected_type(op, pp, h49, Prv, Rev, pubs[0]) is None
        for dev in (False, True):
            assert run(bad, strict=False, dev=dev) == (b"\xff" * 147, b"\xff" * 147, b"\xff" * 3)
        with pytest.raises(C12381Error) as e:
            run(bad)
        assert e.value.code == E_POINT
        assert run(wd) == good


def test_more_than_one_block(ctx, op):
    wd = mh.World(op, 6004, 4)
    Prv, Rev = (0, 2), (1,)
    pubs = spans(9900, 2, 6) + [mh.field(bytes(96), 1, R)]
    rows = [mi.expected_type(op, wd.pp, wd.h49, Prv, Rev, p) for p in pubs]
    idx = [(3 * j) % 7 for j in range(300)]
    want = b"".join(rows[i][0] for i in idx), b"".join(rows[i][1] for i in idx), bytes(rows[i][2] for i in idx)
    mi.both(lambda dev: ctx.mhac_bbs_type(wd.pp, wd.h49, Prv, Rev, b"".join(pubs[i] for i in idx), dev=dev), want)
