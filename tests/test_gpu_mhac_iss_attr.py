"""c12381_mhac_bbs_attr_batch: generate_attributes of the reference's examples/MHAC-bbs from the caller's randomness.  Every output byte of the host and
the _dev form equals tests/mhac_iss_cases.py's expected_attr (exact integer powers, term-by-term sums by the CPU oracle): the reference's world;
t = 1, 5, 8; nPrv = 0 and nPrv = m; Prv permuted; randomness at and above r; a share equal to 0; an h record outside G1 or at infinity (the generic
route); public records that do not decode; a batch with more than one block of lanes."""
import pytest

import mhac_bbs_cases as mh
import mhac_iss_cases as mi
from g1_torsion import enc as enc96, eigenpoint, point_of_order
from util import R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = mi.ctx_fixture()
    yield c
    c.close()


@pytest.fixture(scope="module")
def op(oracle_port):
    return mh.Ops(oracle_port)


def check(ctx, op, wd, Prv, t, nparties, rnds):
    want = mi.want_attr(op, wd, Prv, t, nparties, rnds)
    mi.both(lambda dev: ctx.mhac_bbs_attr(wd.pp, wd.h49, Prv, t, nparties, b"".join(rnds), dev=dev), want)
    return want


@pytest.mark.parametrize("m,Prv,t,nparties,count", [(4, (0, 2), 3, 6, 5), (4, (0, 2), 1, 1, 3), (4, (0, 2), 1, 4, 3), (4, (2, 0), 5, 6, 3), (4, (0, 2), 8, 8, 3),
                                                    (4, (), 3, 6, 3), (4, (0, 1, 2, 3), 2, 3, 3), (4, (3, 1, 0), 2, 64, 3), (1, (0,), 2, 2, 4), (32, (31, 0, 7), 3, 4, 3)])
def test_shapes(ctx, op, m, Prv, t, nparties, count):
    """the reference's world first; the first credential of each batch draws values at and above r"""
    wd = mh.World(op, 6000 + m, m)
    pub, ashare, C = check(ctx, op, wd, Prv, t, nparties, mi.attr_rnd(9000 + t, m, Prv, t, count))
    assert len(pub) == 48 * (m - len(Prv)) * count and len(ashare) == 48 * len(Prv) * nparties * count and len(C) == 49 * nparties * count
    if not Prv:
        assert C == bytes(len(C))


def test_a_share_equal_to_zero(ctx, op):
    """t = 2: attr = r - 3 and the coefficient 1 make party 2's share 0, so its commitment has one term at infinity; both shares 0: C = infinity"""
    wd = mh.World(op, 6004, 4)
    Prv, t, np_ = (0, 2), 2, 4
    base = mi.rnd_values(mi.attr_rnd(9100, 4, Prv, t, 1, big_first=False)[0])
    one = mi.rnd_bytes([R - 3] + base[1:4] + [1] + base[5:])
    two = mi.rnd_bytes([R - 3, base[1], R - 3, base[3], 1, 1])
    _, ashare, C = check(ctx, op, wd, Prv, t, np_, [one, two])
    assert ashare[48 * (2 * 2):48 * (2 * 2) + 48] == bytes(48)
    assert C[49 * (4 + 2):49 * (4 + 3)] == bytes(49)


@pytest.mark.parametrize("kind", ["order 3 added", "eigenpoint", "infinity"])
def test_h_outside_g1(ctx, op, kind):
    """a private h record outside G1: the sum runs column by column through the generic kernel"""
    base = mh.World(op, 6004, 4)
    h = {"order 3 added": {2: op.add(base.h[2], enc96(point_of_order(3)))}, "eigenpoint": {0: enc96(eigenpoint(10177)[0])}, "infinity": {2: bytes(96)}}[kind]
    wd = mh.World(op, 6004, 4, h=h)
    check(ctx, op, wd, (0, 2), 3, 6, mi.attr_rnd(9200, 4, (0, 2), 3, 3))


def test_public_records(ctx, op):
    """an undecodable pp or private h: every byte 0xff and C12381_E_POINT; an undecodable record at a public position is not read"""
    from types import SimpleNamespace
    from crypto12381_amd.capi import C12381Error, E_POINT
    wd = mh.World(op, 6004, 4)
    Prv, t, np_ = (0, 2), 3, 6
    rnds = mi.attr_rnd(9300, 4, Prv, t, 3)
    good = check(ctx, op, wd, Prv, t, np_, rnds)
    run = lambda w, **kw: ctx.mhac_bbs_attr(w.pp, w.h49, Prv, t, np_, b"".join(rnds), **kw)
    unread = SimpleNamespace(pp=wd.pp, h49=wd.h49[:49] + mh.off_curve_x() + wd.h49[98:])
    assert run(unread) == good and run(unread, dev=True) == good
    for pp, h49 in ((b"\x05" + wd.pp[1:], wd.h49), (wd.pp[:49] + b"\x04" + wd.pp[50:], wd.h49), (wd.pp, mh.off_curve_x() + wd.h49[49:]),
                    (wd.pp, wd.h49[:98] + b"\x07" + wd.h49[99:])):
        bad = SimpleNamespace(pp=pp, h49=h49)
        assert mi.expected_attr(op, pp, h49, Prv, t, np_, rnds[0]) is None
        for dev in (False, True):
            assert run(bad, strict=False, dev=dev) == tuple(b"\xff" * len(g) for g in good)
        with pytest.raises(C12381Error) as e:
            run(bad)
        assert e.value.code == E_POINT
        assert run(wd) == good                                                       # the context recovers


def test_more_than_one_block(ctx, op):
    """70 credentials of 6 parties: 420 lanes, two blocks; six distinct credentials tiled"""
    wd = mh.World(op, 6004, 4)
    Prv, t, np_ = (0, 2), 3, 6
    rnds = mi.attr_rnd(9400, 4, Prv, t, 6)
    rows = [mi.expected_attr(op, wd.pp, wd.h49, Prv, t, np_, r) for r in rnds]
    idx = [(5 * j) % 6 for j in range(70)]
    want = tuple(b"".join(rows[i][k] for i in idx) for k in range(3))
    mi.both(lambda dev: ctx.mhac_bbs_attr(wd.pp, wd.h49, Prv, t, np_, b"".join(rnds[i] for i in idx), dev=dev), want)
