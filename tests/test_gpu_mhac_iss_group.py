"""c12381_mhac_bbs_group_batch: make_pres_group of the reference's examples/MHAC-bbs, with the gather of the rows of S.  lambda, D, the gathered rows and
the status of the host and the _dev form equal tests/mhac_iss_cases.py's expected_group: the reference's world (6 parties, S = (0, 2, 5)); S permuted;
t = 1, t = 5 (4 + 1 terms) and t = 8 of 8 parties (two products joined by an addition); nPrv = 0; the optional rows absent; D records at infinity and
outside G1 (order-3 and order-11 points added, and a point of order 11 alone); rows that are not below r are copied verbatim; D
records that do not decode, in S (0xff) and outside S (never read); more than one block."""
import pytest

import mhac_bbs_cases as mh
import mhac_iss_cases as mi
from g1_torsion import enc as enc96, point_of_order
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


def rows_of(op, wd, Prv, t, nparties, count, seed):
    """(D49, es48, as48) of `count` honest credentials"""
    return [(i[2], i[1], a[1]) for a, i, _, _, _ in mi.honest(op, wd, Prv, t, nparties, count, seed)]


def check(ctx, op, S, nparties, nPrv, rows):
    want = mi.want_group(op, S, nparties, nPrv, rows)
    none = lambda k: None if rows[0][k] is None else b"".join(r[k] for r in rows)
    mi.both(lambda dev: ctx.mhac_bbs_group(S, nparties, nPrv, b"".join(r[0] for r in rows), none(1), none(2), dev=dev), want)
    return want


@pytest.mark.parametrize("Prv,t,nparties,S", [((0, 2), 3, 6, (0, 2, 5)), ((0, 2), 3, 6, (5, 0, 2)), ((0, 2), 3, 6, (2, 5, 0)), ((0, 2), 1, 1, (0,)), ((0, 2), 1, 4, (3,)),
                                              ((2, 0), 5, 6, (5, 1, 0, 3, 2)), ((0, 2), 8, 8, (7, 0, 1, 2, 3, 4, 5, 6)), ((), 2, 3, (2, 0)), ((0, 1, 2, 3), 2, 64, (63, 0))])
def test_shapes(ctx, op, Prv, t, nparties, S):
    wd = mh.World(op, 6004, 4)
    rows = rows_of(op, wd, Prv, t, nparties, 3, 10000 + t)
    lam, Dg, eS, aS, st = check(ctx, op, S, nparties, len(Prv), rows)
    assert st == bytes(3) and len(eS) == 48 * t * 3 and len(aS) == 48 * t * len(Prv) * 3
    xs = [i + 1 for i in S]
    assert lam[:48 * t] == b"".join(mh.b48(mh.lagrange(xs, k)) for k in range(t))


def test_the_optional_rows(ctx, op):
    wd = mh.World(op, 6004, 4)
    rows = rows_of(op, wd, (0, 2), 3, 6, 3, 10100)
    full = check(ctx, op, (0, 2, 5), 6, 2, rows)
    no_e = check(ctx, op, (0, 2, 5), 6, 2, [(d, None, a) for d, e, a in rows])
    no_a = check(ctx, op, (0, 2, 5), 6, 2, [(d, e, None) for d, e, a in rows])
    none = check(ctx, op, (0, 2, 5), 6, 2, [(d, None, None) for d, e, a in rows])
    assert no_e == full[:2] + (b"",) + full[3:] and no_a == full[:3] + (b"",) + full[4:] and none == full[:2] + (b"", b"") + full[4:]


def test_degenerate_and_bad_lanes(ctx, op):
    wd = mh.World(op, 6004, 4)
    S, np_ = (0, 2, 5), 6
    rows = rows_of(op, wd, (0, 2), 3, np_, 3, 10200)
    D, es, as_ = rows[0]
    rec = lambda b, i, new: b[:49 * i] + new + b[49 * i + 49:]
    pt = lambda i: op.dec(D[49 * i:49 * i + 49])[0]
    t3, t11 = enc96(point_of_order(3)), enc96(point_of_order(11))
    lanes = list(rows)
    lanes.append((rec(D, 2, bytes(49)), es, as_))                                             # a D record of S at infinity
    lanes.append((rec(D, 0, b"\x00" + bytes(range(1, 49))), es, as_))
    lanes.append((rec(D, 5, op.enc(op.add(pt(5), t3))), es, as_))                             # outside G1
    lanes.append((rec(D, 0, op.enc(op.add(pt(0), t11))), es, as_))
    lanes.append((rec(D, 2, op.enc(t11)), es, as_))
    lanes.append((D, mh.field(es, 2, R), mh.field(as_, 1, (1 << 384) - 1)))                   # copied verbatim: pres checks them
    lanes.append((rec(D, 1, mh.off_curve_x()), es, as_))                                      # party 1 is outside S: never read
    lanes.append((rec(D, 3, b"\x05" + D[49 * 3 + 1:49 * 4]), es, as_))
    good = len(lanes)
    lanes.insert(1, (rec(D, 0, mh.off_curve_x()), es, as_))
    lanes.insert(3, (rec(D, 5, b"\x05" + D[49 * 5 + 1:49 * 6]), es, as_))
    lanes.append((rec(D, 2, b"\x04" + D[49 * 2 + 1:49 * 3]), es, as_))
    lam, Dg, eS, aS, st = check(ctx, op, S, np_, 2, lanes)
    assert st.count(0) == good and st.count(0xff) == 3
    assert lam[48 * 3:48 * 6] == b"\xff" * 144 and eS[48 * 3:48 * 6] == b"\xff" * 144 and aS[96 * 3:96 * 6] == b"\xff" * 288


def test_more_than_one_block(ctx, op):
    wd = mh.World(op, 6004, 4)
    S, np_ = (0, 2, 5), 6
    rows = rows_of(op, wd, (0, 2), 3, np_, 5, 10300)
    rows.append((rows[0][0][:49 * 2] + mh.off_curve_x() + rows[0][0][49 * 3:], rows[0][1], rows[0][2]))
    exp = [mi.expected_group(op, S, np_, 2, *r) for r in rows]
    idx = [(5 * j) % 6 for j in range(300)]
    want = tuple(b"".join(exp[i][k] for i in idx) for k in range(4)) + (bytes(exp[i][4] for i in idx),)
    mi.both(lambda dev: ctx.mhac_bbs_group(S, np_, 2, *(b"".join(rows[i][k] for i in idx) for k in range(3)), dev=dev), want)
