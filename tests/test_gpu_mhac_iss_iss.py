"""c12381_mhac_bbs_iss_batch: cred_iss of the reference's examples/MHAC-bbs from the wire formats and the caller's randomness.  A, e_share, D and the status
of the host and the _dev form equal tests/mhac_iss_cases.py's expected_iss (term by term on the CPU oracle): the reference's world; t = 1, t = 5
(4 + 1 terms) and t = 8 of 8 parties (two products joined by an addition); nPub = 0 and nPub = m; pub_idx permuted; randomness at and above r;
gamma + e = 0 (A at infinity, D = C); an e_share equal to 0; C records at infinity; C records outside G1 (order-3 and order-11 points, among the
first t and behind them), where one power of merged exponents would be another point; a public h record outside G1; bad lanes beside good ones
(off-curve x, bad tag, value = r, value = 2^384 - 1); sk = r; public records that do not decode; more than one block."""
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


def creds_of(op, wd, Prv, t, nparties, count, seed, pub_idx=None):
    """(C49, pub48, rnd) of `count` honest credentials; the first draws e and the last coefficient at and above r"""
    return [(a[2], pub48, ri) for a, _, _, ri, pub48 in mi.honest(op, wd, Prv, t, nparties, count, seed, pub_idx)]


def run(ctx, wd, sk48, pub_idx, t, nparties, creds, **kw):
    return ctx.mhac_bbs_iss(wd.pp, wd.h49, sk48, pub_idx, t, nparties, *(b"".join(c[k] for c in creds) for k in range(3)), **kw)


def check(ctx, op, wd, pub_idx, t, nparties, creds, sk48=None):
    sk48 = mh.b48(wd.gamma) if sk48 is None else sk48
    want = mi.want_iss(op, wd, sk48, pub_idx, t, nparties, creds)
    mi.both(lambda dev: run(ctx, wd, sk48, pub_idx, t, nparties, creds, dev=dev), want)
    return want


@pytest.mark.parametrize("m,Prv,t,nparties,pub_idx", [(4, (0, 2), 3, 6, (1, 3)), (4, (0, 2), 3, 6, (3, 1)), (4, (0, 2), 1, 1, (1, 3)), (4, (0, 2), 1, 4, (1, 3)),
                                                      (4, (2, 0), 5, 6, (1, 3)), (4, (0, 2), 8, 8, (3, 1)), (4, (0, 1, 2, 3), 2, 3, ()), (4, (), 2, 3, (2, 0, 3, 1)),
                                                      (1, (0,), 2, 64, ()), (32, (0, 2), 4, 4, tuple(range(31, 2, -1)) + (1,))])
def test_shapes(ctx, op, m, Prv, t, nparties, pub_idx):
    wd = mh.World(op, 6000 + m, m)
    A, es, D, st = check(ctx, op, wd, pub_idx, t, nparties, creds_of(op, wd, Prv, t, nparties, 3, 11000 + t, pub_idx))
    assert st == bytes(3) and len(A) == 147 and len(es) == 48 * nparties * 3 and len(D) == 49 * nparties * 3


def test_gamma_plus_e_zero_and_a_zero_share(ctx, op):
    wd = mh.World(op, 6004, 4)
    t, np_, pub_idx = 2, 4, (1, 3)
    creds = creds_of(op, wd, (0, 2), t, np_, 3, 11100)
    C, pub48, rnd = creds[1]
    creds.append((C, pub48, mi.rnd_bytes([(R - wd.gamma) % R]) + rnd[32:]))                  # gamma + e = 0: A = infinity, D = C
    creds.append((C, pub48, mi.rnd_bytes([R - 3, 1])))                                       # e_share[2] = 0: D[2] = C[2]
    creds.append((C, pub48, mi.rnd_bytes([(1 << 256) - 1, R])))                              # a coefficient that reduces to 0
    A, es, D, st = check(ctx, op, wd, pub_idx, t, np_, creds)
    assert st == bytes(6)
    assert A[49 * 3:49 * 4] == bytes(49) and D[49 * np_ * 3:49 * np_ * 4] == C
    assert es[48 * (np_ * 4 + 2):48 * (np_ * 4 + 3)] == bytes(48) and D[49 * (np_ * 4 + 2):49 * (np_ * 4 + 3)] == C[49 * 2:49 * 3]


def test_c_records_at_infinity_and_outside_g1(ctx, op):
    wd = mh.World(op, 6004, 4)
    t, np_, pub_idx = 3, 6, (1, 3)
    creds = creds_of(op, wd, (0, 2), t, np_, 2, 11200)
    C, pub48, rnd = creds[1]
    rec = lambda i, new: C[:49 * i] + new + C[49 * i + 49:]
    pt = lambda i: op.dec(C[49 * i:49 * i + 49])[0]
    t3, t11, te = enc96(point_of_order(3)), enc96(point_of_order(11)), enc96(eigenpoint(10177)[0])
    for i in (0, 2, 4):
        creds.append((rec(i, bytes(49)), pub48, rnd))
        creds.append((rec(i, op.enc(op.add(pt(i), t3))), pub48, rnd))
        creds.append((rec(i, op.enc(op.add(pt(i), t11))), pub48, rnd))
    creds.append((rec(1, op.enc(te)), pub48, rnd))
    creds.append((rec(5, b"\x00" + bytes(range(1, 49))), pub48, rnd))
    creds.append((bytes(49 * np_), pub48, rnd))
    _, _, _, st = check(ctx, op, wd, pub_idx, t, np_, creds)
    assert st == bytes(len(creds))


@pytest.mark.parametrize("kind", ["order 3 added", "eigenpoint", "infinity"])
def test_public_h_outside_g1(ctx, op, kind):
    base = mh.World(op, 6004, 4)
    h = {"order 3 added": {3: op.add(base.h[3], enc96(point_of_order(3)))}, "eigenpoint": {1: enc96(eigenpoint(10177)[0])}, "infinity": {3: bytes(96)}}[kind]
    wd = mh.World(op, 6004, 4, h=h)
    check(ctx, op, wd, (1, 3), 3, 6, creds_of(op, wd, (0, 2), 3, 6, 3, 11300))


def test_bad_lanes_beside_good_ones(ctx, op):
    wd = mh.World(op, 6004, 4)
    t, np_, pub_idx = 3, 6, (1, 3)
    creds = creds_of(op, wd, (0, 2), t, np_, 3, 11400)
    C, pub48, rnd = creds[0]
    rec = lambda i, new: C[:49 * i] + new + C[49 * i + 49:]
    for i in (0, 2, 3, 5):                                                                   # among the first t and behind them: every record is parsed
        creds.insert(1, (rec(i, mh.off_curve_x()), pub48, rnd))
        creds.append((rec(i, b"\x05" + C[49 * i + 1:49 * i + 49]), pub48, rnd))
    for k in range(2):
        creds.insert(2, (C, mh.field(pub48, k, R), rnd))
        creds.append((C, mh.field(pub48, k, (1 << 384) - 1), rnd))
    A, es, D, st = check(ctx, op, wd, pub_idx, t, np_, creds)
    assert st.count(0xff) == 12 and st.count(0) == 3
    j = st.index(0xff)
    assert A[49 * j:49 * j + 49] == b"\xff" * 49 and es[48 * np_ * j:48 * np_ * (j + 1)] == b"\xff" * (48 * np_) and D[49 * np_ * j:49 * np_ * (j + 1)] == b"\xff" * (49 * np_)


def test_sk_and_public_records(ctx, op):
    """sk = r (and above): every byte 0xff and C12381_E_ARG; an undecodable pp or used h: every byte 0xff and C12381_E_POINT; a private h record is not read"""
    from types import SimpleNamespace
    from crypto12381_amd.capi import C12381Error, E_ARG, E_POINT
    wd = mh.World(op, 6004, 4)
    t, np_, pub_idx = 3, 6, (1, 3)
    creds = creds_of(op, wd, (0, 2), t, np_, 3, 11500)
    sk = mh.b48(wd.gamma)
    good = check(ctx, op, wd, pub_idx, t, np_, creds)
    ff = tuple(b"\xff" * len(g) for g in good)
    for bad_sk in (mh.b48(R), mh.b48((1 << 384) - 1), mh.b48(1 << 256)):
        assert mi.expected_iss(op, wd.pp, wd.h49, bad_sk, pub_idx, t, np_, *creds[0]) is None
        with pytest.raises(C12381Error) as e:
            run(ctx, wd, bad_sk, pub_idx, t, np_, creds)
        assert e.value.code == E_ARG
        with pytest.raises(C12381Error) as e:
            run(ctx, wd, bad_sk, pub_idx, t, np_, creds, dev=True)
        assert e.value.code == E_ARG
        assert run(ctx, wd, sk, pub_idx, t, np_, creds) == good
    assert check(ctx, op, wd, pub_idx, t, np_, creds, sk48=mh.b48(R - 1))[3] == bytes(3)
    assert check(ctx, op, wd, pub_idx, t, np_, creds, sk48=bytes(48))[3] == bytes(3)
    unread = SimpleNamespace(pp=wd.pp, h49=mh.off_curve_x() + wd.h49[49:])
    assert run(ctx, unread, sk, pub_idx, t, np_, creds) == good
    for pp, h49 in ((b"\x05" + wd.pp[1:], wd.h49), (wd.pp[:49] + b"\x04" + wd.pp[50:], wd.h49), (wd.pp, wd.h49[:49] + mh.off_curve_x() + wd.h49[98:]),
                    (wd.pp, wd.h49[:147] + mh.off_curve_x())):
        bad = SimpleNamespace(pp=pp, h49=h49)
        assert mi.expected_iss(op, pp, h49, sk, pub_idx, t, np_, *creds[0]) is None
        for dev in (False, True):
            assert run(ctx, bad, sk, pub_idx, t, np_, creds, strict=False, dev=dev) == ff
        with pytest.raises(C12381Error) as e:
            run(ctx, bad, sk, pub_idx, t, np_, creds)
        assert e.value.code == E_POINT
        assert run(ctx, wd, sk, pub_idx, t, np_, creds) == good


def test_more_than_one_block(ctx, op):
    """70 credentials of 6 parties: 420 lanes; a bad credential among the tiled ones"""
    wd = mh.World(op, 6004, 4)
    t, np_, pub_idx = 3, 6, (1, 3)
    creds = creds_of(op, wd, (0, 2), t, np_, 5, 11600)
    creds.append((creds[0][0][:49 * 4] + mh.off_curve_x() + creds[0][0][49 * 5:], creds[0][1], creds[0][2]))
    sk = mh.b48(wd.gamma)
    rows = [mi.expected_iss(op, wd.pp, wd.h49, sk, pub_idx, t, np_, *c) for c in creds]
    idx = [(5 * j) % 6 for j in range(70)]
    want = tuple(b"".join(rows[i][k] for i in idx) for k in range(3)) + (bytes(rows[i][3] for i in idx),)
    mi.both(lambda dev: run(ctx, wd, sk, pub_idx, t, np_, [creds[i] for i in idx], dev=dev), want)
