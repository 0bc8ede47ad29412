"""c12381_mhac_bbs_pres_batch: MHAC-bbs presentations (the reference's examples/MHAC-bbs/src/cred_pres.cpp) from the wire formats and the caller's
randomness.  Every output byte equals tests/mhac_bbs_cases.py's expected_pres (one flat loop over the reference's terms by the CPU oracle), in the
host and the _dev form, and every presentation is fed back through c12381_mhac_bbs_verify_batch.  t = 1 (no beta_share, two per-lane powers),
t = 3, t = 4 (five powers: the first split into two products), t = 8 (nine powers, three products); the list bound (m = 4, Prv = all, Rev = (),
t = 8 fills 32 positions; m = 5, Prv = (0, 1, 2, 3), t = 8 is 33 and refused); an h record outside G1 at a used position, where the repeated-base
terms must not be merged; A off the subgroup; r = 0; 0xff lanes beside good ones; undecodable public records."""
import pytest

import mhac_bbs_cases as mh
from g1_torsion import enc as enc96, eigenpoint, point_of_order
from util import R

pytestmark = pytest.mark.gpu
NAMES = ("A49", "D49", "lam48", "es48", "as48", "crev49", "cpub49", "pub48", "rnd")


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


def inputs(op, wd, Prv, Rev, t, count, seed, **kw):
    """`count` holders' wire records with their randomness; the first draw has values at and above r (reduced first)"""
    out = []
    for i in range(count):
        hd = mh.Holder(op, wd, Prv, Rev, t, seed + 100 * i, **kw)
        vals = mh.draw(seed + 100 * i + 50, mh.rnd_count(wd.m, Prv, Rev, t))
        if i == 0:
            vals = ([R + 5, (1 << 256) - 1] + vals[2:])[:len(vals)]
        out.append((hd, hd.pres_inputs(op, vals)))
    return out


def run(ctx, wd, Prv, Rev, t, ins, **kw):
    cols = [b"".join(i[name] for i in ins) for name in NAMES]
    return ctx.mhac_bbs_pres(wd.pp, wd.h49, Prv, Rev, t, *cols, **kw)


def expect(op, wd, Prv, Rev, t, ins):
    rows = [mh.expected_pres(op, wd.pp, wd.h49, Prv, Rev, t, **i) for i in ins]
    return tuple(b"".join(r[k] for r in rows) for k in range(3)) + (bytes(r[3] for r in rows),)


def check(ctx, op, wd, Prv, Rev, t, made, verify=True):
    """host and _dev bytes equal expected_pres; every good presentation goes back through the verify entry and gets expected_verify's byte"""
    ins = [i for _, i in made]
    want = expect(op, wd, Prv, Rev, t, ins)
    assert run(ctx, wd, Prv, Rev, t, ins) == want
    assert run(ctx, wd, Prv, Rev, t, ins, dev=True) == want
    fixed, z, zhp, st = want
    nP, nhp = len(Prv), len(mh.sets(wd.m, Prv, Rev)[2])
    lanes = [mh.Lane("made", i["crev49"], fixed[242 * j:242 * j + 242], z[48 * nP * j:48 * nP * (j + 1)], zhp[48 * nhp * j:48 * nhp * (j + 1)],
                     b"".join(mh.b48(v) for v in hd.revealed)) for j, (hd, i) in enumerate(made) if st[j] == 0]
    if verify and lanes:
        got = ctx.mhac_bbs_verify(wd.pp, wd.h49, wd.pk, Prv, Rev, *mh.pack(lanes))
        assert got == mh.expect(op, wd, Prv, Rev, lanes)
        return got
    return b""


@pytest.mark.parametrize("t", [1, 3, 4, 8])
def test_small_world(ctx, op, t):
    wd = mh.World(op, 6000, mh.M_MAIN)
    made = inputs(op, wd, mh.PRV_MAIN, mh.REV_MAIN, t, 3, 7400 + t)
    assert check(ctx, op, wd, mh.PRV_MAIN, mh.REV_MAIN, t, made) == b"\x01\x01\x01"


@pytest.mark.parametrize("m,Prv,Rev,t", [(4, (), (1,), 3), (4, (0, 1, 2, 3), (), 3), (4, (0, 2), (), 2), (4, (2, 0), (1,), 3), (4, (0, 2), (1, 3), 3), (1, (), (0,), 1),
                                         (1, (0,), (), 2), (32, (0, 1), (5, 31, 17), 2), (16, (0, 1, 2, 3), (7,), 3)])
def test_further_shapes(ctx, op, m, Prv, Rev, t):
    wd = mh.World(op, 6600 + m, m)
    check(ctx, op, wd, Prv, Rev, t, inputs(op, wd, Prv, Rev, t, 2, 7500))


def test_the_list_bound(ctx, op):
    """nHid + (t - 1) nPrv positions: 4 + 7 x 4 = 32 fills the list, 5 + 7 x 4 = 33 is refused before anything runs"""
    from crypto12381_amd.capi import C12381Error, E_ARG
    wd = mh.World(op, 6604, 4)
    assert check(ctx, op, wd, (0, 1, 2, 3), (), 8, inputs(op, wd, (0, 1, 2, 3), (), 8, 2, 7600)) == b"\x01\x01"
    wd5 = mh.World(op, 6605, 5)
    made = inputs(op, wd5, (0, 1, 2, 3), (), 8, 1, 7600)
    with pytest.raises(C12381Error) as e:
        run(ctx, wd5, (0, 1, 2, 3), (), 8, [i for _, i in made])
    assert e.value.code == E_ARG
    check(ctx, op, wd5, (0, 1, 2, 3), (), 7, inputs(op, wd5, (0, 1, 2, 3), (), 7, 1, 7600))      # 5 + 6 x 4 = 29


@pytest.mark.parametrize("kind", ["private h + order 3", "private h eigenpoint", "hidden public h + order 3", "hidden h at infinity"])
def test_h_outside_g1(ctx, op, kind):
    """a used h record outside G1: the sum runs position by position through the generic kernel.  h[Prv[ii]] stands at t positions of the list (once
    under beta_share_j, t - 1 times under beta_share); multiply is not additive in the scalar off the subgroup, so one power of the summed exponents
    would be another point — expected_pres multiplies term by term"""
    t3 = enc96(point_of_order(3))
    base = mh.World(op, 6800, mh.M_MAIN)
    h = {"private h + order 3": {2: op.add(base.h[2], t3)}, "private h eigenpoint": {0: enc96(eigenpoint(10177)[0])},
         "hidden public h + order 3": {3: op.add(base.h[3], t3)}, "hidden h at infinity": {3: bytes(96)}}[kind]
    wd = mh.World(op, 6800, mh.M_MAIN, h=h)
    check(ctx, op, wd, mh.PRV_MAIN, mh.REV_MAIN, 3, inputs(op, wd, mh.PRV_MAIN, mh.REV_MAIN, 3, 3, 7700))


def test_merged_exponents_would_differ(op):
    """the premise of the case above, on the CPU oracle: for h = H + T (T of order 3) the powers under b0 and b1 do not add up to the power under b0 + b1
    for some pair of small scalars"""
    h = op.add(mh.World(op, 6800, 1).h[0], enc96(point_of_order(3)))
    assert any(op.add(op.mul(h, a), op.mul(h, b)) != op.mul(h, a + b) for a in range(1, 4) for b in range(1, 4))


def test_degenerate_lanes(ctx, op):
    """A off the subgroup (an order-3 point added; an eigenpoint), A at infinity, r = 0 (A_ = B_ = infinity), lambda = 0 and e = 0"""
    wd = mh.World(op, 6000, mh.M_MAIN)
    Prv, Rev, t = mh.PRV_MAIN, mh.REV_MAIN, 3
    made = inputs(op, wd, Prv, Rev, t, 2, 7800)
    hd, ins = made[1]
    zero_r = dict(ins, rnd=bytes(32) + ins["rnd"][32:])
    made.append((hd, zero_r))
    made.append((hd, dict(ins, A49=op.enc(op.add(hd.A, enc96(point_of_order(3)))))))
    made.append((hd, dict(ins, A49=op.enc(enc96(eigenpoint(10177)[0])))))
    made.append((hd, dict(ins, A49=bytes(49))))
    made.append((hd, dict(ins, A49=b"\x00" + bytes(range(1, 49)))))
    made.append((hd, dict(ins, lam48=mh.field(ins["lam48"], 1, 0), es48=mh.field(ins["es48"], 0, 0))))
    got = check(ctx, op, wd, Prv, Rev, t, made)
    assert got[:3] == b"\x01\x01\x01"
    want = expect(op, wd, Prv, Rev, t, [zero_r])
    assert want[0][0] == 0 and want[0][49] == 0


def test_bad_lanes_beside_good_ones(ctx, op):
    wd = mh.World(op, 6000, mh.M_MAIN)
    Prv, Rev, t = mh.PRV_MAIN, mh.REV_MAIN, 3
    made = inputs(op, wd, Prv, Rev, t, 3, 7900)
    hd, ins = made[0]
    for name in ("A49", "D49", "crev49", "cpub49"):
        made.insert(1, (hd, dict(ins, **{name: b"\x05" + ins[name][1:]})))
        made.append((hd, dict(ins, **{name: mh.off_curve_x()})))
    for name, count in (("lam48", 3), ("es48", 3), ("as48", 6), ("pub48", 2)):
        made.insert(2, (hd, dict(ins, **{name: mh.field(ins[name], count - 1, R)})))
        made.append((hd, dict(ins, **{name: mh.field(ins[name], 0, (1 << 384) - 1)})))
    want = expect(op, wd, Prv, Rev, t, [i for _, i in made])
    assert want[3].count(0xff) == 16 and want[3].count(0) == 3
    assert check(ctx, op, wd, Prv, Rev, t, made) == b"\x01\x01\x01"


def test_public_records(ctx, op):
    """an undecodable pp or used h: every byte 0xff and C12381_E_POINT; an undecodable record at the revealed position is not read"""
    from types import SimpleNamespace
    from crypto12381_amd.capi import C12381Error, E_POINT
    wd = mh.World(op, 6000, mh.M_MAIN)
    Prv, Rev, t = mh.PRV_MAIN, mh.REV_MAIN, 3
    ins = [i for _, i in inputs(op, wd, Prv, Rev, t, 3, 8000)]
    good = expect(op, wd, Prv, Rev, t, ins)
    unread = SimpleNamespace(m=4, pp=wd.pp, h49=wd.h49[:49] + mh.off_curve_x() + wd.h49[98:])
    assert run(ctx, unread, Prv, Rev, t, ins) == good
    for pp, h49 in ((b"\x05" + wd.pp[1:], wd.h49), (wd.pp[:49] + b"\x04" + wd.pp[50:], wd.h49), (wd.pp, wd.h49[:147] + mh.off_curve_x()),
                    (wd.pp, mh.off_curve_x() + wd.h49[49:])):
        bad = SimpleNamespace(m=4, pp=pp, h49=h49)
        assert mh.expected_pres(op, pp, h49, Prv, Rev, t, **ins[0]) is None
        assert run(ctx, bad, Prv, Rev, t, ins, strict=False) == (b"\xff" * (242 * 3), b"\xff" * (96 * 3), b"\xff" * (48 * 3), b"\xff" * 3)
        with pytest.raises(C12381Error) as e:
            run(ctx, bad, Prv, Rev, t, ins)
        assert e.value.code == E_POINT
        assert run(ctx, wd, Prv, Rev, t, ins) == good                                # the context recovers


def test_large_tiled_host_and_dev(ctx, op):
    wd = mh.World(op, 6000, mh.M_MAIN)
    Prv, Rev, t = mh.PRV_MAIN, mh.REV_MAIN, 3
    ins = [i for _, i in inputs(op, wd, Prv, Rev, t, 12, 8100)]
    ins.append(dict(ins[0], D49=b"\x05" + ins[0]["D49"][1:]))
    ins.append(dict(ins[1], pub48=mh.field(ins[1]["pub48"], 1, R)))
    rows = [mh.expected_pres(op, wd.pp, wd.h49, Prv, Rev, t, **i) for i in ins]
    n = (1 << 12) + 1
    idx = [(j * 5) % len(ins) for j in range(n)]
    want = tuple(b"".join(rows[i][k] for i in idx) for k in range(3)) + (bytes(rows[i][3] for i in idx),)
    tiled = [ins[i] for i in idx]
    assert run(ctx, wd, Prv, Rev, t, tiled) == want
    assert run(ctx, wd, Prv, Rev, t, tiled, dev=True) == want
