"""c12381_ac_bbs_issue_batch / c12381_ac_rbbs_issue_batch: issue of the reference's examples/AC-bbs and AC-rbbs from the wire formats and the caller's
randomness.  The records and statuses of the host and the _dev form equal tests/ac_issue_cases.py's expected_bbs_issue (term by term on the CPU
oracle) on every lane: nattr = 1, 2, 4, 31, 32 with the whole lane list (valid; all attributes 0 and r - 1; an attribute = r and = 2^384 - 1; rnd = 0,
r, 2^256 - 1; w = r - x, where the inverse is 0; a sum at infinity); the list tiled to 2^12 + 1 and to 2^18 + 3 lanes, the second chunk; another key and
back; Y_i outside G1, at infinity, Y_1 = -Y_0; g outside G1 (with the w = r - x lane, where multiply(B, 0) is not infinity's encoding by assumption but
whatever the reference's multiply gives) and at infinity; key records that do not decode; sk fields = r."""
import pytest

import ac_bbs_cases as ab
import ac_issue_cases as ai
import mhac_iss_cases as mi
from ac_bbs_cases import b48
from g1_torsion import enc as enc96, eigenpoint, point_of_order
from util import R

from crypto12381_amd.capi import C12381Error, E_ARG, E_POINT

pytestmark = pytest.mark.gpu
SCHEMES = ("bbs", "rbbs")


@pytest.fixture(scope="module")
def ctx():
    c = mi.ctx_fixture()
    yield c
    c.close()


@pytest.fixture(scope="module")
def op(oracle_port):
    return ab.Ops(oracle_port)


def make_key(op, scheme, seed, nattr, **kw):
    return (ai.bbs_key if scheme == "bbs" else ai.rbbs_key)(op, seed, nattr, **kw)


def lanes_of(scheme, key, seed, honest=True):
    dlog = None if not honest else (ai.bbs_dlog if scheme == "bbs" else ai.rbbs_dlog)(key)
    return ai.bbs_lanes(key.x, dlog, key.nattr, seed)


def run(ctx, scheme, sk, pk, Y49, lanes, **kw):
    return (ctx.ac_bbs_issue if scheme == "bbs" else ctx.ac_rbbs_issue)(sk, pk, Y49, *ai.pack(lanes), **kw)


def check(ctx, op, scheme, key, lanes, Y49=None):
    Y49 = key.Y49 if Y49 is None else Y49
    want = ai.want_bbs(op, key, Y49, key.nattr, lanes)
    mi.both(lambda dev: run(ctx, scheme, key.sk, key.pk, Y49, lanes, dev=dev), want)
    assert want[1] == bytes(ln.status for ln in lanes)
    return want


@pytest.mark.parametrize("nattr", ai.NATTRS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_every_lane_of_the_list(ctx, op, scheme, nattr):
    key = make_key(op, scheme, 9100 + nattr, nattr)
    lanes = lanes_of(scheme, key, 9200 + nattr)
    sig, st = check(ctx, op, scheme, key, lanes)
    kinds = [ln.kind for ln in lanes]
    for kind in ("w = r - x", "sum at infinity"):
        j = kinds.index(kind)
        assert sig[97 * j:97 * j + 49] == bytes(49), kind
    assert st.count(0xff) == 2 and sig[97 * st.index(0xff):97 * st.index(0xff) + 97] == b"\xff" * 97


@pytest.mark.parametrize("scheme,nattr,n", [("bbs", 4, (1 << 12) + 1), ("rbbs", 4, (1 << 12) + 1), ("bbs", 2, (1 << 18) + 3)])
def test_the_list_tiled_over_blocks_and_into_the_second_chunk(ctx, op, scheme, nattr, n):
    key = make_key(op, scheme, 9300 + nattr, nattr)
    lanes = lanes_of(scheme, key, 9400)
    rows = [ai.expected_bbs_issue(op, key.sk, key.pk, key.Y49, nattr, ln.attr, ln.rnd) for ln in lanes]
    L = len(lanes)
    want = ai.tile([r[0] for r in rows], n), bytes(rows[i % L][1] for i in range(n))
    attr, rnd = ai.tile([ln.attr for ln in lanes], n), ai.tile([ln.rnd for ln in lanes], n)
    fn = ctx.ac_bbs_issue if scheme == "bbs" else ctx.ac_rbbs_issue
    mi.both(lambda dev: fn(key.sk, key.pk, key.Y49, attr, rnd, dev=dev), want)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_another_key_and_back(ctx, op, scheme):
    k1, k2 = make_key(op, scheme, 9500, 4), make_key(op, scheme, 9501, 4)
    l1, l2 = lanes_of(scheme, k1, 9510), lanes_of(scheme, k2, 9511)
    first = check(ctx, op, scheme, k1, l1)
    assert check(ctx, op, scheme, k2, l2) != first
    assert check(ctx, op, scheme, k1, l1) == first


@pytest.mark.parametrize("kind", ["Y2 + order 3", "Y1 eigenpoint", "Y3 at infinity", "Y1 = -Y0", "g + order 3", "g eigenpoint", "g at infinity"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_keys_outside_g1_and_at_infinity(ctx, op, scheme, kind):
    base = make_key(op, scheme, 9600, 4)
    t3, te = enc96(point_of_order(3)), enc96(eigenpoint(10177)[0])
    kw = {"Y2 + order 3": dict(Y={2: op.add(base.Y[2], t3)}), "Y1 eigenpoint": dict(Y={1: te}), "Y3 at infinity": dict(Y={3: bytes(96)}),
          "Y1 = -Y0": dict(Y={1: ai.neg96(base.Y[0])}), "g + order 3": dict(g=op.add(base.g, t3)), "g eigenpoint": dict(g=te),
          "g at infinity": dict(g=bytes(96))}[kind]
    key = make_key(op, scheme, 9600, 4, **kw)
    lanes = lanes_of(scheme, key, 9610, honest=False)
    sig, st = check(ctx, op, scheme, key, lanes)
    assert st.count(0) == len(lanes) - 2
    # back to the honest key: the tables of the positions that changed are rebuilt
    check(ctx, op, scheme, base, lanes_of(scheme, base, 9620))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_key_records_that_do_not_decode(ctx, op, scheme):
    key = make_key(op, scheme, 9700, 4)
    lanes = lanes_of(scheme, key, 9710)
    good = check(ctx, op, scheme, key, lanes)
    ff = tuple(b"\xff" * len(g) for g in good)
    bad49 = ab.off_curve_x()
    cases = [(key.pk, key.Y49[:49 * i] + rec + key.Y49[49 * (i + 1):]) for i, rec in ((0, bad49), (3, b"\x05" + key.Y49[49 * 3 + 1:49 * 4]))]
    cases += [(bad49 + key.pk[49:], key.Y49), (key.pk[:49] + ai.bad_g2(key.pk[49:146]) + key.pk[146:], key.Y49), (key.pk[:146] + ai.bad_g2(key.pk[146:]), key.Y49)]
    for pk, Y49 in cases:
        assert ai.expected_bbs_issue(op, key.sk, pk, Y49, 4, lanes[0].attr, lanes[0].rnd) is None
        for dev in (False, True):
            assert run(ctx, scheme, key.sk, pk, Y49, lanes, strict=False, dev=dev) == ff
            with pytest.raises(C12381Error) as e:
                run(ctx, scheme, key.sk, pk, Y49, lanes, dev=dev)
            assert e.value.code == E_POINT
        assert ctx.sync() == 0                                                               # reported once
        assert run(ctx, scheme, key.sk, key.pk, key.Y49, lanes) == good
    if scheme == "rbbs":                                                                     # behind the first nattr: never read
        for k in (4, 5, 7):
            Y49 = key.Y49[:49 * k] + bad49 + key.Y49[49 * (k + 1):]
            mi.both(lambda dev: run(ctx, scheme, key.sk, key.pk, Y49, lanes, dev=dev), good)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_sk_out_of_range(ctx, op, scheme):
    key = make_key(op, scheme, 9800, 2)
    lanes = lanes_of(scheme, key, 9810)
    good = check(ctx, op, scheme, key, lanes)
    n = len(lanes)
    bad_sks = [b48(R), b48((1 << 384) - 1)] if scheme == "bbs" else [b48(R) + key.sk[48:], key.sk[:48] + b48(R), key.sk[:48] + b48(1 << 256)]
    name = "c12381_ac_%s_issue_batch" % scheme
    for sk in bad_sks:
        assert ai.key_failure(op, "bbs", sk, key.pk, key.Y49, 2) == "arg"
        attr, rnd = ai.pack(lanes)
        rc, rs, outs = ai.raw(ctx, name, (n, 2), [sk, key.pk, key.Y49[:98], attr, rnd], [97 * n, n], dev=False)
        assert (rc, rs) == (E_ARG, 0) and outs == (b"\xff" * (97 * n), b"\xff" * n)
        rc, rs, outs = ai.raw(ctx, name, (n, 2), [sk, key.pk, key.Y49[:98], attr, rnd], [97 * n, n], dev=True)
        assert (rc, rs) == (0, E_ARG) and outs == (b"\xff" * (97 * n), b"\xff" * n)
        assert ctx.sync() == 0
        assert run(ctx, scheme, key.sk, key.pk, key.Y49, lanes) == good
    # sk >= r takes precedence over a key record that does not decode
    rc, rs, outs = ai.raw(ctx, name, (n, 2), [bad_sks[0], ab.off_curve_x() + key.pk[49:], key.Y49[:98], *ai.pack(lanes)], [97 * n, n], dev=True)
    assert (rc, rs) == (0, E_ARG) and outs[1] == b"\xff" * n and ctx.sync() == 0
    # the ends of the range are keys like any other
    for x in (0, R - 1):
        k2 = make_key(op, scheme, 9800, 2)
        k2.x, k2.sk = x, b48(x) + key.sk[48:]
        check(ctx, op, scheme, k2, ai.bbs_lanes(x, None, 2, 9820))
