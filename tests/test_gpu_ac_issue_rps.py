"""c12381_ac_rps_issue_batch and c12381_ac_rps_user_keygen_batch: issue and user_keygen of the reference's examples/AC-rps from the wire formats and the
caller's randomness.  The records and statuses of the host and the _dev form equal tests/ac_issue_cases.py's expected functions (term by term on the
CPU oracle) on every lane: nattr = 1, 2, 4, 31, 32 with the whole lane list (valid; alpha = 0, r, 2^256 - 1; all attributes 0; x + ym = 0; sigma at
infinity; upk at infinity, outside G1, a leading 0x00 with bytes behind it; upk with a bad tag and off the curve; an attribute = r); the list tiled to
2^12 + 1 and to 2^18 + 3 lanes, the second chunk; y = 0, 1, r - 1 and x = 0; g outside G1 — where h^(x + ym) is not g^(alpha (x + ym)) — and at infinity;
tilde_Y[i] outside G2 and at infinity; key records that do not decode, read and unread; sk fields = r.  user_keygen: rnd = 0, 1, r - 1, r, 2^256 - 1 under
the same g variants, and a pk that does not decode."""
import pytest

import ac_bbs_cases as ab
import ac_issue_cases as ai
import ac_rps_cases as arp
import mhac_iss_cases as mi
from ac_bbs_cases import b48
from g1_torsion import enc as enc96, eigenpoint, point_of_order
from util import R, prng

from crypto12381_amd.capi import C12381Error, E_ARG, E_POINT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = mi.ctx_fixture()
    yield c
    c.close()


@pytest.fixture(scope="module")
def op(oracle_port):
    return ab.Ops(oracle_port)


def run(ctx, sk, pk, tY97, lanes, **kw):
    return ctx.ac_rps_issue(sk, pk, tY97, *ai.pack(lanes), **kw)


def check(ctx, op, key, lanes, sk=None, tY97=None):
    sk, tY97 = key.sk if sk is None else sk, key.tY97 if tY97 is None else tY97
    want = ai.want_rps(op, key, lanes, sk, tY97)
    mi.both(lambda dev: run(ctx, sk, key.pk, tY97, lanes, dev=dev), want)
    assert want[1] == bytes(ln.status for ln in lanes)
    return want


def g_variants(op, base_g):
    t3, te = enc96(point_of_order(3)), enc96(eigenpoint(10177)[0])
    return {"g + order 3": op.add(base_g, t3), "g eigenpoint": te, "g at infinity": bytes(96)}


@pytest.mark.parametrize("nattr", ai.NATTRS)
def test_every_lane_of_the_list(ctx, op, nattr):
    key = ai.rps_key(op, 9100 + nattr, nattr)
    lanes = ai.rps_lanes(op, key.g, key.x, key.y, nattr, 9200 + nattr)
    sig, st = check(ctx, op, key, lanes)
    kinds = [ln.kind for ln in lanes]
    rec = lambda kind: sig[195 * kinds.index(kind):195 * kinds.index(kind) + 195]
    assert rec("alpha = 0")[:98] == bytes(98) and rec("all a = 0")[98:] == bytes(97) and rec("sigma at infinity")[49:98] == bytes(49)
    assert st.count(0xff) == 3 and rec("upk off curve") == b"\xff" * 195


@pytest.mark.parametrize("nattr,n", [(4, (1 << 12) + 1), (2, (1 << 18) + 3)])
def test_the_list_tiled_over_blocks_and_into_the_second_chunk(ctx, op, nattr, n):
    key = ai.rps_key(op, 9300 + nattr, nattr)
    lanes = ai.rps_lanes(op, key.g, key.x, key.y, nattr, 9400)
    rows = [ai.expected_rps_issue(op, key.sk, key.pk, key.tY97, nattr, ln.upk, ln.attr, ln.rnd) for ln in lanes]
    L = len(lanes)
    want = ai.tile([r[0] for r in rows], n), bytes(rows[i % L][1] for i in range(n))
    upk, attr, rnd = (ai.tile([getattr(ln, f) for ln in lanes], n) for f in ("upk", "attr", "rnd"))
    mi.both(lambda dev: ctx.ac_rps_issue(key.sk, key.pk, key.tY97, upk, attr, rnd, dev=dev), want)


@pytest.mark.parametrize("x,y", [(None, 0), (None, 1), (None, R - 1), (0, None), (0, 0), (R - 1, R - 1)])
def test_the_ends_of_the_range_of_sk(ctx, op, x, y):
    key = ai.rps_key(op, 9500, 4)
    x, y = key.x if x is None else x, key.y if y is None else y
    check(ctx, op, key, ai.rps_lanes(op, key.g, x, y, 4, 9510), sk=b48(x) + b48(y))


def test_another_key_and_back(ctx, op):
    k1, k2 = ai.rps_key(op, 9520, 4), ai.rps_key(op, 9521, 4)
    l1, l2 = (ai.rps_lanes(op, k.g, k.x, k.y, 4, 9530 + i) for i, k in enumerate((k1, k2)))
    first = check(ctx, op, k1, l1)
    assert check(ctx, op, k2, l2) != first
    assert check(ctx, op, k1, l1) == first


@pytest.mark.parametrize("kind", ["g + order 3", "g eigenpoint", "g at infinity", "tilde_Y1 outside G2", "tilde_Y3 at infinity", "tilde_Y0 outside G2"])
def test_keys_outside_the_subgroups_and_at_infinity(ctx, op, kind):
    base = ai.rps_key(op, 9600, 4)
    kw = {k: dict(g=v) for k, v in g_variants(op, base.g).items()}
    kw.update({"tilde_Y1 outside G2": dict(tilde_Y={1: ab.g2_outside()}), "tilde_Y3 at infinity": dict(tilde_Y={3: bytes(192)}),
               "tilde_Y0 outside G2": dict(tilde_Y={0: arp.g2add(op, base.tilde_Y[0], ab.g2_outside())})})
    key = ai.rps_key(op, 9600, 4, **kw[kind])
    lanes = ai.rps_lanes(op, key.g, key.x, key.y, 4, 9610)
    sig, st = check(ctx, op, key, lanes)
    if kind == "g + order 3":                                                                 # the lane a merged exponent would miss
        ln = lanes[0]
        a, alpha = ab._fields(ln.attr, 4), int.from_bytes(ln.rnd, "big") % R
        e1 = (key.x + sum(a[i] * pow(key.y, i + 1, R) for i in range(4))) % R
        merged = op.add(op.mul(key.g, alpha * e1 % R), op.mul(op.dec(ln.upk)[0], alpha * pow(key.y, 5, R) % R))
        assert sig[49:98] != op.enc(merged)
    check(ctx, op, base, ai.rps_lanes(op, base.g, base.x, base.y, 4, 9620))


def test_key_records_that_do_not_decode(ctx, op):
    key = ai.rps_key(op, 9700, 4)
    lanes = ai.rps_lanes(op, key.g, key.x, key.y, 4, 9710)
    good = check(ctx, op, key, lanes)
    ff = tuple(b"\xff" * len(g) for g in good)
    rec = lambda i, new: key.tY97[:97 * i] + new + key.tY97[97 * (i + 1):]
    # tilde_Y[nattr] is never read
    mi.both(lambda dev: run(ctx, key.sk, key.pk, rec(4, ai.bad_g2(key.tY97[97 * 4:])), lanes, dev=dev), good)
    cases = [(key.pk, rec(0, ai.bad_g2(key.tY97[:97]))), (key.pk, rec(3, ai.bad_g2(key.tY97[97 * 3:97 * 4]))), (ab.off_curve_x() + key.pk[49:], key.tY97),
             (key.pk[:49] + ai.bad_g2(key.pk[49:146]) + key.pk[146:], key.tY97), (key.pk[:146] + ai.bad_g2(key.pk[146:]), key.tY97)]
    for pk, tY97 in cases:
        assert ai.key_failure(op, "rps", key.sk, pk, tY97, 4) == "point"
        for dev in (False, True):
            assert run(ctx, key.sk, pk, tY97, lanes, strict=False, dev=dev) == ff
            with pytest.raises(C12381Error) as e:
                run(ctx, key.sk, pk, tY97, lanes, dev=dev)
            assert e.value.code == E_POINT
        assert ctx.sync() == 0
        assert run(ctx, key.sk, key.pk, key.tY97, lanes) == good


def test_sk_out_of_range(ctx, op):
    key = ai.rps_key(op, 9800, 2)
    lanes = ai.rps_lanes(op, key.g, key.x, key.y, 2, 9810)
    good = check(ctx, op, key, lanes)
    n = len(lanes)
    ins = lambda sk, pk=key.pk: [sk, pk, key.tY97[:97 * 2], *ai.pack(lanes)]
    for sk in (b48(R) + key.sk[48:], key.sk[:48] + b48(R), key.sk[:48] + b48((1 << 384) - 1)):
        assert ai.key_failure(op, "rps", sk, key.pk, key.tY97, 2) == "arg"
        rc, rs, outs = ai.raw(ctx, "c12381_ac_rps_issue_batch", (n, 2), ins(sk), [195 * n, n], dev=False)
        assert (rc, rs) == (E_ARG, 0) and outs == (b"\xff" * (195 * n), b"\xff" * n)
        rc, rs, outs = ai.raw(ctx, "c12381_ac_rps_issue_batch", (n, 2), ins(sk), [195 * n, n], dev=True)
        assert (rc, rs) == (0, E_ARG) and outs == (b"\xff" * (195 * n), b"\xff" * n)
        assert ctx.sync() == 0
        assert run(ctx, key.sk, key.pk, key.tY97, lanes) == good


@pytest.mark.parametrize("kind", ["honest", "g + order 3", "g eigenpoint", "g at infinity"])
def test_user_keygen(ctx, op, kind):
    base = ai.rps_key(op, 9900, 2)
    key = base if kind == "honest" else ai.rps_key(op, 9900, 2, g=g_variants(op, base.g)[kind])
    vals = list(ai.KEYGEN_RND) + [prng(9910, i, 32) for i in range(4)]
    n = (1 << 8) + 3                                                                         # more than one block
    rows = [ai.expected_user_keygen(op, key.pk, ai.b32raw(v))[0] for v in vals]
    want = ai.tile([r[0] for r in rows], n), ai.tile([r[1] for r in rows], n)
    rnd = ai.tile([ai.b32raw(v) for v in vals], n)
    mi.both(lambda dev: ctx.ac_rps_user_keygen(key.pk, rnd, dev=dev), want)
    assert want[0][:48] == bytes(48) == want[0][48 * 3:48 * 4]                               # rnd = 0 and rnd = r: usk = 0
    if kind == "honest":                                                                     # outside G1 multiply(g, 0) is whatever the reference makes of it
        assert want[1][:49] == bytes(49) == want[1][49 * 3:49 * 4] and rows[1] == (b48(1), op.enc(key.g))


def test_user_keygen_with_a_pk_that_does_not_decode(ctx, op):
    key = ai.rps_key(op, 9900, 2)
    rnd = ai.tile([ai.b32raw(v) for v in ai.KEYGEN_RND], 7)
    good = ctx.ac_rps_user_keygen(key.pk, rnd)
    for pk in (ab.off_curve_x() + key.pk[49:], key.pk[:49] + ai.bad_g2(key.pk[49:146]) + key.pk[146:], key.pk[:146] + ai.bad_g2(key.pk[146:])):
        assert ai.expected_user_keygen(op, pk, rnd[:32]) is None
        for dev in (False, True):
            assert ctx.ac_rps_user_keygen(pk, rnd, strict=False, dev=dev) == (b"\xff" * (48 * 7), b"\xff" * (49 * 7))
            with pytest.raises(C12381Error) as e:
                ctx.ac_rps_user_keygen(pk, rnd, dev=dev)
            assert e.value.code == E_POINT
        assert ctx.sync() == 0
        assert ctx.ac_rps_user_keygen(key.pk, rnd) == good
