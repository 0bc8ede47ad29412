"""c12381_ac_rbbs_redact_batch: AC-rbbs redact caches (the reference's examples/AC-rbbs/src/redact.cpp) from the wire formats: every output byte
equals redact composed from the CPU oracle's primitives and hashlib (tests/ac_rbbs_cases.py expected_redact: D over exactly the k the reference's
filter keeps).  Shapes: nattr = 1, 2, 4, 16, I empty, all, unordered with several i per k; lanes: honest credentials, attributes at 0, 1, r - 1,
A at infinity and outside G1, w = 0, A not decodable and w or an attribute >= r (0xff records, the other lanes unaffected); keys: a second key
and back, g and records of Y outside G1 in every part of the base list (the generic route, exact term by term), any undecodable record of Y
(every lane 0xff, C12381_E_POINT, the context usable afterwards); one tiled run of 2^12 + 1 lanes in host and _dev form and a second chunk."""
from types import SimpleNamespace

import pytest

import ac_rbbs_cases as rc
from g1_torsion import enc as enc96, point_of_order
from util import R

pytestmark = pytest.mark.gpu


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
    return rc.Ops(oracle_port)


def attrs(vals):
    return b"".join(rc.b48(v) for v in vals)


def lanes_of(op, key, I, seed=6400):
    """(attr_48 span, sig_97) per lane"""
    n = key.nattr
    creds = [rc.Cred(op, key, I, seed, i) for i in range(3)]
    out = [(c.attr_all, c.sig) for c in creds]
    c = creds[0]
    for vals in ([0] * n, [1] * n, [R - 1] * n, [(0, 1, R - 1)[k % 3] for k in range(n)]):
        out.append((attrs(vals), c.sig))
    out.append((c.attr_all, bytes(49) + c.sig[49:]))                                        # A at infinity
    out.append((c.attr_all, c.sig[:49] + bytes(48)))                                        # w = 0
    out.append((c.attr_all, op.enc(op.add(op.dec(c.sig[:49])[0], enc96(point_of_order(3)))) + c.sig[49:]))
    out.append((c.attr_all, b"\x05" + c.sig[1:]))                                           # where the reference would throw
    out.append((c.attr_all, rc.off_curve_x() + c.sig[49:]))
    out.append((c.attr_all, c.sig[:49] + rc.b48(R)))
    out.append((c.attr_all[:48 * (n - 1)] + rc.b48(R), c.sig))
    out.append((rc.b48((1 << 384) - 1) + c.attr_all[48:], c.sig))
    out.append(out[1])
    return out


def expected(op, key, I, lanes):
    res = [rc.expected_redact(op, key.pk, key.Y49, key.nattr, I, a, s) for a, s in lanes]
    return b"".join(c for c, _ in res), bytes(s for _, s in res)


def call(ctx, key, I, lanes, **kw):
    return ctx.ac_rbbs_redact(key.pk, key.Y49, I, b"".join(a for a, _ in lanes), b"".join(s for _, s in lanes), **kw)


def check(ctx, op, key, I, lanes):
    (got_c, got_s), (want_c, want_s) = call(ctx, key, I, lanes), expected(op, key, I, lanes)
    assert got_s == want_s
    bad = [j for j in range(len(lanes)) if got_c[196 * j:196 * j + 196] != want_c[196 * j:196 * j + 196]]
    assert not bad, bad
    return want_c, want_s


@pytest.mark.parametrize("nattr,I", rc.SHAPES + [(16, (15, 7, 8, 0)), (16, tuple(range(16))), (5, (4, 2))])
def test_shapes(ctx, op, nattr, I):
    key = rc.Key(op, 5200 + nattr, nattr)
    _, st = check(ctx, op, key, I, lanes_of(op, key, I))
    assert st == bytes(10) + b"\xff" * 5 + bytes(1)


def test_second_key_and_back(ctx, op):
    key, other = rc.Key(op, 5000, rc.NATTR), rc.Key(op, 5001, rc.NATTR)
    lanes = lanes_of(op, key, rc.I_MAIN)[:4]
    first = check(ctx, op, key, rc.I_MAIN, lanes)
    assert check(ctx, op, other, rc.I_MAIN, lanes) != first
    assert check(ctx, op, key, (3, 0), lanes) != first                   # another set under the same key
    assert call(ctx, key, rc.I_MAIN, lanes) == first
    assert call(ctx, key, rc.I_MAIN, lanes) == first                     # the same key and set again: the cached tables


@pytest.mark.parametrize("k", ["g", 0, 1, 2, 3, 5, 7])
def test_generic_routes(ctx, op, k):
    """g or one record of Y outside G1.  K_D = {2, 3, 5, 6} here: 0 is in I alone, 3 in I and K_D, 1 in J alone, 2 in J and K_D, 5 above nattr,
    7 in no sum.  The fixed-base sums that hold the record fall back to the generic kernel column by column, and the result equals the reference's
    product term by term"""
    t3 = enc96(point_of_order(3))
    base = rc.Key(op, 5600, rc.NATTR)
    key = rc.Key(op, 5600, rc.NATTR, g=op.add(base.g, t3)) if k == "g" else rc.Key(op, 5600, rc.NATTR, Y={k: op.add(base.Y[k], t3)})
    check(ctx, op, key, rc.I_MAIN, lanes_of(op, key, rc.I_MAIN, 6500)[:8])


def test_undecodable_key(ctx, op):
    from crypto12381_amd.capi import C12381Error, E_POINT
    key = rc.Key(op, 5000, rc.NATTR)
    lanes = lanes_of(op, key, rc.I_MAIN)[:3]
    good = call(ctx, key, rc.I_MAIN, lanes)
    bad49 = rc.off_curve_x()
    keys = [(b"\x05" + key.pk[1:], key.Y49), (key.pk[:49] + b"\x04" + key.pk[50:], key.Y49)]
    keys += [(key.pk, key.Y49[:49 * k] + bad49 + key.Y49[49 * k + 49:]) for k in range(8)]         # the record at nattr, which no sum uses, included
    for pk, Y in keys:
        bad = SimpleNamespace(pk=pk, Y49=Y)
        assert rc.expected_redact(op, pk, Y, rc.NATTR, rc.I_MAIN, *lanes[0]) is None
        assert call(ctx, bad, rc.I_MAIN, lanes, strict=False) == (b"\xff" * (196 * 3), b"\xff" * 3)
        with pytest.raises(C12381Error) as e:
            call(ctx, bad, rc.I_MAIN, lanes)
        assert e.value.code == E_POINT
        assert call(ctx, key, rc.I_MAIN, lanes) == good and good[1] == bytes(3)


def test_large_tiled_host_and_dev_and_second_chunk(ctx, op):
    import torch
    key = rc.Key(op, 5000, rc.NATTR)
    lanes = lanes_of(op, key, rc.I_MAIN)
    want_c, want_s = expected(op, key, rc.I_MAIN, lanes)
    m = len(lanes)
    for n in ((1 << 12) + 1, (1 << 18) + 3):
        idx = [(j * 37) % m for j in range(n)] if n < (1 << 18) else [j % m for j in range(n)]
        a, s = b"".join(lanes[i][0] for i in idx), b"".join(lanes[i][1] for i in idx)
        want = b"".join(want_c[196 * i:196 * i + 196] for i in idx), bytes(want_s[i] for i in idx)
        assert ctx.ac_rbbs_redact(key.pk, key.Y49, rc.I_MAIN, a, s) == want
        if n > (1 << 12) + 1:
            continue
        d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda") for b in (key.pk, key.Y49, a, s)]
        d_c = torch.full((196 * n,), 7, dtype=torch.uint8, device="cuda")
        d_s = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.ac_rbbs_redact_dev(n, rc.NATTR, rc.I_MAIN, *(t.data_ptr() for t in d), d_c.data_ptr(), d_s.data_ptr())
        assert ctx.sync() == 0
        assert (bytes(d_c.cpu().numpy().tobytes()), bytes(d_s.cpu().numpy().tobytes())) == want
