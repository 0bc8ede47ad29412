"""c12381_ac_bbs_pres_batch: AC-bbs presentations (the reference's examples/AC-bbs/src/pres.cpp) from the wire formats with the caller's
randomness.  The expected bytes of every lane are pres composed from the CPU oracle's primitives (tests/ac_bbs_cases.py expected_pres); the
entry's own verify accepts every lane it made.  Shapes as in the verify tests; lanes the reference would throw on (w >= r, a hidden or a
disclosed attribute >= r, an undecodable A) are 0xff with their neighbours intact; random values at and above r are reduced first; a key
outside G1 takes the generic route; an undecodable key is C12381_E_POINT; the _dev form equals the host form."""
import pytest

import ac_bbs_cases as ac
from g1_torsion import enc as enc96, point_of_order
from util import R, prng

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
    return ac.Ops(oracle_port)


class Holder:
    """count credentials under key: attribute spans, signatures, messages and randomness as the entry takes them"""

    def __init__(self, op, key, I, count, seed, msg_len=ac.MSG_LEN):
        self.key, self.I, self.msg_len, self.nJ = key, I, msg_len, key.nattr - len(I)
        self.a = [ac.attributes(seed + 100 + j, key.nattr) for j in range(count)]
        self.attr = [b"".join(ac.b48(v) for v in a) for a in self.a]
        self.sig = [ac.issue(op, key, a, seed + 200 + j) for j, a in enumerate(self.a)]
        self.msg = [ac.message(seed, j, msg_len) for j in range(count)]
        self.rnd = [b"".join(prng(seed + 300 + j, k, 32).to_bytes(32, "big") for k in range(3 + self.nJ)) for j in range(count)]

    def expected(self, op):
        return [ac.expected_pres(op, self.key, self.I, self.attr[j], self.sig[j], self.msg[j], self.rnd[j]) for j in range(len(self.sig))]

    def run(self, ctx, **kw):
        return ctx.ac_bbs_pres(self.key.pk, self.key.Y49, self.I, b"".join(self.attr), b"".join(self.sig), b"".join(self.msg), b"".join(self.rnd),
                               self.msg_len, **kw)

    def disclosed(self):
        return b"".join(ac.b48(a[i]) for a in self.a for i in self.I)


def compare(got, want, nJ):
    pres, u, st = got
    for j, (wp, wu, ws) in enumerate(want):
        assert st[j] == ws, j
        assert pres[243 * j:243 * j + 243] == wp, j
        assert u[48 * nJ * j:48 * nJ * (j + 1)] == wu, j


@pytest.mark.parametrize("nattr,I,msg_len", [(4, (0, 3), 32), (4, (), 32), (4, (0, 1, 2, 3), 32), (4, (3, 0), 32), (1, (), 32), (1, (0,), 32), (32, (0, 3), 32),
                                             (4, (0, 3), 0)])
def test_shapes_and_round_trip(ctx, op, nattr, I, msg_len):
    h = Holder(op, ac.Key(op, 5200 + nattr, nattr), I, 3, 6000 + nattr, msg_len)
    got = h.run(ctx)
    compare(got, h.expected(op), h.nJ)
    assert got[2] == bytes(3)
    assert ctx.ac_bbs_verify(h.key.pk, h.key.Y49, I, got[0], got[1], h.disclosed(), b"".join(h.msg), msg_len) == b"\x01" * 3


def test_random_values_are_reduced(ctx, op):
    """r, alpha, beta, delta_j at 0, r - 1, r, r + 1 and 2^256 - 1"""
    h = Holder(op, ac.Key(op, 5204, 4), (0, 3), 5, 6100)
    for j, v in enumerate((0, R - 1, R, R + 1, (1 << 256) - 1)):
        h.rnd[j] = v.to_bytes(32, "big") * 5
    got = h.run(ctx)
    compare(got, h.expected(op), h.nJ)
    assert ctx.ac_bbs_verify(h.key.pk, h.key.Y49, h.I, got[0], got[1], h.disclosed(), b"".join(h.msg), 32) == ac.expect(
        op, h.key, h.I, [ac.Lane("made", h.msg[j], got[0][243 * j:243 * j + 243], got[1][96 * j:96 * j + 96], h.disclosed()[96 * j:96 * j + 96]) for j in range(5)])


def test_lanes_the_reference_throws_on(ctx, op):
    h = Holder(op, ac.Key(op, 5204, 4), (0, 3), 9, 6200)
    h.sig[1] = h.sig[1][:49] + ac.b48(R)                                          # w = r
    h.attr[3] = h.attr[3][:48] + ac.b48((1 << 384) - 1) + h.attr[3][96:]         # hidden attribute 1
    h.attr[4] = ac.b48(R) + h.attr[4][48:]                                       # disclosed attribute 0
    h.sig[6] = ac.off_curve_x() + h.sig[6][49:]                                  # A off the curve
    h.sig[7] = b"\x05" + h.sig[7][1:]                                            # A with a bad tag
    h.sig[8] = bytes(49) + ac.b48(0)                                             # A at infinity and w = 0 are values, not errors
    got, want = h.run(ctx), h.expected(op)
    assert bytes(w[2] for w in want) == bytes([0, 0xff, 0, 0xff, 0xff, 0, 0xff, 0xff, 0])
    compare(got, want, h.nJ)
    for j in (1, 3, 4, 6, 7):
        assert got[0][243 * j:243 * j + 243] == b"\xff" * 243 and got[1][96 * j:96 * j + 96] == b"\xff" * 96


def test_key_outside_g1(ctx, op):
    t3 = enc96(point_of_order(3))
    base = ac.Key(op, 5600, 4)
    for kw in (dict(g=op.add(base.g, t3)), dict(Y={2: op.add(base.Y[2], t3)})):
        h = Holder(op, ac.Key(op, 5600, 4, **kw), (0, 3), 3, 6300)
        compare(h.run(ctx), h.expected(op), h.nJ)


def test_undecodable_key(ctx, op):
    from crypto12381_amd.capi import C12381Error, E_POINT
    h = Holder(op, ac.Key(op, 5204, 4), (0, 3), 3, 6400)
    good = h.key.pk
    h.key.pk = b"\x05" + good[1:]
    assert h.run(ctx, strict=False) == (b"\xff" * (243 * 3), b"\xff" * (96 * 3), b"\xff" * 3)
    with pytest.raises(C12381Error) as e:
        h.run(ctx)
    assert e.value.code == E_POINT
    h.key.pk = good
    assert h.run(ctx)[2] == bytes(3)                                             # the context recovers


def test_dev_form_equals_host_form(ctx, op):
    import torch
    h = Holder(op, ac.Key(op, 5204, 4), (0, 3), 8, 6500)
    h.sig[5] = b"\x05" + h.sig[5][1:]
    n = 300                                                                      # more than one block
    tile = lambda xs: b"".join(xs[(j * 5) % 8] for j in range(n))
    attr, sig, msg, rnd = tile(h.attr), tile(h.sig), tile(h.msg), tile(h.rnd)
    host = ctx.ac_bbs_pres(h.key.pk, h.key.Y49, h.I, attr, sig, msg, rnd, 32)
    want = h.expected(op)
    compare(host, [want[(j * 5) % 8] for j in range(n)], h.nJ)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    d = [dev(b) for b in (h.key.pk, h.key.Y49, attr, sig, msg, rnd)]
    outs = [torch.full((k * n,), 7, dtype=torch.uint8, device="cuda") for k in (243, 96, 1)]
    torch.cuda.synchronize()
    ctx.ac_bbs_pres_dev(n, 4, h.I, 32, *(t.data_ptr() for t in d), *(t.data_ptr() for t in outs))
    assert ctx.sync() == 0
    assert tuple(bytes(t.cpu().numpy().tobytes()) for t in outs) == host


def test_second_chunk(ctx, op):
    """2^18 + 3 lanes: the batch runs in chunks of 2^18, and the second chunk reads and writes behind the first"""
    h = Holder(op, ac.Key(op, 5204, 4), (0, 3), 8, 6500)
    h.sig[5] = b"\x05" + h.sig[5][1:]
    n = (1 << 18) + 3
    rep = lambda xs: b"".join(xs) * (n // 8) + b"".join(xs[:n % 8])
    pres, u, st = ctx.ac_bbs_pres(h.key.pk, h.key.Y49, h.I, rep(h.attr), rep(h.sig), rep(h.msg), rep(h.rnd), 32)
    want = h.expected(op)
    assert (pres, u, st) == (rep([w[0] for w in want]), rep([w[1] for w in want]), rep([bytes([w[2]]) for w in want]))
