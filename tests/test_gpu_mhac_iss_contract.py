"""The argument contract of the MHAC-bbs issuance entries (include/c12381_mhac.h) in both forms: the bounds of t, nparties and m, every error of the index
sets (Prv, Rev, pub_idx, S), every null pointer and the ones that may be NULL — all checked before the empty-batch rule; n = 0 returns C12381_OK and
touches nothing.  The stream contract of the four _dev entries by the method of tests/test_gpu_stream_contract.py.  One chain on _dev buffers alone:
attr -> iss -> group (with the gather) -> type -> pres -> verify gives ok = 1 on every lane, and ok = 0 where one e_share row is taken from another
credential.  And the seam: nparties = 64, t = 2, nPrv = 1, n = 4097 — one credential past a chunk of 4096."""
import ctypes

import pytest

import mhac_bbs_cases as mh
import mhac_iss_cases as mi
from stream_cases import Idx, In, Out, ins
from util import R, prng

from crypto12381_amd.capi import E_ARG

pytestmark = pytest.mark.gpu
BUF = ctypes.create_string_buffer(1 << 16)
P = ctypes.cast(BUF, ctypes.c_void_p)
# pointer arguments behind the scalars and index arrays
NPTR = {"attr": 6, "iss": 10, "group": 8, "type": 6}
AT = dict(pp=0, h=1, rnd=2, pub=3, ashare=4, C=5)
IS = dict(pp=0, h=1, sk=2, C=3, pub=4, rnd=5, A=6, eshare=7, D=8, status=9)
GR = dict(D=0, eshare=1, ashare=2, lam=3, Dg=4, eS=5, aS=6, status=7)
TY = dict(pp=0, h=1, pub=2, crev=3, cpub=4, status=5)


@pytest.fixture(scope="module")
def ctx():
    c = mi.ctx_fixture()
    yield c
    c.close()


@pytest.fixture(scope="module")
def op(oracle_port):
    return mh.Ops(oracle_port)


def arr(I):
    return None if I is None else (ctypes.c_uint32 * max(len(I), 1))(*I)


def call(ctx, name, n, head, null=()):
    """the entry in both forms on dummy HOST buffers — every call made here returns before it touches them; null: pointer positions passed as NULL"""
    ptrs = [None if k in null else P for k in range(NPTR[name])]
    return {form: getattr(ctx.lib, "c12381_mhac_bbs_%s_batch%s" % (name, form))(ctx.h, n, *head, *ptrs) for form in ("", "_dev")}


def attr(ctx, n, m=4, t=3, np_=6, Prv=(0, 2), count=None, null=()):
    return call(ctx, "attr", n, (m, t, np_, len(Prv) if count is None else count, arr(Prv)), null)


def iss(ctx, n, m=4, t=3, np_=6, pub_idx=(1, 3), count=None, null=()):
    return call(ctx, "iss", n, (m, t, np_, len(pub_idx) if count is None else count, arr(pub_idx)), null)


def group(ctx, n, np_=6, S=(0, 2, 5), nPrv=2, t=None, null=()):
    return call(ctx, "group", n, (np_, len(S) if t is None else t, arr(S), nPrv), null)


def type_(ctx, n, m=4, Prv=(0, 2), Rev=(1,), null=(), counts=None):
    cP, cR = counts or (len(Prv), len(Rev))
    return call(ctx, "type", n, (m, cP, arr(Prv), cR, arr(Rev)), null)


bad = lambda got: set(got.values()) == {E_ARG}
ok = lambda got: set(got.values()) == {0}


@pytest.mark.parametrize("n", [0, 3])
def test_shape_errors(ctx, n):
    for t, np_ in ((0, 6), (9, 16), (3, 2), (1, 0), (1, 65), (1 << 40, 1 << 40), (8, 7)):
        assert bad(attr(ctx, n, t=t, np_=np_)) and bad(iss(ctx, n, t=t, np_=np_)), (t, np_)
    assert bad(group(ctx, n, np_=2, S=(0, 1, 2))) and bad(group(ctx, n, np_=65, S=(0,))) and bad(group(ctx, n, np_=0, S=(0,)))
    assert bad(group(ctx, n, np_=16, S=tuple(range(9)))) and bad(group(ctx, n, S=(), t=0)) and bad(group(ctx, n, nPrv=33))
    for m in (0, 33, 1 << 40):
        assert bad(attr(ctx, n, m=m, Prv=())) and bad(iss(ctx, n, m=m, pub_idx=())) and bad(type_(ctx, n, m=m, Prv=(), Rev=())), m


@pytest.mark.parametrize("n", [0, 3])
def test_index_errors(ctx, n):
    for Prv in ((4,), (0, 0), (1 << 31,), (0, 1, 2, 3, 0)):
        assert bad(attr(ctx, n, Prv=Prv)) and bad(type_(ctx, n, Prv=Prv, Rev=())), Prv
    for Rev in ((4,), (1, 1), (2,), (36,)):
        assert bad(type_(ctx, n, Rev=Rev)), Rev
    for idx in ((4,), (1, 1), (1 << 31,), (0, 1, 2, 3, 0)):
        assert bad(iss(ctx, n, pub_idx=idx)), idx
    for S in ((0, 0, 1), (0, 2, 6), (1 << 31, 0, 1), (0, 64, 1)):
        assert bad(group(ctx, n, S=S)), S
    assert bad(attr(ctx, n, Prv=None, count=2)) and bad(iss(ctx, n, pub_idx=None, count=2)) and bad(group(ctx, n, S=None, t=3))
    assert bad(type_(ctx, n, Prv=None, counts=(2, 1))) and bad(type_(ctx, n, Rev=None, counts=(2, 1)))


@pytest.mark.parametrize("n", [0, 3])
def test_null_pointers(ctx, n):
    """the small world has every count above 0: no pointer may be NULL, but the optional rows of group"""
    for k in range(6):
        assert bad(attr(ctx, n, null=(k,))) and bad(type_(ctx, n, null=(k,))), k
    for k in range(10):
        assert bad(iss(ctx, n, null=(k,))), k
    for k in (GR["D"], GR["lam"], GR["Dg"], GR["status"]):
        assert bad(group(ctx, n, null=(k,))), k
    for k in (GR["eshare"], GR["eS"], GR["ashare"], GR["aS"]):                     # one of a pair
        assert bad(group(ctx, n, null=(k,))), k
    lib = ctx.lib
    assert lib.c12381_mhac_bbs_attr_batch(None, n, 4, 3, 6, 2, arr((0, 2)), *[P] * 6) == E_ARG
    assert lib.c12381_mhac_bbs_iss_batch_dev(None, n, 4, 3, 6, 2, arr((1, 3)), *[P] * 10) == E_ARG
    assert lib.c12381_mhac_bbs_group_batch(None, n, 6, 3, arr((0, 2, 5)), 2, *[P] * 8) == E_ARG
    assert lib.c12381_mhac_bbs_type_batch_dev(None, n, 4, 2, arr((0, 2)), 1, arr((1,)), *[P] * 6) == E_ARG


def test_pointers_that_may_be_null(ctx):
    assert ok(attr(ctx, 0, Prv=(), null=(AT["ashare"],))) and ok(attr(ctx, 0, Prv=None, count=0, null=(AT["ashare"],)))
    assert bad(attr(ctx, 0, Prv=(), null=(AT["pub"],)))
    assert ok(attr(ctx, 0, Prv=(0, 1, 2, 3), null=(AT["pub"],))) and bad(attr(ctx, 0, Prv=(0, 1, 2, 3), null=(AT["ashare"],)))
    assert ok(iss(ctx, 0, pub_idx=(), null=(IS["pub"],))) and ok(iss(ctx, 0, pub_idx=None, count=0, null=(IS["pub"],)))
    assert ok(group(ctx, 0, null=(GR["eshare"], GR["eS"]))) and ok(group(ctx, 0, null=(GR["ashare"], GR["aS"])))
    assert ok(group(ctx, 0, null=(GR["eshare"], GR["eS"], GR["ashare"], GR["aS"])))
    assert ok(group(ctx, 0, nPrv=0, null=(GR["ashare"],))) and ok(group(ctx, 0, nPrv=0, null=(GR["aS"],)))      # not looked at
    assert ok(type_(ctx, 0, Prv=(0, 1, 2, 3), Rev=(), null=(TY["pub"],))) and ok(type_(ctx, 0, Prv=None, Rev=None, counts=(0, 0)))
    assert bad(type_(ctx, 0, Prv=(0, 1, 2), Rev=(), null=(TY["pub"],)))
    # the bounds themselves are accepted
    assert ok(attr(ctx, 0, m=32, t=8, np_=64, Prv=tuple(range(32)))) and ok(iss(ctx, 0, m=32, t=8, np_=64, pub_idx=tuple(range(32))))
    assert ok(attr(ctx, 0, t=1, np_=1)) and ok(group(ctx, 0, np_=64, S=(63, 0, 5, 7, 9, 11, 13, 15), nPrv=32)) and ok(group(ctx, 0, np_=1, S=(0,)))


def test_empty_batch_touches_nothing(ctx):
    BUF.raw = b"\x5a" * len(BUF.raw)
    assert ok(attr(ctx, 0)) and ok(iss(ctx, 0)) and ok(group(ctx, 0)) and ok(type_(ctx, 0))
    assert BUF.raw == b"\x5a" * len(BUF.raw) and ctx.sync() == 0


# ---------------------------------------------------------------- the stream contract of the four _dev entries
N, M, PRV, REV, T, NP, S = 5, mh.M_MAIN, mh.PRV_MAIN, mh.REV_MAIN, mh.T_MAIN, 6, (0, 2, 5)
PUB = (1, 3)


def _world(op, v):
    wd = mh.World(op, 9000 + v, M)
    return wd, mi.honest(op, wd, PRV, T, NP, N, 9300 + 1000 * v)


def _attr_row(op, v):
    wd, hon = _world(op, v)
    rnds = [ra for _, _, ra, _, _ in hon]
    args = [N, M, T, NP, len(PRV), Idx(PRV), In(wd.pp), In(wd.h49), In(b"".join(rnds)), Out(48 * 2 * N), Out(48 * 2 * NP * N), Out(49 * NP * N)]
    return args, list(mi.want_attr(op, wd, PRV, T, NP, rnds))


def _iss_row(op, v):
    wd, hon = _world(op, v)
    creds = [(a[2], pub48, ri) for a, _, _, ri, pub48 in hon]
    j = 1 if v == 0 else 3
    creds[j] = (creds[j][0], mh.field(creds[j][1], 0, R), creds[j][2])               # one 0xff credential, elsewhere in B
    args = [N, M, T, NP, len(PUB), Idx(PUB), In(wd.pp), In(wd.h49), In(mh.b48(wd.gamma))] + [In(b"".join(c[k] for c in creds)) for k in range(3)]
    args += [Out(49 * N), Out(48 * NP * N), Out(49 * NP * N), Out(N)]
    return args, list(mi.want_iss(op, wd, mh.b48(wd.gamma), PUB, T, NP, creds))


def _group_row(op, v):
    _, hon = _world(op, v)
    rows = [(i[2], i[1], a[1]) for a, i, _, _, _ in hon]
    j = 2 if v == 0 else 4
    rows[j] = (rows[j][0][:49 * 2] + mh.off_curve_x() + rows[j][0][49 * 3:],) + rows[j][1:]
    args = [N, NP, T, Idx(S), len(PRV)] + [In(b"".join(r[k] for r in rows)) for k in range(3)] + [Out(48 * T * N), Out(49 * N), Out(48 * T * N), Out(96 * T * N), Out(N)]
    return args, list(mi.want_group(op, S, NP, len(PRV), rows))


def _type_row(op, v):
    wd, hon = _world(op, v)
    pubs = [a[0] for a, _, _, _, _ in hon]
    j = 0 if v == 0 else 2
    pubs[j] = mh.field(pubs[j], 1, R)
    args = [N, M, len(PRV), Idx(PRV), len(REV), Idx(REV), In(wd.pp), In(wd.h49), In(b"".join(pubs)), Out(49 * N), Out(49 * N), Out(N)]
    return args, list(mi.want_type(op, wd, PRV, REV, pubs))


# entry -> (row builder, {argument index: why the outputs do not depend on it})
ROWS = {"mhac_bbs_attr_batch": (_attr_row, {6: "pp is decoded for its status alone: generate_attributes parses g1 and g2 and uses neither"}),
        "mhac_bbs_iss_batch": (_iss_row, {}), "mhac_bbs_group_batch": (_group_row, {}), "mhac_bbs_type_batch": (_type_row, {})}


@pytest.mark.parametrize("host", list(ROWS))
def test_inputs_written_behind_a_spin_on_the_contexts_stream(oracle_port, host):
    """warm with B; then spin, copies of A into the same buffers, an event, the _dev call, the read-back and B over the inputs again, all on the
    context's stream with no host wait: the event must still be pending when the call returns, and the outputs are those of A"""
    import torch
    from test_gpu_stream_contract import SPIN, Buffers, World, host_form, pinned
    op = mh.Ops(oracle_port)
    build, unread = ROWS[host]
    (a, want_a), (b, want_b) = build(op, 0), build(op, 1)
    assert want_a != want_b
    w = World()
    try:
        src_a = {i: pinned(torch, x) for i, x in ins(a)}
        src_b = {i: pinned(torch, x) for i, x in ins(b)}
        buf = Buffers(a, b)
        ready = torch.cuda.Event()
        for _ in range(2):
            assert buf.call(w.ctx, host + "_dev") == 0
            assert w.ctx.sync() == 0
        with torch.cuda.stream(w.S):
            buf.read_back()
        w.S.synchronize()
        assert buf.outputs() == want_b, "the builder's batch B under the synchronous bracket"
        with torch.cuda.stream(w.S):
            torch.cuda._sleep(SPIN)
            for i, d in buf.d_in.items():
                d.copy_(src_a[i], non_blocking=True)
            ready.record(w.S)
        rc = buf.call(w.ctx, host + "_dev")
        done_already = ready.query()
        assert rc == 0
        assert not done_already, "the entry blocked the host (or the spin is too short to prove anything)"
        with torch.cuda.stream(w.S):
            buf.read_back()
            for i, d in buf.d_in.items():                               # the clobber: what still reads caller memory now may meet B again
                d.copy_(src_b[i], non_blocking=True)
        w.S.synchronize()
        assert buf.outputs() == want_a
        assert w.ctx.sync() == 0
        # the premise: the outputs depend on every input buffer, so a misordered read of any of them shows
        assert host_form(w.ref, host, a) == (0, want_a)
        for i, x in ins(a):
            rc, outs = host_form(w.ref, host, a[:i] + [b[i]] + a[i + 1:])
            assert rc == 0, (host, i, rc)
            if i in unread:
                assert outs == want_a, (host, i, unread[i])
            else:
                assert outs != want_a, "%s: the outputs do not depend on argument %d" % (host, i)
    finally:
        w.close()


# ---------------------------------------------------------------- the chain on _dev buffers alone
def test_the_chain_on_device_buffers(ctx, op):
    """setup -> attr -> iss -> group (with the gather) -> type -> pres -> verify through the _dev forms on torch buffers, nothing read back in between:
    ok = 1 on every lane; with the e_share rows of lane 0 taken from lane 1 that lane is 0 (the hash half holds, the pairing half does not)"""
    import torch
    from crypto12381_amd.capi import _p
    n, wd = 7, mh.World(op, 6000, M)
    nP, nPub, nhp = len(PRV), 2, 1
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    out = lambda k: torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    ptr = lambda t: _p(t.data_ptr())
    u32 = lambda I: (ctypes.c_uint32 * max(len(I), 1))(*I)
    pp, h, pk, sk = dev(wd.pp), dev(wd.h49), dev(wd.pk), dev(mh.b48(wd.gamma))
    rnd_a = dev(b"".join(mi.attr_rnd(12000, M, PRV, T, n)))
    rnd_i = dev(b"".join(mi.iss_rnd(12100, T, n)))
    rnd_p = dev(b"".join(mi.rnd_bytes(mh.draw(12200 + j, mh.rnd_count(M, PRV, REV, T))) for j in range(n)))
    pub, ashare, C = out(48 * nPub * n), out(48 * nP * NP * n), out(49 * NP * n)
    A, eshare, D, st_i = out(49 * n), out(48 * NP * n), out(49 * NP * n), out(n)
    lam, Dg, eS, aS, st_g = out(48 * T * n), out(49 * n), out(48 * T * n), out(48 * T * nP * n), out(n)
    crev, cpub, st_t = out(49 * n), out(49 * n), out(n)
    torch.cuda.synchronize()
    lib, hd = ctx.lib, ctx.h
    prv, rev = u32(PRV), u32(REV)

    def present_and_verify(rev48):
        fixed, z, zhp, st_p, okv = out(242 * n), out(48 * nP * n), out(48 * nhp * n), out(n), out(n)
        torch.cuda.synchronize()
        assert lib.c12381_mhac_bbs_pres_batch_dev(hd, n, M, T, nP, prv, len(REV), rev, ptr(pp), ptr(h), ptr(A), ptr(Dg), ptr(lam), ptr(eS), ptr(aS), ptr(crev),
                                                  ptr(cpub), ptr(pub), ptr(rnd_p), ptr(fixed), ptr(z), ptr(zhp), ptr(st_p)) == 0
        assert lib.c12381_mhac_bbs_verify_batch_dev(hd, n, M, nP, prv, len(REV), rev, ptr(pp), ptr(h), ptr(pk), ptr(crev), ptr(fixed), ptr(z), ptr(zhp), ptr(rev48),
                                                    ptr(okv)) == 0
        assert ctx.sync() == 0
        return bytes(st_p.cpu().numpy()), bytes(okv.cpu().numpy())

    assert lib.c12381_mhac_bbs_attr_batch_dev(hd, n, M, T, NP, nP, prv, ptr(pp), ptr(h), ptr(rnd_a), ptr(pub), ptr(ashare), ptr(C)) == 0
    assert lib.c12381_mhac_bbs_iss_batch_dev(hd, n, M, T, NP, nPub, u32(PUB), ptr(pp), ptr(h), ptr(sk), ptr(C), ptr(pub), ptr(rnd_i), ptr(A), ptr(eshare), ptr(D),
                                             ptr(st_i)) == 0
    assert lib.c12381_mhac_bbs_group_batch_dev(hd, n, NP, T, u32(S), nP, ptr(D), ptr(eshare), ptr(ashare), ptr(lam), ptr(Dg), ptr(eS), ptr(aS), ptr(st_g)) == 0
    assert lib.c12381_mhac_bbs_type_batch_dev(hd, n, M, nP, prv, len(REV), rev, ptr(pp), ptr(h), ptr(pub), ptr(crev), ptr(cpub), ptr(st_t)) == 0
    # six entries queued back to back on the context's stream; torch's stream is not the context's, so the one torch operation of the chain — the
    # revealed values of verify, position 0 of Pub (attribute 1) of every lane, a strided device copy — waits for the context first
    assert ctx.sync() == 0
    rev48 = pub.view(n, nPub, 48)[:, 0, :].contiguous()
    assert present_and_verify(rev48) == (bytes(n), b"\x01" * n)
    assert bytes(st_i.cpu().numpy()) == bytes(n) and bytes(st_g.cpu().numpy()) == bytes(n) and bytes(st_t.cpu().numpy()) == bytes(n)
    eS.view(n, 48 * T)[0].copy_(eS.view(n, 48 * T)[1])
    assert present_and_verify(rev48) == (bytes(n), b"\x00" + b"\x01" * (n - 1))


# ---------------------------------------------------------------- one credential past a chunk
def test_the_chunk_seam(ctx, op):
    """nparties = 64, t = 2, nPrv = 1, n = 4097: a chunk holds 2^18 / 64 = 4096 credentials.  Host and _dev outputs are equal over all lanes; they are
    checked against the expected functions on the credentials either side of the seam and at both ends"""
    n, np_, t, Prv, m = 4097, 64, 2, (0,), 2
    wd = mh.World(op, 6002, m)
    rnd_a = b"".join(mi.rnd_bytes([prng(13000, 4 * j + i) % (1 << 256) for i in range(3)]) for j in range(n))
    rnd_i = b"".join(mi.rnd_bytes([prng(13001, 2 * j + i) % (1 << 256) for i in range(2)]) for j in range(n))
    sk = mh.b48(wd.gamma)
    a = ctx.mhac_bbs_attr(wd.pp, wd.h49, Prv, t, np_, rnd_a)
    assert ctx.mhac_bbs_attr(wd.pp, wd.h49, Prv, t, np_, rnd_a, dev=True) == a
    pub, ashare, C = a
    i = ctx.mhac_bbs_iss(wd.pp, wd.h49, sk, (1,), t, np_, C, pub, rnd_i)
    assert ctx.mhac_bbs_iss(wd.pp, wd.h49, sk, (1,), t, np_, C, pub, rnd_i, dev=True) == i
    A, es, D, st = i
    assert st == bytes(n)
    for j in (0, 4095, 4096):
        ea = mi.expected_attr(op, wd.pp, wd.h49, Prv, t, np_, rnd_a[96 * j:96 * j + 96])
        assert (pub[48 * j:48 * j + 48], ashare[48 * np_ * j:48 * np_ * (j + 1)], C[49 * np_ * j:49 * np_ * (j + 1)]) == ea, j
        ei = mi.expected_iss(op, wd.pp, wd.h49, sk, (1,), t, np_, ea[2], ea[0], rnd_i[64 * j:64 * j + 64])
        assert (A[49 * j:49 * j + 49], es[48 * np_ * j:48 * np_ * (j + 1)], D[49 * np_ * j:49 * np_ * (j + 1)], st[j]) == ei, j
