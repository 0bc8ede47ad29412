"""The argument contract of the AC issuance entries (include/c12381_ac_issue.h) in both forms: nattr = 0 and nattr above the bound, every null pointer and
a null context — all checked before the empty-batch rule; n = 0 returns C12381_OK and touches nothing.  The stream contract of the four _dev entries by
the method of tests/test_gpu_stream_contract.py.  And per scheme one chain on _dev buffers alone: issue -> (redact ->) pres -> verify gives ok = 1 on
every lane, and ok = 0 where one credential's disclosed attribute is changed after issuance."""
import ctypes

import pytest

import ac_bbs_cases as ab
import ac_issue_cases as ai
import ac_rbbs_cases as arb
import ac_rps_cases as arp
import mhac_iss_cases as mi
from ac_bbs_cases import b48
from stream_cases import Idx, In, Out, ins
from util import R, prng

from crypto12381_amd.capi import E_ARG

pytestmark = pytest.mark.gpu
BUF = ctypes.create_string_buffer(1 << 16)
P = ctypes.cast(BUF, ctypes.c_void_p)
# entry -> (has nattr, pointer arguments)
ENTRIES = {"ac_bbs_issue": (True, 7), "ac_rbbs_issue": (True, 7), "ac_rps_user_keygen": (False, 4), "ac_rps_issue": (True, 8)}


@pytest.fixture(scope="module")
def ctx():
    c = mi.ctx_fixture()
    yield c
    c.close()


@pytest.fixture(scope="module")
def op(oracle_port):
    return ab.Ops(oracle_port)


def call(ctx, name, n, nattr=4, null=(), h=True):
    """the entry in both forms on dummy HOST buffers — every call made here returns before it touches them; null: pointer positions passed as NULL"""
    has_nattr, nptr = ENTRIES[name]
    ptrs = [None if k in null else P for k in range(nptr)]
    head = (n, nattr) if has_nattr else (n,)
    return {form: getattr(ctx.lib, "c12381_%s_batch%s" % (name, form))(ctx.h if h else None, *head, *ptrs) for form in ("", "_dev")}


bad = lambda got: set(got.values()) == {E_ARG}
ok = lambda got: set(got.values()) == {0}


@pytest.mark.parametrize("n", [0, 3])
def test_argument_errors(ctx, n):
    for name, (has_nattr, nptr) in ENTRIES.items():
        if has_nattr:
            for nattr in (0, 33, 1 << 40):
                assert bad(call(ctx, name, n, nattr)), (name, nattr)
        for k in range(nptr):
            assert bad(call(ctx, name, n, null=(k,))), (name, k)
        assert bad(call(ctx, name, n, h=False)), name


def test_empty_batch_touches_nothing_and_the_bounds_are_accepted(ctx):
    BUF.raw = b"\x5a" * len(BUF.raw)
    for name in ENTRIES:
        for nattr in (1, 32):
            assert ok(call(ctx, name, 0, nattr)), (name, nattr)
    assert BUF.raw == b"\x5a" * len(BUF.raw) and ctx.sync() == 0


# ---------------------------------------------------------------- the stream contract of the four _dev entries
N, NATTR, I_SET = 5, 4, (0, 3)


def _bbs_row(op, v, scheme="bbs"):
    key = (ai.bbs_key if scheme == "bbs" else ai.rbbs_key)(op, 9000 + v, NATTR)
    lanes = ai.bbs_lanes(key.x, None, NATTR, 9300 + 1000 * v)[:N]
    j = 1 if v == 0 else 3
    lanes[j] = ai.Lane("a = r", lanes[j].attr[:48] + b48(R) + lanes[j].attr[96:], lanes[j].rnd, 0xff)            # one 0xff credential, elsewhere in B
    Y49 = key.Y49[:49 * NATTR]
    args = [N, NATTR, In(key.sk), In(key.pk), In(Y49), *(In(b) for b in ai.pack(lanes)), Out(97 * N), Out(N)]
    return args, list(ai.want_bbs(op, key, Y49, NATTR, lanes))


def _rbbs_row(op, v):
    return _bbs_row(op, v, "rbbs")


def _keygen_row(op, v):
    key = ai.rps_key(op, 9010 + v, NATTR)
    rnds = [ai.b32raw(prng(9400 + v, i, 32)) for i in range(N)]
    rows = [ai.expected_user_keygen(op, key.pk, r)[0] for r in rnds]
    return [N, In(key.pk), In(b"".join(rnds)), Out(48 * N), Out(49 * N)], [b"".join(r[0] for r in rows), b"".join(r[1] for r in rows)]


def _rps_row(op, v):
    key = ai.rps_key(op, 9020 + v, NATTR)
    lanes = ai.rps_lanes(op, key.g, key.x, key.y, NATTR, 9500 + 1000 * v)[:N]
    j = 2 if v == 0 else 4
    lanes[j] = ai.Lane("upk off curve", lanes[j].attr, lanes[j].rnd, 0xff, ab.off_curve_x())
    tY97 = key.tY97[:97 * NATTR]
    args = [N, NATTR, In(key.sk), In(key.pk), In(tY97), *(In(b) for b in ai.pack(lanes)), Out(195 * N), Out(N)]
    return args, list(ai.want_rps(op, key, lanes))


# entry -> (row builder, {argument index: why the outputs do not depend on it})
ROWS = {"ac_bbs_issue_batch": (_bbs_row, {}), "ac_rbbs_issue_batch": (_rbbs_row, {}), "ac_rps_user_keygen_batch": (_keygen_row, {}),
        "ac_rps_issue_batch": (_rps_row, {})}


@pytest.mark.parametrize("host", list(ROWS))
def test_inputs_written_behind_a_spin_on_the_contexts_stream(oracle_port, host):
    """warm with B; then spin, copies of A into the same buffers, an event, the _dev call, the read-back and B over the inputs again, all on the
    context's stream with no host wait: the event must still be pending when the call returns, and the outputs are those of A"""
    import torch
    from test_gpu_stream_contract import SPIN, Buffers, World, host_form, pinned
    op = ab.Ops(oracle_port)
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


# ---------------------------------------------------------------- the chains on _dev buffers alone
def _tools():
    import torch
    from crypto12381_amd.capi import _p
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    out = lambda k: torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    ptr = lambda t: _p(t.data_ptr())
    return torch, dev, out, ptr


def _disclosed(attr, n, I):
    """the disclosed fields of every lane in the order of I: a strided device copy (a torch operation: the caller has synchronised the context)"""
    import torch
    return attr.view(n, NATTR, 48)[:, torch.tensor(list(I), device=attr.device), :].contiguous()


def _tamper(attr, n, i):
    """lane 0 claims another value for attribute i"""
    import torch
    attr.view(n, NATTR, 48)[0, i].copy_(torch.frombuffer(bytearray(b48(123456789)), dtype=torch.uint8).to(attr.device))


def _bytes(t):
    return bytes(t.cpu().numpy().tobytes())


@pytest.mark.parametrize("scheme", ["bbs", "rbbs"])
def test_the_bbs_chains_on_device_buffers(ctx, op, scheme):
    torch, dev, out, ptr = _tools()
    n, I, L = 7, I_SET, ab.MSG_LEN
    key = (ai.bbs_key if scheme == "bbs" else ai.rbbs_key)(op, 9600, NATTR)
    idx = (ctypes.c_uint32 * len(I))(*I)
    nJ = NATTR - len(I)
    sk, pk, Y = dev(key.sk), dev(key.pk), dev(key.Y49)
    attr = dev(b"".join(ai.span(ab.attributes(9610 + j, NATTR)) for j in range(n)))
    rnd_i = dev(b"".join(ai.b32raw(prng(9620, j, 32)) for j in range(n)))
    msgs = dev(b"".join(ab.message(9630, j) for j in range(n)))
    sig, st_i = out(97 * n), out(n)
    torch.cuda.synchronize()
    lib, hd = ctx.lib, ctx.h
    assert getattr(lib, "c12381_ac_%s_issue_batch_dev" % scheme)(hd, n, NATTR, ptr(sk), ptr(pk), ptr(Y), ptr(attr), ptr(rnd_i), ptr(sig), ptr(st_i)) == 0

    def present_and_verify():
        aI, okv, st_p = _disclosed(attr, n, I), out(n), out(n)
        torch.cuda.synchronize()
        if scheme == "bbs":
            rnd_p = dev(b"".join(ab.b32(v) for j in range(n) for v in ab.draw(9640 + j, nJ)))
            pres, u = out(243 * n), out(48 * nJ * n)
            torch.cuda.synchronize()
            assert lib.c12381_ac_bbs_pres_batch_dev(hd, n, NATTR, len(I), idx, L, ptr(pk), ptr(Y), ptr(attr), ptr(sig), ptr(msgs), ptr(rnd_p), ptr(pres), ptr(u),
                                                    ptr(st_p)) == 0
            assert lib.c12381_ac_bbs_verify_batch_dev(hd, n, NATTR, len(I), idx, L, ptr(pk), ptr(Y), ptr(pres), ptr(u), ptr(aI), ptr(msgs), ptr(okv)) == 0
        else:
            tY = dev(key.tY97)
            rnd_p = dev(b"".join(ab.b32(v) for j in range(n) for v in arb.draw(9640 + j)))
            cache, st_r, pres = out(196 * n), out(n), out(341 * n)
            torch.cuda.synchronize()
            assert lib.c12381_ac_rbbs_redact_batch_dev(hd, n, NATTR, len(I), idx, ptr(pk), ptr(Y), ptr(attr), ptr(sig), ptr(cache), ptr(st_r)) == 0
            assert lib.c12381_ac_rbbs_pres_batch_dev(hd, n, L, ptr(sig), ptr(cache), ptr(msgs), ptr(rnd_p), ptr(pres), ptr(st_p)) == 0
            assert lib.c12381_ac_rbbs_verify_batch_dev(hd, n, NATTR, len(I), idx, L, ptr(pk), ptr(Y), ptr(tY), ptr(pres), ptr(aI), ptr(msgs), ptr(okv)) == 0
        assert ctx.sync() == 0
        return _bytes(st_p), _bytes(okv)

    assert ctx.sync() == 0                                               # torch's stream is not the context's: the gather of the disclosed fields waits
    assert present_and_verify() == (bytes(n), b"\x01" * n)
    assert _bytes(st_i) == bytes(n)
    _tamper(attr, n, I[1])
    assert present_and_verify() == (bytes(n), b"\x00" + b"\x01" * (n - 1))


def test_the_rps_chain_on_device_buffers(ctx, op):
    torch, dev, out, ptr = _tools()
    n, I = 7, I_SET
    key = ai.rps_key(op, 9700, NATTR)
    idx = (ctypes.c_uint32 * len(I))(*I)
    sk, pk, Y, tY = dev(key.sk), dev(key.pk), dev(key.Y49), dev(key.tY97)
    attr = dev(b"".join(ai.span(ab.attributes(9710 + j, NATTR)) for j in range(n)))
    rnd_k, rnd_i = (dev(b"".join(ai.b32raw(prng(9720 + k, j, 32)) for j in range(n))) for k in range(2))
    rnd_p = dev(b"".join(ab.b32(v) for j in range(n) for v in arp.draw(9740 + j)))
    usk, upk, sig, st_i = out(48 * n), out(49 * n), out(195 * n), out(n)
    torch.cuda.synchronize()
    lib, hd = ctx.lib, ctx.h
    assert lib.c12381_ac_rps_user_keygen_batch_dev(hd, n, ptr(pk), ptr(rnd_k), ptr(usk), ptr(upk)) == 0
    assert lib.c12381_ac_rps_issue_batch_dev(hd, n, NATTR, ptr(sk), ptr(pk), ptr(tY), ptr(upk), ptr(attr), ptr(rnd_i), ptr(sig), ptr(st_i)) == 0

    def present_and_verify():
        aI, cache, st_r, pres, st_p, okv = _disclosed(attr, n, I), out(97 * n), out(n), out(389 * n), out(n), out(n)
        torch.cuda.synchronize()
        assert lib.c12381_ac_rps_redact_batch_dev(hd, n, NATTR, len(I), idx, ptr(tY), ptr(attr), ptr(sig), ptr(cache), ptr(st_r)) == 0
        assert lib.c12381_ac_rps_pres_batch_dev(hd, n, NATTR, len(I), idx, ptr(pk), ptr(Y), ptr(attr), ptr(sig), ptr(cache), ptr(usk), ptr(rnd_p), ptr(pres),
                                                ptr(st_p)) == 0
        assert lib.c12381_ac_rps_verify_batch_dev(hd, n, NATTR, len(I), idx, ptr(pk), ptr(Y), ptr(tY), ptr(pres), ptr(aI), ptr(okv)) == 0
        assert ctx.sync() == 0
        return _bytes(st_r), _bytes(st_p), _bytes(okv)

    assert ctx.sync() == 0
    assert present_and_verify() == (bytes(n), bytes(n), b"\x01" * n)
    assert _bytes(st_i) == bytes(n)
    _tamper(attr, n, I[1])
    assert present_and_verify() == (bytes(n), bytes(n), b"\x00" + b"\x01" * (n - 1))
