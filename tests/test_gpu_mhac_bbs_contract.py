"""The argument contract of the MHAC-bbs entries (include/c12381_mhac.h), row by row in both forms: every null pointer, every error of the index
sets (m = 0, m above the bound, an index >= m, a repeated index, Rev meeting Prv, a null set with a count), t outside 1 .. C12381_MHAC_T_MAX and
the list bound of pres — all checked before the empty-batch rule; n = 0 returns C12381_OK and touches nothing; which pointers may be NULL.  And the
stream contract of the two _dev entries by the method of tests/test_gpu_stream_contract.py, with rows of this file's own: the inputs are written on
the context's stream behind a long-running kernel, with no host wait before the call, while the buffers, tables and workspaces hold another batch."""
import ctypes

import pytest

import mhac_bbs_cases as mh
from stream_cases import Idx, In, Out, ins
from util import R

from crypto12381_amd.capi import E_ARG

pytestmark = pytest.mark.gpu
COUNTS = {"verify": 9, "pres": 15}                       # pointer arguments behind the sets
V = dict(pp=0, h=1, pk=2, crev=3, fixed=4, z=5, zhp=6, pub=7, ok=8)
Pp = dict(pp=0, h=1, A=2, D=3, lam=4, eshare=5, ashare=6, crev=7, cpub=8, pub=9, rnd=10, fixed=11, z=12, zhp=13, status=14)


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


def arr(I):
    return (ctypes.c_uint32 * max(len(I), 1))(*I)


BUF = ctypes.create_string_buffer(1 << 16)
P = ctypes.cast(BUF, ctypes.c_void_p)


def entries(ctx, n, m, Prv, Rev, t=3, null=(), null_prv=False, null_rev=False, only=None):
    """both entries (or only one) in both forms on dummy HOST buffers — every call made here returns before it touches them; null: the positions
    of the pointer arguments to pass as NULL"""
    pa, ra = (None if null_prv else arr(Prv)), (None if null_rev else arr(Rev))
    out = {}
    for name, count in COUNTS.items():
        if only not in (None, name):
            continue
        ptrs = [None if k in null else P for k in range(count)]
        head = (n, m) + ((t,) if name == "pres" else ()) + (len(Prv), pa, len(Rev), ra)
        for form in ("", "_dev"):
            out[name + form] = getattr(ctx.lib, "c12381_mhac_bbs_%s_batch%s" % (name, form))(ctx.h, *head, *ptrs)
    return out


BAD_SETS = [(0, (), ()), (33, (), ()), (4, (4,), ()), (4, (), (4,)), (4, (0, 0), ()), (4, (), (1, 1)), (4, (0, 2), (2,)), (4, (1 << 31,), ()), (4, (), (36,)),
            (4, (0, 1, 2, 3, 0), ()), (1, (0,), (0,))]


@pytest.mark.parametrize("n", [0, 3])
@pytest.mark.parametrize("m,Prv,Rev", BAD_SETS)
def test_bad_sets(ctx, n, m, Prv, Rev):
    assert set(entries(ctx, n, m, Prv, Rev).values()) == {E_ARG}


@pytest.mark.parametrize("n", [0, 3])
def test_t_and_the_list_bound(ctx, n):
    for t in (0, 9, 1 << 40):
        got = entries(ctx, n, 4, (0, 2), (1,), t=t, only="pres")
        assert set(got.values()) == {E_ARG}, t
    assert set(entries(ctx, n, 5, (0, 1, 2, 3), (), t=8, only="pres").values()) == {E_ARG}          # 5 + 7 x 4 = 33 positions
    assert set(entries(ctx, n, 32, tuple(range(16)), (), t=2, only="pres").values()) == {E_ARG}     # 32 + 16
    if n == 0:
        assert set(entries(ctx, 0, 4, (0, 1, 2, 3), (), t=8).values()) == {0}                       # 4 + 7 x 4 = 32 fills the list
        assert set(entries(ctx, 0, 32, tuple(range(16)), tuple(range(16, 32)), t=2, only="pres").values()) == {0}
        assert set(entries(ctx, 0, 32, (), (), t=8).values()) == {0}


@pytest.mark.parametrize("n", [0, 3])
def test_null_pointers(ctx, n):
    """the small world has every count above 0: no pointer may be NULL"""
    assert set(entries(ctx, n, 4, (0, 2), (1,), null_prv=True).values()) == {E_ARG}
    assert set(entries(ctx, n, 4, (0, 2), (1,), null_rev=True).values()) == {E_ARG}
    for name, count in COUNTS.items():
        for k in range(count):
            assert set(entries(ctx, n, 4, (0, 2), (1,), null=(k,), only=name).values()) == {E_ARG}, (name, k)
    from crypto12381_amd.capi import E_ARG as e
    lib = ctx.lib
    assert lib.c12381_mhac_bbs_verify_batch(None, n, 4, 2, arr((0, 2)), 1, arr((1,)), *[P] * 9) == e
    assert lib.c12381_mhac_bbs_pres_batch_dev(None, n, 4, 3, 2, arr((0, 2)), 1, arr((1,)), *[P] * 15) == e


def test_pointers_that_may_be_null(ctx):
    """each array whose count is 0, and no other: Prv empty — prv, z, a_share; Rev empty — rev, the revealed values of verify; Prv = all — the public
    values, zhp; Rev = all of Pub — zhp, while pres still takes the whole public span"""
    ok = lambda got: set(got.values()) == {0}
    bad = lambda got: set(got.values()) == {E_ARG}
    assert ok(entries(ctx, 0, 4, (), (1,), null=(V["z"],), null_prv=True, only="verify"))
    assert ok(entries(ctx, 0, 4, (), (1,), null=(Pp["ashare"], Pp["z"]), null_prv=True, only="pres"))
    assert bad(entries(ctx, 0, 4, (), (1,), null=(V["zhp"],), only="verify")) and bad(entries(ctx, 0, 4, (), (1,), null=(Pp["pub"],), only="pres"))
    assert ok(entries(ctx, 0, 4, (0, 2), (), null=(V["pub"],), null_rev=True, only="verify"))
    assert bad(entries(ctx, 0, 4, (0, 2), (), null=(Pp["pub"],), null_rev=True, only="pres"))
    assert ok(entries(ctx, 0, 4, (0, 1, 2, 3), (), null=(V["zhp"], V["pub"]), null_rev=True, only="verify"))
    assert ok(entries(ctx, 0, 4, (0, 1, 2, 3), (), null=(Pp["pub"], Pp["zhp"]), null_rev=True, only="pres"))
    assert bad(entries(ctx, 0, 4, (0, 1, 2, 3), (), null=(V["z"],), only="verify"))
    assert ok(entries(ctx, 0, 4, (0, 2), (1, 3), null=(V["zhp"],), only="verify")) and ok(entries(ctx, 0, 4, (0, 2), (1, 3), null=(Pp["zhp"],), only="pres"))
    assert bad(entries(ctx, 0, 4, (0, 2), (1, 3), null=(V["pub"],), only="verify")) and bad(entries(ctx, 0, 4, (0, 2), (1, 3), null=(Pp["pub"],), only="pres"))
    assert ok(entries(ctx, 0, 1, (), (), null=(V["z"], V["pub"]), null_prv=True, null_rev=True, only="verify"))


def test_empty_batch_touches_nothing(ctx):
    BUF.raw = b"\x5a" * len(BUF.raw)
    assert set(entries(ctx, 0, 4, (0, 2), (1,)).values()) == {0}
    assert BUF.raw == b"\x5a" * len(BUF.raw) and ctx.sync() == 0


# ---------------------------------------------------------------- the stream contract of the two _dev entries
N = 5
PRV, REV, T = mh.PRV_MAIN, mh.REV_MAIN, mh.T_MAIN


def _verify_row(op, v):
    """batch A (v = 0) / B (v = 1): another world, other holders; lanes 1, 3 tampered in A, 0, 2 in B"""
    wd = mh.World(op, 9000 + v, mh.M_MAIN)
    lanes = mh.valid_lanes(op, wd, PRV, REV, T, N, 9100 + 1000 * v)
    for j in ((1, 3) if v == 0 else (0, 2)):
        lanes[j] = mh.with_(lanes[j], "zr+1", fixed=mh.plus1(lanes[j].fixed, 1, 98))
    args = [N, mh.M_MAIN, len(PRV), Idx(PRV), len(REV), Idx(REV), In(wd.pp), In(wd.h49), In(wd.pk)] + [In(b) for b in mh.pack(lanes)] + [Out(N)]
    return args, [mh.expect(op, wd, PRV, REV, lanes)]


def _pres_row(op, v):
    wd = mh.World(op, 9000 + v, mh.M_MAIN)
    rows, cols = [], {k: b"" for k in ("A49", "D49", "lam48", "es48", "as48", "crev49", "cpub49", "pub48", "rnd")}
    for j in range(N):
        hd = mh.Holder(op, wd, PRV, REV, T, 9200 + 1000 * v + 100 * j)
        i = hd.pres_inputs(op, mh.draw(9250 + 1000 * v + 100 * j, mh.rnd_count(mh.M_MAIN, PRV, REV, T)))
        if j == (2 if v == 0 else 4):
            i["lam48"] = mh.field(i["lam48"], 1, R)                   # one 0xff lane, elsewhere in B
        rows.append(mh.expected_pres(op, wd.pp, wd.h49, PRV, REV, T, **i))
        for k in cols:
            cols[k] += i[k]
    args = [N, mh.M_MAIN, T, len(PRV), Idx(PRV), len(REV), Idx(REV), In(wd.pp), In(wd.h49)] + [In(cols[k]) for k in cols] + [Out(242 * N), Out(96 * N), Out(48 * N), Out(N)]
    return args, [b"".join(r[k] for r in rows) for k in range(3)] + [bytes(r[3] for r in rows)]


# entry -> (row builder, {argument index: why the outputs do not depend on it})
ROWS = {"mhac_bbs_verify_batch": (_verify_row, {}),
        "mhac_bbs_pres_batch": (_pres_row, {7: "pp is decoded for its status alone: cred_pres parses g1 and g2 and uses neither"})}


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
