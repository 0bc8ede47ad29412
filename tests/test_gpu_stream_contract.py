"""GPU test of the stream contract of the _dev entries (include/c12381_hip.h "Stream ordering of _dev calls", inherited by include/c12381_ac.h):
every kernel of a context runs on the context's stream or is joined back into it, the inputs only have to be complete ON THAT STREAM when the call
is made, and the call does not block the host.  Every row of tests/stream_cases.py is called while its inputs are still being written behind a
long-running kernel on the context's stream, and while the device buffers, the cached tables and the workspaces still hold another valid batch:
a launch on the side stream without its fork, a table check that ran ahead of its producer, or a read of caller memory on a stream that is not
joined would return that batch's results — valid bytes, no error — and fail here.  Expected bytes: stream_cases (oracle, never the library)."""
import ctypes

import pytest

import stream_cases as sc
from stream_cases import Idx, In, Out

pytestmark = pytest.mark.gpu

SPIN = 400_000_000                       # torch.cuda._sleep cycles: about 0.2 s, the spin of test_gpu_api_contract.py
IDS = [r.id for r in sc.ROWS]
PIPELINED = [r.id for r in sc.ROWS if r.pipelined]

# _dev entries that block the host although nothing can grow: {row id: reason}.  include/c12381_hip.h promises there are none.
BLOCKS_THE_HOST = {}


class World:
    """one context on a torch stream S, and a second context with a stream of its own for the synchronous host forms of the premises"""

    def __init__(self):
        import torch
        torch.cuda.init()
        import tools.libsel  # noqa: F401  C12381_LIB -> capi.use_library, as the variant tests select a build
        from crypto12381_amd import Context
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.S = torch.cuda.Stream(device=self.dev)
        self.ctx = Context(0)
        self.ctx.set_stream(self.S.cuda_stream)
        self.ref = Context(0)

    def close(self):
        self.S.synchronize()
        self.ctx.close()
        self.ref.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def pinned(torch, b):
    return torch.frombuffer(bytearray(bytes(b)), dtype=torch.uint8).pin_memory()


class Buffers:
    """device buffers of one argument list, filled on the default stream (followed by a device-wide wait), and pinned host buffers for the outputs"""

    def __init__(self, args, fill):
        import torch
        dev = torch.device("cuda", 0)
        self.args = args
        self.d_in = {i: torch.frombuffer(bytearray(bytes(fill[i])), dtype=torch.uint8).to(dev) for i, _ in sc.ins(args)}
        self.d_out = {i: torch.zeros(int(a), dtype=torch.uint8, device=dev) for i, a in enumerate(args) if isinstance(a, Out)}
        self.h_out = {i: torch.zeros(int(a), dtype=torch.uint8).pin_memory() for i, a in enumerate(args) if isinstance(a, Out)}
        torch.cuda.synchronize(dev)

    def call(self, ctx, dev):
        """the _dev entry on these buffers: its return code"""
        from crypto12381_amd.capi import _p
        cargs, keep = [], []
        for i, a in enumerate(self.args):
            if isinstance(a, Idx):
                keep.append((ctypes.c_uint32 * max(len(a), 1))(*a))
                cargs.append(keep[-1])
            elif isinstance(a, In):
                cargs.append(_p(self.d_in[i].data_ptr()))
            elif isinstance(a, Out):
                cargs.append(_p(self.d_out[i].data_ptr()))
            else:
                cargs.append(int(a))
        return getattr(ctx.lib, "c12381_" + dev)(ctx.h, *cargs)

    def read_back(self):
        """queue the copy of every output into pinned memory on the current stream"""
        for i, o in self.d_out.items():
            self.h_out[i].copy_(o, non_blocking=True)

    def outputs(self):
        return [bytes(self.h_out[i].numpy()) for i in sorted(self.h_out)]


def host_form(ctx, host, args):
    """the synchronous host form: (return code, [output bytes])"""
    from crypto12381_amd.capi import _p
    outs, cargs, keep = [], [], []
    for a in args:
        if isinstance(a, Idx):
            keep.append((ctypes.c_uint32 * max(len(a), 1))(*a))
            cargs.append(keep[-1])
        elif isinstance(a, In):
            cargs.append(_p(bytes(a)))
        elif isinstance(a, Out):
            outs.append(ctypes.create_string_buffer(int(a)))
            cargs.append(_p(outs[-1]))
        else:
            cargs.append(int(a))
    rc = getattr(ctx.lib, "c12381_" + host)(ctx.h, *cargs)
    return rc, [o.raw for o in outs]


# ---------------------------------------------------------------- a. late inputs, stale caches, no host wait
@pytest.mark.parametrize("id", IDS)
def test_inputs_written_behind_a_spin_on_the_contexts_stream(world, oracle_port, id):
    """warm with B; then spin, copies of A into the same buffers, an event, the _dev call, the read-back and B over the inputs again, all on the
    context's stream with no host wait: the event must still be pending when the call returns, and the outputs are those of A"""
    w, torch, row = world, world.torch, sc.BY_ID[id]
    a, want_a, st_a = sc.case(oracle_port, row, v=0)
    b, want_b, st_b = sc.case(oracle_port, row, v=1)
    src_a = {i: pinned(torch, x) for i, x in sc.ins(a)}
    src_b = {i: pinned(torch, x) for i, x in sc.ins(b)}
    buf = Buffers(a, b)
    ready = torch.cuda.Event()
    try:
        # 1. warm with B, twice — the first call may grow and zero a workspace, the second one runs as every later call does: tables, caches
        # and workspaces hold B's keys at their final sizes
        for _ in range(2):
            assert buf.call(w.ctx, row.dev) == 0
            assert w.ctx.sync() == st_b
        with torch.cuda.stream(w.S):
            buf.read_back()
        w.S.synchronize()
        assert buf.outputs() == want_b, "the builder's batch B under the synchronous bracket"
        # 2. everything on S, no host wait between the steps
        with torch.cuda.stream(w.S):
            torch.cuda._sleep(SPIN)
            for i, d in buf.d_in.items():
                d.copy_(src_a[i], non_blocking=True)
            ready.record(w.S)
        rc = buf.call(w.ctx, row.dev)
        # 3. the inputs were not there yet when the call returned: it was made while the device held B, and it did not wait
        done_already = ready.query()
        assert rc == 0
        if id not in BLOCKS_THE_HOST:
            assert not done_already, "the entry blocked the host (or the spin is too short to prove anything)"
        with torch.cuda.stream(w.S):
            buf.read_back()
            for i, d in buf.d_in.items():                               # the clobber: what still reads caller memory now may meet B again
                d.copy_(src_b[i], non_blocking=True)
        # 4.
        w.S.synchronize()
        assert buf.outputs() == want_a
        assert w.ctx.sync() == st_a
    finally:
        w.S.synchronize()
    # 5. the premise: the outputs depend on every input buffer, so a misordered read of any of them shows
    assert host_form(w.ref, row.host, a) == (st_a, want_a)
    for i, x in sc.ins(a):
        rc, outs = host_form(w.ref, row.host, a[:i] + [b[i]] + a[i + 1:])
        assert rc == 0, (id, i, rc)
        if i in row.unread:
            assert outs == want_a, (id, i, row.unread[i])
        else:
            assert outs != want_a, "%s: the outputs do not depend on argument %d" % (id, i)


# ---------------------------------------------------------------- b. back to back, no wait, growing
@pytest.mark.parametrize("id", PIPELINED)
def test_two_calls_back_to_back_the_second_one_larger(oracle_port, id):
    """a fresh context: call(A), then call(B at twice the lane count) while the first is still queued behind the spin — the second call grows the
    workspaces under the first one (it may block the host for that)"""
    import torch
    from crypto12381_amd import Context
    row = sc.BY_ID[id]
    a, want_a, st_a = sc.case(oracle_port, row, v=0)
    b, want_b, st_b = sc.case(oracle_port, row, n=2 * row.n, v=1)
    S = torch.cuda.Stream(device=torch.device("cuda", 0))
    c = Context(0)
    try:
        c.set_stream(S.cuda_stream)
        buf_a, buf_b = Buffers(a, a), Buffers(b, b)
        with torch.cuda.stream(S):
            torch.cuda._sleep(SPIN)
        assert buf_a.call(c, row.dev) == 0
        assert buf_b.call(c, row.dev) == 0
        with torch.cuda.stream(S):
            buf_a.read_back()
            buf_b.read_back()
        S.synchronize()                                                 # the one wait
        assert buf_a.outputs() == want_a
        assert buf_b.outputs() == want_b
        assert c.sync() == 0 and st_a == 0 and st_b == 0
    finally:
        S.synchronize()
        c.close()


# ---------------------------------------------------------------- d. c12381_trim with work in flight
def test_trim_with_a_forking_call_in_flight(oracle_port):
    """c12381_trim waits for the context's streams before it frees: the call queued behind the spin completes with the right bytes, and the
    next call rebuilds tables and workspaces and gives the same bytes again"""
    import torch
    from crypto12381_amd import Context
    row = sc.BY_ID["bbs_plus_verify_wire"]
    a, want_a, st_a = sc.case(oracle_port, row, v=0)
    S = torch.cuda.Stream(device=torch.device("cuda", 0))
    c = Context(0)
    try:
        c.set_stream(S.cuda_stream)
        buf = Buffers(a, a)
        with torch.cuda.stream(S):
            torch.cuda._sleep(SPIN)
        assert buf.call(c, row.dev) == 0
        c.trim()
        with torch.cuda.stream(S):
            buf.read_back()
        S.synchronize()
        assert buf.outputs() == want_a
        assert c.sync() == st_a
        for o in buf.d_out.values():
            o.zero_()
        torch.cuda.synchronize()
        assert buf.call(c, row.dev) == 0
        assert c.sync() == st_a
        with torch.cuda.stream(S):
            buf.read_back()
        S.synchronize()
        assert buf.outputs() == want_a
    finally:
        S.synchronize()
        c.close()
