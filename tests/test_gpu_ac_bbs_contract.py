"""The argument contract of the four AC-bbs names of include/c12381_ac.h, the rows tests/test_gpu_api_contract.py holds for the names of
c12381_hip.h: every null pointer and every idx / nattr error returns C12381_E_ARG, in the host and the _dev form alike, errors are reported
before the empty-batch rule, and n = 0 returns C12381_OK and touches nothing."""
import ctypes

import pytest

import ac_bbs_cases as ac
from util import prng

pytestmark = pytest.mark.gpu

NATTR, I = 4, (0, 3)
# positions of the pointer arguments behind (ctx, n, nattr, nI, idx, msg_len)
VERIFY_ARGS = ["pk", "Y", "pres", "u", "attr", "msgs", "ok"]
PRES_ARGS = ["pk", "Y", "attr", "sig", "msgs", "rnd", "pres", "u", "status"]


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(oracle_port):
    op = ac.Ops(oracle_port)
    key = ac.Key(op, 5204, NATTR)
    ln = ac.valid_lanes(op, key, I, 1, 5300)[0]
    a = ac.attributes(5300 + 1000, NATTR)
    sig = ac.issue(op, key, a, 5300 + 2000)
    rnd = b"".join(prng(7000, k, 32).to_bytes(32, "big") for k in range(5))
    host = {"pk": key.pk, "Y": key.Y49, "pres": ln.pres, "u": ln.u, "attr": ln.attr, "msgs": ln.msg}
    host_pres = {"pk": key.pk, "Y": key.Y49, "attr": b"".join(ac.b48(v) for v in a), "sig": sig, "msgs": ln.msg, "rnd": rnd}
    return host, host_pres


def idx_array(values):
    return (ctypes.c_uint32 * max(len(values), 1))(*values)


def call(fn, ctx, n, nattr, idx, msg_len, names, bufs, null=None, nI=None):
    args = [None if k == null else bufs[k] for k in names]
    return fn(ctx.h, n, nattr, len(idx) if nI is None else nI, idx_array(idx), msg_len, *args)


def buffers(world, form, which):
    """host form: bytes in, ctypes buffers out; _dev form: torch tensors (kept alive by the caller) and their addresses"""
    import torch
    host, host_pres = world
    src = host if which == "verify" else host_pres
    outs = {"ok": 1} if which == "verify" else {"pres": 243, "u": 96, "status": 1}
    keep = {}
    if form == "host":
        bufs = dict(src)
        for k, size in outs.items():
            keep[k] = ctypes.create_string_buffer(b"\x07" * size, size)
            bufs[k] = ctypes.cast(keep[k], ctypes.c_void_p)
        read = lambda k: keep[k].raw
    else:
        bufs = {}
        for k, v in src.items():
            keep[k] = torch.frombuffer(bytearray(v), dtype=torch.uint8).to("cuda")
        for k, size in outs.items():
            keep[k] = torch.full((size,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        bufs = {k: ctypes.c_void_p(t.data_ptr()) for k, t in keep.items()}
        read = lambda k: bytes(keep[k].cpu().numpy().tobytes())
    return bufs, outs, read, keep


@pytest.mark.parametrize("which,form", [("verify", "host"), ("verify", "dev"), ("pres", "host"), ("pres", "dev")])
def test_contract(ctx, world, which, form):
    from crypto12381_amd.capi import E_ARG
    fn = getattr(ctx.lib, "c12381_ac_bbs_%s_batch%s" % (which, "" if form == "host" else "_dev"))
    names = VERIFY_ARGS if which == "verify" else PRES_ARGS
    bufs, outs, read, keep = buffers(world, form, which)
    untouched = lambda: all(read(k) == b"\x07" * size for k, size in outs.items())
    for n in (1, 0):                                                 # errors are reported before the empty-batch rule
        for k in names:
            assert call(fn, ctx, n, NATTR, I, 32, names, bufs, null=k) == E_ARG, (n, k)
        assert fn(ctx.h, n, NATTR, 2, None, 32, *[bufs[k] for k in names]) == E_ARG                     # idx
        assert fn(None, n, NATTR, 2, idx_array(I), 32, *[bufs[k] for k in names]) == E_ARG              # ctx
        for nattr, idx in ((0, ()), (33, (0, 3)), (4, (0, 4)), (4, (3, 3)), (4, (0, 1, 2, 3, 0)), (2, (0, 3))):
            assert call(fn, ctx, n, nattr, idx, 32, names, bufs) == E_ARG, (n, nattr, idx)
        assert untouched()
    # what may be NULL: msgs with msg_len = 0; u with nJ = 0; verify's attr with nI = 0 (checked at n = 0: the pointers are not followed)
    assert call(fn, ctx, 0, NATTR, I, 0, names, bufs, null="msgs") == 0
    assert call(fn, ctx, 0, NATTR, (0, 1, 2, 3), 32, names, bufs, null="u") == 0
    assert call(fn, ctx, 0, NATTR, (), 32, names, bufs, null="attr") == (0 if which == "verify" else E_ARG)
    assert call(fn, ctx, 0, NATTR, (), 32, names, bufs) == 0         # nI = 0 with a null idx
    assert fn(ctx.h, 0, NATTR, 0, None, 32, *[bufs[k] for k in names]) == 0
    assert call(fn, ctx, 0, NATTR, I, 32, names, bufs) == 0          # n = 0 touches nothing
    assert ctx.sync() == 0 and untouched()
    assert call(fn, ctx, 1, NATTR, I, 32, names, bufs) == 0          # and the same arguments with n = 1 do the work
    assert ctx.sync() == 0
    if which == "verify":
        assert read("ok") == b"\x01"
    else:
        assert read("status") == b"\x00" and read("pres") != b"\x07" * 243 and read("u") != b"\x07" * 96
