"""The argument contract of the six AC-rbbs names of include/c12381_ac.h, as tests/test_gpu_ac_bbs_contract.py holds it for AC-bbs: every null
pointer and every idx / nattr error returns C12381_E_ARG, in the host and the _dev form alike, errors are reported before the empty-batch rule,
n = 0 returns C12381_OK and touches nothing, redact refuses nattr = 17, and a second call with the same key and set returns the same bytes (from
the cached tables: results alone cannot show whether one was rebuilt, tests/test_gpu_table_slots.py)."""
import ctypes

import pytest

import ac_rbbs_cases as rc

pytestmark = pytest.mark.gpu

NATTR, I = 4, (0, 3)
# the pointer arguments behind the scalar ones, and the scalar arguments behind (ctx, n)
ARGS = {"verify": ["pk", "Y", "tY", "pres", "attr", "msgs", "ok"], "pres": ["sig", "cache", "msgs", "rnd", "pres_out", "status"],
        "redact": ["pk", "Y", "attr_all", "sig", "cache_out", "status"]}
OUTS = {"verify": {"ok": 1}, "pres": {"pres_out": 341, "status": 1}, "redact": {"cache_out": 196, "status": 1}}


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
    op = rc.Ops(oracle_port)
    key = rc.Key(op, 5204, NATTR)
    cr = rc.Cred(op, key, I, 5300, 0)
    pres = rc.pres(op, cr.msg, cr.sig, cr.cache, cr.rnd)
    return {"pk": key.pk, "Y": key.Y49, "tY": key.tY97, "pres": pres, "attr": cr.attr, "msgs": cr.msg, "sig": cr.sig, "cache": cr.cache,
            "rnd": b"".join(v.to_bytes(32, "big") for v in cr.rnd), "attr_all": cr.attr_all}, pres, cr.cache


def idx_array(values):
    return (ctypes.c_uint32 * max(len(values), 1))(*values)


def scalars(which, nattr, idx, msg_len, nI=None, null_idx=False):
    arr = None if null_idx else idx_array(idx)
    nI = len(idx) if nI is None else nI
    return {"verify": [nattr, nI, arr, msg_len], "pres": [msg_len], "redact": [nattr, nI, arr]}[which]


def buffers(world, form, which):
    """host form: bytes in, ctypes buffers out; _dev form: torch tensors (kept alive by the caller) and their addresses"""
    import torch
    src = {k: world[0][k] for k in ARGS[which] if k in world[0]}
    keep = {}
    if form == "host":
        bufs = dict(src)
        for k, size in OUTS[which].items():
            keep[k] = ctypes.create_string_buffer(b"\x07" * size, size)
            bufs[k] = ctypes.cast(keep[k], ctypes.c_void_p)
        read = lambda k: keep[k].raw
    else:
        for k, v in src.items():
            keep[k] = torch.frombuffer(bytearray(v), dtype=torch.uint8).to("cuda")
        for k, size in OUTS[which].items():
            keep[k] = torch.full((size,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        bufs = {k: ctypes.c_void_p(t.data_ptr()) for k, t in keep.items()}
        read = lambda k: bytes(keep[k].cpu().numpy().tobytes())
    return bufs, read, keep


@pytest.mark.parametrize("which,form", [(w, f) for w in ("verify", "pres", "redact") for f in ("host", "dev")])
def test_contract(ctx, world, which, form):
    from crypto12381_amd.capi import E_ARG
    fn = getattr(ctx.lib, "c12381_ac_rbbs_%s_batch%s" % (which, "" if form == "host" else "_dev"))
    names, outs = ARGS[which], OUTS[which]
    bufs, read, keep = buffers(world, form, which)
    ptrs = lambda null=None: [None if k == null else bufs[k] for k in names]
    untouched = lambda: all(read(k) == b"\x07" * size for k, size in outs.items())
    for n in (1, 0):                                                 # errors are reported before the empty-batch rule
        for k in names:
            assert fn(ctx.h, n, *scalars(which, NATTR, I, 32), *ptrs(k)) == E_ARG, (n, k)
        assert fn(None, n, *scalars(which, NATTR, I, 32), *ptrs()) == E_ARG                              # ctx
        if which != "pres":
            assert fn(ctx.h, n, *scalars(which, NATTR, I, 32, null_idx=True), *ptrs()) == E_ARG          # idx
            for nattr, idx in ((0, ()), (33, (0, 3)), (4, (0, 4)), (4, (3, 3)), (4, (0, 1, 2, 3, 0)), (2, (0, 3))):
                assert fn(ctx.h, n, *scalars(which, nattr, idx, 32), *ptrs()) == E_ARG, (n, nattr, idx)
        if which == "redact":
            assert fn(ctx.h, n, *scalars(which, 17, I, 32), *ptrs()) == E_ARG                            # the bound of redact's base list
            assert fn(ctx.h, n, *scalars(which, 32, I, 32), *ptrs()) == E_ARG
        assert untouched()
    # what may be NULL (checked at n = 0: the pointers are not followed): msgs with msg_len = 0; verify's attr with nI = 0; idx with nI = 0
    if which != "redact":
        assert fn(ctx.h, 0, *scalars(which, NATTR, I, 0), *ptrs("msgs")) == 0
    if which == "verify":
        assert fn(ctx.h, 0, *scalars(which, NATTR, (), 32), *ptrs("attr")) == 0
        assert fn(ctx.h, 0, *scalars(which, 32, I, 32), *ptrs()) == 0                                    # verify takes 32 attributes
    if which != "pres":
        assert fn(ctx.h, 0, *scalars(which, NATTR, (), 32, null_idx=True), *ptrs()) == 0
    assert fn(ctx.h, 0, *scalars(which, NATTR, I, 32), *ptrs()) == 0                                     # n = 0 touches nothing
    assert ctx.sync() == 0 and untouched()
    for _ in range(2):                                               # the same arguments with n = 1 do the work; the second call finds every table built
        assert fn(ctx.h, 1, *scalars(which, NATTR, I, 32), *ptrs()) == 0
        assert ctx.sync() == 0
        if which == "verify":
            assert read("ok") == b"\x01"
        elif which == "pres":
            assert read("status") == b"\x00" and read("pres_out") == world[1]
        else:
            assert read("status") == b"\x00" and read("cache_out") == world[2]
