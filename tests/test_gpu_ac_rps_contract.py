"""The argument contract of the AC-rps entries (include/c12381_ac.h): every C12381_E_ARG condition in both forms, checked before the empty-batch
rule; n = 0 returns C12381_OK and touches nothing; pres refuses the shapes whose base list does not fit and takes the one that fills it; the host
form and the _dev form return the same bytes."""
import ctypes

import pytest

import ac_rps_cases as rc

from crypto12381_amd.capi import E_ARG

pytestmark = pytest.mark.gpu
COUNTS = {"verify": 6, "pres": 9, "redact": 5}                # pointer arguments behind idx


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


def idx_arr(I):
    return (ctypes.c_uint32 * max(len(I), 1))(*I)


BUF = ctypes.create_string_buffer(1 << 16)
P = ctypes.cast(BUF, ctypes.c_void_p)
BAD_SETS = [(0, ()), (33, ()), (4, (0, 1, 2, 3, 0)), (4, (4,)), (4, (0, 0)), (4, (1 << 31,))]


def entries(ctx, n, nattr, I, null=None, null_idx=False, only=None):
    """the three entries (or only one) in both forms on dummy HOST buffers — every call made here returns before it touches them; null: the
    position of a pointer argument to pass as NULL"""
    lib, arr = ctx.lib, None if null_idx else idx_arr(I)
    out = {}
    for name, count in COUNTS.items():
        if only not in (None, name):
            continue
        ptrs = [None if k == null else P for k in range(count)]
        for form in ("", "_dev"):
            out[name + form] = getattr(lib, "c12381_ac_rps_%s_batch%s" % (name, form))(ctx.h, n, nattr, len(I), arr, *ptrs)
    return out


@pytest.mark.parametrize("n", [0, 3])
@pytest.mark.parametrize("nattr,I", BAD_SETS)
def test_bad_sets(ctx, n, nattr, I):
    assert set(entries(ctx, n, nattr, I).values()) == {E_ARG}


@pytest.mark.parametrize("n", [0, 3])
def test_null_pointers(ctx, n):
    assert set(entries(ctx, n, 4, (0, 3), null_idx=True).values()) == {E_ARG}
    for name, count in COUNTS.items():
        for k in range(count):
            assert set(entries(ctx, n, 4, (0, 3), null=k, only=name).values()) == {E_ARG}, (name, k)
    # attr_48 of verify may be NULL when nI = 0 (position 4), and idx with it
    assert set(entries(ctx, 0, 4, (), null=4, null_idx=True, only="verify").values()) == {0}


def test_list_bounds(ctx):
    """verify: nI + 1 <= 32; pres: nI + 1 + |K| <= 32; redact takes nI = 32"""
    full = tuple(range(32))
    got = entries(ctx, 0, 32, full)
    assert got["verify"] == got["verify_dev"] == got["pres"] == got["pres_dev"] == E_ARG and got["redact"] == got["redact_dev"] == 0
    got = entries(ctx, 0, 32, full[:31])                          # 32 fixed positions: verify's list is full, pres has J = {31} on top of it
    assert got["verify"] == got["verify_dev"] == got["redact"] == got["redact_dev"] == 0 and got["pres"] == got["pres_dev"] == E_ARG
    for nattr, I in rc.REFUSED_PRES_SHAPES:
        got = entries(ctx, 0, nattr, I)
        assert got["pres"] == got["pres_dev"] == E_ARG and got["verify"] == got["redact"] == 0
    assert set(entries(ctx, 0, 16, (0, 3)).values()) == {0}


def test_empty_batch_touches_nothing(ctx):
    BUF.raw = b"\x5a" * len(BUF.raw)
    assert set(entries(ctx, 0, 4, (0, 3)).values()) == {0}
    assert BUF.raw == b"\x5a" * len(BUF.raw) and ctx.sync() == 0


def test_the_list_that_fills_32_positions(ctx, op):
    """(16, (0, 3)): 3 + 29 positions, the largest list pres takes; host form == _dev form, and verify accepts the result"""
    nattr, I = 16, (0, 3)
    key = rc.Key(op, 5216, nattr)
    creds = [rc.Cred(op, key, I, 6300, i) for i in range(2)]
    cat = lambda f: b"".join(getattr(c, f) for c in creds)
    args = (key.pk, key.Y49, I, cat("attr_all"), cat("sig"), cat("cache"), cat("usk"), cat("rnd96"))
    want = [rc.expected_pres(op, key.pk, key.Y49, nattr, I, c.attr_all, c.sig, c.cache, c.usk, c.rnd96) for c in creds]
    host = ctx.ac_rps_pres(*args)
    assert host == (b"".join(w[0] for w in want), bytes(2)) and ctx.ac_rps_pres(*args, dev=True) == host
    assert ctx.ac_rps_verify(key.pk, key.Y49, key.tY97, I, host[0], cat("attr")) == ctx.ac_rps_verify(key.pk, key.Y49, key.tY97, I, host[0], cat("attr"), dev=True) == b"\x01\x01"
