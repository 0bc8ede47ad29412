"""c12381_sha3_512_batch: one SHA3-512 per lane (crypto12381_amd/csrc/sha3.hpp), compared with hashlib (FIPS 202; equal to the reference's
hash_state digests, tests/test_host_sim_sha3.py) at the lengths of tests/golden/sha3_512.json — either side of the 72-byte rate — for
batches of 0, 1, 63, 64, 65 and 2^16 messages; the _dev form on torch tensors; argument errors."""
import hashlib

import pytest

from util import golden

pytestmark = pytest.mark.gpu

LENGTHS = golden("sha3_512")["lengths"]


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


def _msgs(n, length, seed):
    # distinct messages without hashing n x length bytes one at a time: a per-length stream cut into n windows
    stream = hashlib.shake_256(b"sha3 gpu|%d|%d" % (seed, length)).digest(n * length) if n * length else b""
    return stream


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_sha3_matches_hashlib(ctx, n, length):
    msgs = _msgs(n, length, n)
    got = ctx.sha3_512(msgs, n, length)
    assert got == b"".join(hashlib.sha3_512(msgs[length * i:length * i + length]).digest() for i in range(n))


def test_golden_digests(ctx):
    g = golden("sha3_512")
    for m, d in zip(g["msgs"], g["digests"]):
        msg = bytes.fromhex(m)
        assert ctx.sha3_512(msg, 1, len(msg)).hex() == d


@pytest.mark.parametrize("length", [0, 72, 143, 919, 1000])
def test_sha3_large_batch(ctx, length):
    n = 1 << 16
    msgs = _msgs(n, length, 7)
    got = ctx.sha3_512(msgs, n, length)
    want = b"".join(hashlib.sha3_512(msgs[length * i:length * i + length]).digest() for i in range(n))
    assert got == want


def test_sha3_dev_on_torch_tensors(ctx):
    import torch
    n, length = 1000, 951
    msgs = _msgs(n, length, 11)
    d_in = torch.frombuffer(bytearray(msgs), dtype=torch.uint8).to("cuda")
    d_out = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.sha3_512_dev(n, length, d_in.data_ptr(), d_out.data_ptr())
    assert ctx.sync() == 0
    got = bytes(d_out.cpu().numpy().tobytes())
    assert got == b"".join(hashlib.sha3_512(msgs[length * i:length * i + length]).digest() for i in range(n))


def test_sha3_argument_errors(ctx):
    import ctypes
    from crypto12381_amd.capi import E_ARG
    out = ctypes.create_string_buffer(64)
    lib = ctx.lib
    assert lib.c12381_sha3_512_batch(ctx.h, 1, 8, None, out) == E_ARG            # message bytes missing
    assert lib.c12381_sha3_512_batch(ctx.h, 1, 8, b"12345678", None) == E_ARG    # no output
    assert lib.c12381_sha3_512_batch_dev(ctx.h, 1, 8, None, None) == E_ARG
    assert lib.c12381_sha3_512_batch(None, 1, 8, b"12345678", out) == E_ARG      # no context
    assert lib.c12381_sha3_512_batch(ctx.h, 0, 8, b"", out) == 0                 # n = 0
    assert lib.c12381_sha3_512_batch(ctx.h, 1, 0, None, out) == 0                # empty message
    assert out.raw == hashlib.sha3_512(b"").digest()
