"""The G1 bucket product on the device (c12381_g1_msm: prep, sort, ranges, sizes and overflow bookkeeping, bucket sums, overflow sums,
overflow combine, window reduction, wave folds, Horner, small-scalar term) on the constructed inputs of msm_cases.py: equal and opposite
points in one bucket, buckets, segments, windows and products at infinity, the two records of a term meeting those of another, chosen
digits, edge scalars, run lengths at the seams of the cut (cap, cap + 1, cap + sl, cap + sl + 1, more than 64 segments of one bucket,
segment lists that straddle a wavefront), the small-scalar bucket with a sum at infinity, inside and outside G1, and the switches of
width (c = 8 -> 16 at 4096 terms) and of key size (2^15 terms).  Every result is compared byte for byte with a value computed on the CPU:
Python integers where every point is in G1, the oracle's chain of multiply() results otherwise.  Through the host entry in both output
formats, the _dev entry on torch tensors, compressed input, and as a sequence of products on one context in both orders."""
import pytest

import msm_cases as mc
from util import golden, prng, scalars

pytestmark = pytest.mark.gpu

ORDER = ["e:long-run", "a:P,-P", "f:S-outside/sum-of-two", "b:zero-scalars", "e:long-run"]


@pytest.fixture(scope="module")
def ctx():
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", mc.NAMES)
def test_product(ctx, oracle_port, name):
    """every case, 96-byte output"""
    pts, sc = mc.case(name).pack()
    assert ctx.g1_msm(pts, sc, 96) == mc.expected96(name, oracle_port)


@pytest.mark.parametrize("name", mc.family("a") + mc.family("b") + mc.family("f"))
def test_product_compressed_output(ctx, oracle_port, name):
    """49-byte output: infinity is 49 zero bytes"""
    pts, sc = mc.case(name).pack()
    exp = mc.expected96(name, oracle_port)
    assert mc.enc49(exp) == oracle_port.g1_compress(exp)
    assert ctx.g1_msm(pts, sc, 49) == mc.enc49(exp)


@pytest.mark.parametrize("name", mc.family("e"))
def test_run_lengths_on_device_buffers(ctx, oracle_port, name):
    """the _dev entry on torch tensors: the output was filled with 0x5a, the stream reports no invalid point"""
    import torch
    dev = torch.device("cuda", 0)
    c = mc.case(name)
    pts, sc = c.pack()
    dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).to(dev)
    ds = torch.frombuffer(bytearray(sc), dtype=torch.uint8).to(dev)
    for fmt in (96, 49):
        out = torch.full((fmt + 32,), 0x5a, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ctx.g1_msm_dev(c.n, dp.data_ptr(), ds.data_ptr(), out.data_ptr(), fmt)
        assert ctx.sync() == 0
        got = out.cpu().numpy().tobytes()
        exp = mc.expected96(name, oracle_port)
        assert got[:fmt] == (exp if fmt == 96 else mc.enc49(exp)) and got[fmt:] == b"\x5a" * 32


@pytest.mark.parametrize("name", mc.family("a") + mc.family("d"))
def test_compressed_input(ctx, oracle_port, name):
    """C12381_F_COMPRESSED_IN: the points compressed by the oracle; then with one more lane whose encoding starts with 00 and goes on
    with the bytes of a coordinate, which is the point at infinity whatever follows (g1_parse49)"""
    from crypto12381_amd.capi import F_COMPRESSED_IN
    pts, sc = mc.case(name).pack()
    exp = mc.expected96(name, oracle_port)
    c49 = oracle_port.g1_compress(pts)
    assert ctx.g1_msm_flags(c49, sc, 96, F_COMPRESSED_IN) == exp
    lane = b"\x00" + mc.POOL[5][0].to_bytes(48, "big")
    k = prng(9830, 0, 32).to_bytes(32, "big")
    assert ctx.g1_msm_flags(lane + c49, k + sc, 96, F_COMPRESSED_IN) == exp
    assert ctx.g1_msm_flags(c49 + lane, sc + k, 49, F_COMPRESSED_IN) == mc.enc49(exp)


def test_products_in_either_order_on_one_context(oracle_port):
    """a heavily cut product, a two-term product, a small-scalar bucket outside G1, a product of nothing, the cut product again — then the
    same list backwards on the same context: ranges, overflow counters and the "term written" flag of one product do not reach the next"""
    from crypto12381_amd import Context
    assert mc.case(ORDER[0]).model()["segments"] > 2000 and not mc.case(ORDER[1]).model()["cut"]
    assert mc.expected96(ORDER[2], oracle_port) != bytes(96) and mc.case(ORDER[2]).model()["small"] == 2
    c = Context(0)
    try:
        for names in (ORDER, ORDER[::-1]):
            for fmt in (96, 49):
                for name in names:
                    exp = mc.expected96(name, oracle_port)
                    assert c.g1_msm(*mc.case(name).pack(), fmt) == (exp if fmt == 96 else mc.enc49(exp)), (name, fmt, names is ORDER)
    finally:
        c.close()


def test_product_after_a_refused_one(oracle_port):
    """a term that is not on the curve raises (the contract of test_gpu_api_contract.py); the next product on that context is whole"""
    from crypto12381_amd import C12381Error, Context
    p_good = bytes.fromhex(golden("g1")["points"][0])
    p_bad = p_good[:95] + bytes([p_good[95] ^ 1])
    c = Context(0)
    try:
        for name in ("e:seams", "e:straddle"):
            with pytest.raises(C12381Error):
                c.g1_msm(p_good + p_bad, scalars(961, 2), 49)
            assert c.g1_msm(*mc.case(name).pack(), 96) == mc.expected96(name, oracle_port), name
    finally:
        c.close()
