"""GPU parity of hash-to-G1 and the Zp / Fp helper entries (k_hash_zp.hip, h2c.hpp, fr.hpp, fp_op_kernel) on the degenerate inputs of
h2c_zp_cases.py, through the C ABI, bit for bit: the zero SSWU denominator (the reference's off-curve pair from map_to_point, infinity
from from_hash), the u that land on the kernel of the 11-isogeny (infinity), the sign boundary, unreduced inputs and every QR / sign
class, each degenerate lane at the edges of a wavefront; cofactor clearing on small-order points and on the off-curve pair (E_POINT,
the poison record, the context usable afterwards); the 21 x 21 edge grids of the Zp and Fp operations; Zp from_hash on edge digests; the
inner-product fold at its stage boundaries, twice on one context so that the two reduction slots change roles.
Expected values: the compiled reference for map_to_point and from_hash (the same calls as tests/test_host_sim_h2c_zp.py makes), Python
integers for everything else."""
import pytest

import h2c_zp_cases as hz

pytestmark = pytest.mark.gpu

DEGENERATE = ("zero-den", "kernel")


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def side(ctx):
    """run(fn): fn with the context on a stream of its own, behind the current stream's uploads"""
    import torch
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)

    def run(fn):
        s.wait_stream(torch.cuda.current_stream(dev))
        ctx.set_stream(s.cuda_stream)
        try:
            fn()
            assert ctx.sync() == 0
        finally:
            ctx.set_stream(None)
    return run


def _up(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")


def _empty(n):
    import torch
    return torch.full((max(n, 1),), 0xa5, dtype=torch.uint8, device="cuda")


def _down(t, n):
    return t.cpu().numpy().tobytes()[:n]


def _differs(got, want, w, labels):
    assert len(got) == len(want) == w * len(labels)
    return "; ".join(str(labels[i]) for i in range(len(labels)) if got[w * i:w * i + w] != want[w * i:w * i + w])


# ---------------------------------------------------------------- map_to_point
def test_map_to_point_on_every_branch(ctx, oracle_ref):
    cases = hz.map_cases()
    labels = [(name, tag) for name, _, tag in cases]
    u48 = hz.map_bytes()
    want = oracle_ref.g1_map_to_point(u48)
    assert _differs(ctx.g1_map_to_point(u48), want, 96, labels) == ""              # no error: mode 1 never reports a bad point
    for i, (name, _, tag) in enumerate(cases):
        if tag == "zero-den":
            assert want[96 * i:96 * i + 96] == hz.enc(hz.ZERO_DEN_PAIR), name
        if tag == "kernel":
            assert want[96 * i:96 * i + 96] == bytes(96), name


@pytest.mark.parametrize("n", (1, 63, 64, 65))
def test_map_to_point_degenerate_lane_at_a_wavefront_edge(ctx, oracle_ref, n):
    """every degenerate input as the last lane of a batch of n (lane 0, 62, 63, and lane 0 of a second wavefront) behind ordinary lanes,
    and as the first lane in front of them"""
    cases = hz.map_cases()
    u48 = hz.map_bytes()
    want = oracle_ref.g1_map_to_point(u48)
    fill = [i for i, c in enumerate(cases) if c[0].startswith("seeded")]
    bad = []
    for i, (name, _, tag) in enumerate(cases):
        if tag not in DEGENERATE:
            continue
        idx = [fill[j % len(fill)] for j in range(n - 1)] + [i]
        for order in (idx, idx[::-1]):
            got = ctx.g1_map_to_point(b"".join(u48[48 * j:48 * j + 48] for j in order))
            if got != b"".join(want[96 * j:96 * j + 96] for j in order):
                bad.append((name, order is idx))
    assert bad == []


# ---------------------------------------------------------------- from_hash
@pytest.mark.parametrize("fmt", (96, 49))
def test_from_hash_on_every_branch(ctx, side, oracle_ref, fmt):
    """degenerate and seeded digests interleaved (hash_cases): the neighbours of a degenerate lane are ordinary lanes"""
    cases = hz.hash_cases()
    labels = [(name, tag) for name, _, tag in cases]
    d = hz.hash_bytes()
    n = len(cases)
    want = oracle_ref.g1_from_hash(d, fmt)
    assert sum(want[fmt * i:fmt * i + fmt] == bytes(fmt) for i in range(n)) == sum(tag in DEGENERATE for _, _, tag in cases) >= 33
    assert _differs(ctx.g1_from_hash(d, fmt), want, fmt, labels) == ""
    d_in, d_out = _up(d), _empty(fmt * n)
    side(lambda: ctx.g1_from_hash_dev(n, d_in.data_ptr(), d_out.data_ptr(), fmt))
    assert _differs(_down(d_out, fmt * n), want, fmt, labels) == ""


# ---------------------------------------------------------------- cofactor clearing
def test_clear_cofactor_on_small_order_points(ctx):
    from crypto12381_amd.capi import C12381Error, E_POINT
    cases = hz.cofactor_cases()
    labels = [c[0] for c in cases]
    pts = b"".join(c[1] for c in cases)
    on = [c for c in cases if c[2] != hz.OFF_CURVE]
    assert len(on) == len(cases) - 1
    assert _differs(ctx.g1_clear_cofactor(b"".join(c[1] for c in on)), b"".join(c[2] for c in on), 96, [c[0] for c in on]) == ""
    with pytest.raises(C12381Error) as e:
        ctx.g1_clear_cofactor(pts)
    assert e.value.code == E_POINT
    # not strict: the rejected lane carries the poison record, every other lane its multiple
    want = b"".join(b"\xff" * 96 if c[2] == hz.OFF_CURVE else c[2] for c in cases)
    assert _differs(ctx.g1_clear_cofactor(pts, strict=False), want, 96, labels) == ""
    # the flag does not outlive the call
    assert ctx.g1_clear_cofactor(on[-1][1]) == on[-1][2]
    assert ctx.g1_clear_cofactor(hz.enc(hz.ZERO_DEN_PAIR), strict=False) == b"\xff" * 96
    assert ctx.g1_clear_cofactor(b"".join(c[1] for c in on)) == b"".join(c[2] for c in on)


def test_clear_cofactor_of_map_to_point_is_from_hash(ctx, oracle_ref):
    cases = hz.map_cases()
    u48 = hz.map_bytes()
    want = oracle_ref.g1_from_hash(b"".join(bytes(16) + u48[48 * i:48 * i + 48] for i in range(len(cases))), 96)
    ok = [i for i, c in enumerate(cases) if c[2] != "zero-den"]
    img = oracle_ref.g1_map_to_point(u48)
    got = ctx.g1_clear_cofactor(b"".join(img[96 * i:96 * i + 96] for i in ok))
    assert _differs(got, b"".join(want[96 * i:96 * i + 96] for i in ok), 96, [cases[i][0] for i in ok]) == ""


# ---------------------------------------------------------------- Zp
@pytest.mark.parametrize("op", hz.ZP_OPS)
def test_zp_op_on_the_edge_grid(ctx, side, op):
    a, b, pairs = hz.zp_grid()
    n = len(pairs)
    labels = [(hex(x), hex(y)) for x, y in pairs]
    want = hz.zp_expected(op, pairs)
    binary = op in ("mul", "add", "sub")
    assert _differs(ctx.zp_op(op, a, b if binary else None), want, 32, labels) == ""
    d_a, d_b = _up(a), _up(b)
    d_out = d_a if op == "inv" else _empty(32 * n)                  # the inversion may write over its input (zp_batch_inv_kernel)
    side(lambda: ctx.zp_op_dev(op, n, d_a.data_ptr(), d_b.data_ptr() if binary else None, d_out.data_ptr()))
    assert _differs(_down(d_out, 32 * n), want, 32, labels) == ""


def test_zp_from_hash_on_edge_digests(ctx):
    assert _differs(ctx.zp_from_hash(hz.zp_digest_bytes()), hz.zp_digest_expected(), 32, [hex(x) for x in hz.ZP_DIGESTS]) == ""


@pytest.mark.parametrize("n", hz.FOLD_SIZES)
def test_zp_inner_product_at_the_stage_boundaries(ctx, n):
    a, b, dot, total = hz.fold_case(n)
    assert ctx.zp_inner_product(a, b) == dot
    assert ctx.zp_inner_product(a) == total


def test_zp_inner_product_dev_swaps_the_reduction_slots(ctx, side):
    """three stages (4097: slot 0, slot 1, out), then two (65: slot 0, out), then four, on one context and one pair of slots"""
    for n in (4097, 65, 262145, 64, 4096):
        a, b, dot, total = hz.fold_case(n)
        d_a, d_b, d_dot, d_sum = _up(a), _up(b), _empty(32), _empty(32)

        def both():
            ctx.zp_inner_product_dev(n, d_a.data_ptr(), d_b.data_ptr(), d_dot.data_ptr())
            ctx.zp_inner_product_dev(n, d_a.data_ptr(), None, d_sum.data_ptr())
        side(both)
        assert _down(d_dot, 32) == dot and _down(d_sum, 32) == total, n


# ---------------------------------------------------------------- Fp
@pytest.mark.parametrize("op", hz.FP_OPS)
def test_fp_op_on_the_edge_grid(ctx, op):
    a, b, pairs = hz.fp_grid()
    binary = op in ("mul", "add", "sub")
    got = ctx.fp_op(op, a, b if binary else None)
    assert _differs(got, hz.fp_expected(op, pairs), 48, [(hex(x), hex(y)) for x, y in pairs]) == ""
