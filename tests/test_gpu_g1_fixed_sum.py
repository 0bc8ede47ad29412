"""c12381_g1_mul_fixed_sum_batch on the device, through the C ABI: per-lane sums over a set of G1 bases shared by the batch, from nb
fixed-base tables when every base is a subgroup point (k_fixed.hip g1_fixed_sum_kernel) and column by column through the generic kernel
otherwise.  The pinned value of a lane is the port oracle's `multiply` per column followed by its `add`, the addend last
(g1_fixed_sum_cases.expected).  Inputs are built on the CPU."""
import ctypes

import pytest

from g1_fixed_sum_cases import O3, OFF_CURVE, addends, edge_case, expected, generic_case, related_cases, seeded, special_bases
from g1_mul_sum_cases import INF, subgroup_pool
from util import R, golden, prng, scalars

pytestmark = pytest.mark.gpu

NBMAX = 32


@pytest.fixture(scope="module")
def ctx():
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


def differing(got, exp, w):
    assert len(got) == len(exp)
    if got == exp:
        return []
    return [i for i in range(len(exp) // w) if got[w * i:w * i + w] != exp[w * i:w * i + w]]


def to49(orc, p96):
    """the oracle's 49-byte form of 96-byte points (its add with the point at infinity, written compressed)"""
    return orc.g1_add(p96, INF * (len(p96) // 96), 49)


def dev_call(ctx, bases, sc, addend=None, fmt=96):
    """the _dev form on torch tensors -> (bytes, status of c12381_sync)"""
    import torch
    dev = torch.device("cuda", 0)
    nb = len(bases) // 96
    n = len(sc) // (32 * nb)
    t = [None if b is None else torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (bases, sc, addend)]
    out = torch.empty(fmt * n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ctx.g1_mul_fixed_sum_dev(n, nb, t[0].data_ptr(), t[1].data_ptr(), out.data_ptr(), None if addend is None else t[2].data_ptr(), fmt)
    rc = ctx.sync()
    return out.cpu().numpy().tobytes(), rc


def check_all_forms(ctx, orc, bases, sc, addend_pt, tag):
    """both formats, with and without the addend, host form; the _dev form on one of them"""
    plain = expected(orc, bases, sc)
    n = len(plain) // 96
    with_add = orc.g1_add(plain, addend_pt * n, 96)
    for addend, exp96 in ((None, plain), (addend_pt, with_add)):
        for fmt in (96, 49):
            exp = exp96 if fmt == 96 else to49(orc, exp96)
            assert differing(ctx.g1_mul_fixed_sum(bases, sc, addend, fmt), exp, fmt)[:8] == [], (tag, addend is not None, fmt)
    got, rc = dev_call(ctx, bases, sc, addend_pt, 49)
    assert rc == 0 and differing(got, to49(orc, with_add), 49)[:8] == [], tag


@pytest.mark.parametrize("nb,n", [(2, 1), (2, 63), (2, 64), (2, 65), (2, 257), (5, 1500), (NBMAX, 65)])
def test_parity_against_the_oracle(ctx, oracle_port, nb, n):
    bases, sc = seeded(oracle_port, nb, n, 9900 + nb + n)
    check_all_forms(ctx, oracle_port, bases, sc, subgroup_pool(oracle_port, 9830, 1)[0], (nb, n))


def test_one_base_equals_g1_mul_fixed(ctx, oracle_port):
    """subgroup base (table route) and bases without a table (generic route), seeded and edge scalars"""
    bases, sc = seeded(oracle_port, 1, 200, 9910)
    sc += edge_case(oracle_port, 1, 0)[1]
    for base in [bases] + [pt for _, pt in special_bases()]:
        for fmt in (49, 96):
            assert ctx.g1_mul_fixed_sum(base, sc, None, fmt) == ctx.g1_mul_fixed(base, sc, fmt)


@pytest.mark.parametrize("nb", (2, 3, 4))
def test_up_to_four_bases_equal_g1_mul_sum_on_replicated_bases(ctx, oracle_port, nb):
    for bases, sc in (seeded(oracle_port, nb, 130, 9920 + nb), edge_case(oracle_port, nb, nb - 1)):
        n = len(sc) // (32 * nb)
        pts = b"".join(bases[96 * i:96 * i + 96] * n for i in range(nb))
        for fmt in (49, 96):
            assert ctx.g1_mul_fixed_sum(bases, sc, None, fmt) == ctx.g1_mul_sum(pts, sc, nb, fmt)


@pytest.mark.parametrize("nb", (2, 3))
def test_related_bases_and_cancellations(ctx, oracle_port, nb):
    """H2 = H1, -H1, 2 H1, phi(H1) run from the tables like any other set; lanes that cancel are 96 / 49 zero bytes"""
    for kind, bases, sc, cancel in related_cases(oracle_port, nb):
        exp = expected(oracle_port, bases, sc)
        got96, got49 = ctx.g1_mul_fixed_sum(bases, sc, None, 96), ctx.g1_mul_fixed_sum(bases, sc, None, 49)
        assert differing(got96, exp, 96) == [] and differing(got49, to49(oracle_port, exp), 49) == [], kind
        for j in cancel:
            assert got96[96 * j:96 * j + 96] == bytes(96) and got49[49 * j:49 * j + 49] == bytes(49), (kind, j)


def test_addends(ctx, oracle_port):
    """absent, infinity, a subgroup point, the negative of lane 0's sum (49 / 96 zero bytes there), the point of order 3"""
    bases, sc = seeded(oracle_port, 3, 70, 9930)
    for name, addend in addends(oracle_port, bases, sc):
        exp = expected(oracle_port, bases, sc, addend)
        assert differing(ctx.g1_mul_fixed_sum(bases, sc, addend, 96), exp, 96) == [], name
        assert differing(ctx.g1_mul_fixed_sum(bases, sc, addend, 49), to49(oracle_port, exp), 49) == [], name
        if name == "-sum0":
            assert exp[:96] == bytes(96)


@pytest.mark.parametrize("name", [name for name, _ in special_bases()])
def test_generic_route(ctx, oracle_port, name):
    """a base that no table serves — off the subgroup, of order 3r, of order 3, infinity — at the first, middle and last position among
    subgroup bases, its column holding the edge scalars (those below x^2 owe the reference's [r]phi(P) term): the oracle's bytes"""
    special = dict(special_bases())[name]
    for pos in range(3):
        bases, sc = generic_case(oracle_port, 3, pos, special)
        addend = O3 if pos == 1 else None
        exp = expected(oracle_port, bases, sc, addend)
        assert differing(ctx.g1_mul_fixed_sum(bases, sc, addend, 96), exp, 96)[:8] == [], (name, pos)
        got, rc = dev_call(ctx, bases, sc, addend, 49)
        assert rc == 0 and differing(got, to49(oracle_port, exp), 49)[:8] == [], (name, pos)


def _bbs_batch(orc):
    """a BBS+ batch of four with nmsg = 3 (signed as examples/bbs-plus/src/bbs+.cpp:38-55 signs): lanes 1 and 3 carry a wrong message"""
    nmsg, n = 3, 4
    g1, g2 = bytes.fromhex(golden("g1")["generator"]), bytes.fromhex(golden("g2")["generator"])
    gs = orc.g1_mul(g1 * (nmsg + 2), scalars(9941, nmsg + 2), 96)
    G1p, h0, h = gs[:96], gs[96:192], gs[192:]
    G2p = orc.g2_mul(g2, scalars(9942, 1), 192)
    gamma = prng(9943, 0) % R
    w = orc.g2_mul(G2p, gamma.to_bytes(32, "big"), 192)
    A, X, Rr, M = b"", b"", b"", [b""] * nmsg
    for j in range(n):
        msgs = [prng(9944 + i, j) % R for i in range(nmsg)]
        x, r = prng(9948, j) % R, prng(9949, j) % R
        B = orc.g1_msm(G1p + h0 + h, (1).to_bytes(32, "big") + r.to_bytes(32, "big") + b"".join(m.to_bytes(32, "big") for m in msgs), 96, 1)
        A += orc.g1_mul(B, pow((gamma + x) % R, -1, R).to_bytes(32, "big"), 96)
        if j % 2:
            msgs[j % nmsg] = (msgs[j % nmsg] + 1) % R
        X += x.to_bytes(32, "big")
        Rr += r.to_bytes(32, "big")
        for i in range(nmsg):
            M[i] += msgs[i].to_bytes(32, "big")
    return (G1p, G2p, h0, h, w, A, X, Rr, b"".join(M)), b"\x01\x00\x01\x00"


def test_table_cache(ctx, oracle_port):
    """one table per base position, rebuilt when its base changes: a set of bases, base j replaced, put back, the set permuted — every
    result is the oracle's; g1_mul_fixed and a BBS+ verification in between keep their results (the table slots do not collide); and
    after c12381_trim the next call rebuilds what it needs"""
    nb, n = 4, 70
    bases, sc = seeded(oracle_port, nb, n, 9950)
    other = subgroup_pool(oracle_port, 9951, 2)
    exp = expected(oracle_port, bases, sc)
    bbs_args, bbs_ok = _bbs_batch(oracle_port)
    fixed_sc = scalars(9952, 50)
    fixed_before = ctx.g1_mul_fixed(other[1], fixed_sc, 96)
    assert ctx.bbs_plus_verify(*bbs_args) == bbs_ok
    assert ctx.g1_mul_fixed_sum(bases, sc, None, 96) == exp
    assert ctx.g1_mul_fixed_sum(bases, sc, None, 96) == exp                      # every table cached
    for j in (0, 2, 3):
        changed = bases[:96 * j] + other[0] + bases[96 * (j + 1):]
        assert ctx.g1_mul_fixed_sum(changed, sc, None, 96) == expected(oracle_port, changed, sc), j
        assert ctx.g1_mul_fixed(other[1], fixed_sc, 96) == fixed_before
        assert ctx.g1_mul_fixed_sum(bases, sc, None, 96) == exp, j
        assert ctx.bbs_plus_verify(*bbs_args) == bbs_ok
    perm = bases[96 * 3:] + bases[96:96 * 3] + bases[:96]
    assert ctx.g1_mul_fixed_sum(perm, sc, None, 96) == expected(oracle_port, perm, sc)
    assert ctx.g1_mul_fixed_sum(bases[:96 * 2], sc[:32 * n * 2], None, 96) == expected(oracle_port, bases[:96 * 2], sc[:32 * n * 2])     # fewer bases
    assert ctx.g1_mul_fixed_sum(bases, sc, None, 96) == exp
    # a base without a table in between: the generic route, then the tables again
    mixed = bases[:96] + O3 + bases[96 * 2:]
    assert ctx.g1_mul_fixed_sum(mixed, sc, None, 96) == expected(oracle_port, mixed, sc)
    assert ctx.g1_mul_fixed_sum(bases, sc, None, 96) == exp
    ctx.trim()
    assert ctx.g1_mul_fixed_sum(bases, sc, None, 96) == exp
    assert ctx.g1_mul_fixed(other[1], fixed_sc, 96) == fixed_before
    assert ctx.bbs_plus_verify(*bbs_args) == bbs_ok


# ---------------------------------------------------------------- the argument contract (the shape of test_gpu_fixed_k_contract.py)
def test_argument_errors(ctx, oracle_port):
    from crypto12381_amd.capi import E_ARG, _p
    bases, sc = seeded(oracle_port, NBMAX, 4, 9960)
    bases += bases[:96]                                                          # room for nb = 33
    sc += sc[:32 * 4]
    out = ctypes.create_string_buffer(96 * 4)
    for name in ("c12381_g1_mul_fixed_sum_batch", "c12381_g1_mul_fixed_sum_batch_dev"):
        f = getattr(ctx.lib, name)
        assert f(ctx.h, 4, 0, _p(bases), None, _p(sc), _p(out), 96) == E_ARG              # nb = 0
        assert f(ctx.h, 4, NBMAX + 1, _p(bases), None, _p(sc), _p(out), 96) == E_ARG      # nb > C12381_G1_FIXED_SUM_MAX
        assert f(ctx.h, 4, 2, _p(bases), None, _p(sc), _p(out), 48) == E_ARG              # out_fmt
        assert f(ctx.h, 4, 2, _p(bases), None, _p(sc), _p(out), 97) == E_ARG
        assert f(ctx.h, 4, 2, None, None, _p(sc), _p(out), 96) == E_ARG
        assert f(ctx.h, 4, 2, _p(bases), None, None, _p(out), 96) == E_ARG
        assert f(ctx.h, 4, 2, _p(bases), None, _p(sc), None, 96) == E_ARG
        assert f(None, 4, 2, _p(bases), None, _p(sc), _p(out), 96) == E_ARG
        assert f(ctx.h, 0, 0, _p(bases), None, _p(sc), _p(out), 96) == E_ARG              # checks before the empty-batch rule
        assert f(ctx.h, 0, 2, _p(bases), None, _p(sc), None, 96) == E_ARG
    assert ctx.sync() == 0


def test_empty_batch_leaves_the_output(ctx, oracle_port):
    from crypto12381_amd.capi import _p
    bases, sc = seeded(oracle_port, 3, 4, 9961)
    out = ctypes.create_string_buffer(b"\xab" * 96, 96)
    for name in ("c12381_g1_mul_fixed_sum_batch", "c12381_g1_mul_fixed_sum_batch_dev"):
        f = getattr(ctx.lib, name)
        assert f(ctx.h, 0, 3, _p(bases), None, _p(sc), _p(out), 96) == 0
        assert f(ctx.h, 0, 3, _p(bases), _p(bases), _p(sc), _p(out), 49) == 0
    assert out.raw == b"\xab" * 96
    assert ctx.sync() == 0
    assert ctx.g1_mul_fixed_sum(bases, b"", None, 96) == b""


def test_host_form_equals_dev_form(ctx, oracle_port):
    bases, sc = seeded(oracle_port, 6, 130, 9962)
    addend = subgroup_pool(oracle_port, 9830, 1)[0]
    for a in (None, addend):
        for fmt in (49, 96):
            got, rc = dev_call(ctx, bases, sc, a, fmt)
            assert rc == 0 and got == ctx.g1_mul_fixed_sum(bases, sc, a, fmt)


def test_a_point_off_the_curve_poisons_the_batch(ctx, oracle_port):
    """an off-curve base (first, last) or addend: every output byte 0xff, C12381_E_POINT from the host form or from c12381_sync — once —
    and the next clean call is right"""
    from crypto12381_amd.capi import C12381Error, E_POINT
    nb, n = 3, 70
    bases, sc = seeded(oracle_port, nb, n, 9963)
    addend = subgroup_pool(oracle_port, 9830, 1)[0]
    exp = expected(oracle_port, bases, sc, addend)
    bad = [(OFF_CURVE + bases[96:], addend), (bases[:96 * 2] + OFF_CURVE, None), (bases, OFF_CURVE), (bases[:96] + O3 + OFF_CURVE, OFF_CURVE)]
    for b, a in bad:
        with pytest.raises(C12381Error) as e:
            ctx.g1_mul_fixed_sum(b, sc, a, 96)
        assert e.value.code == E_POINT
        for fmt in (96, 49):
            assert ctx.g1_mul_fixed_sum(b, sc, a, fmt, strict=False) == b"\xff" * (fmt * n)
            got, rc = dev_call(ctx, b, sc, a, fmt)
            assert rc == E_POINT and got == b"\xff" * (fmt * n)
            assert ctx.sync() == 0                                                 # the status was collected once
        assert ctx.g1_mul_fixed_sum(bases, sc, addend, 96) == exp
    got, rc = dev_call(ctx, bases, sc, addend, 96)
    assert rc == 0 and got == exp
