"""c12381_g2_mul_fixed_sum_batch on the device, through the C ABI: per-lane sums over a set of G2 bases shared by the batch, from nb
fixed-base tables when every base is an element of G2 (k_fixed.hip g2_fixed_sum_kernel) and column by column through the generic kernel
otherwise.  The pinned value of a lane is the port oracle's `multiply` per column followed by its `add`, the addend last
(g2_fixed_sum_cases.expected).  Inputs are built on the CPU."""
import ctypes

import pytest

from g1_torsion import ec_mul as g1_ec_mul
from g1_torsion import enc as g1_enc
from g1_torsion import generator as g1_generator
from g2_fixed_sum_cases import (G2GEN, INF, OFF_TWIST, addends, b32, edge_case, expected, generic_case, related_cases, seeded, special_bases,
                                subgroup_pool)
from util import R, prng, scalars

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


def to97(orc, p192):
    """the oracle's 97-byte form of 192-byte points (its add with the point at infinity, written compressed)"""
    return orc.g2_add(p192, INF * (len(p192) // 192), 97)


def dev_call(ctx, bases, sc, addend=None, fmt=192):
    """the _dev form on torch tensors -> (bytes, status of c12381_sync)"""
    import torch
    dev = torch.device("cuda", 0)
    nb = len(bases) // 192
    n = len(sc) // (32 * nb)
    t = [None if b is None else torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (bases, sc, addend)]
    out = torch.empty(fmt * n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ctx.g2_mul_fixed_sum_dev(n, nb, t[0].data_ptr(), t[1].data_ptr(), out.data_ptr(), None if addend is None else t[2].data_ptr(), fmt)
    rc = ctx.sync()
    return out.cpu().numpy().tobytes(), rc


def check_all_forms(ctx, orc, bases, sc, addend_pt, tag, dev=False):
    """both formats, with and without the addend, host form; the _dev form where asked"""
    plain = expected(orc, bases, sc)
    n = len(plain) // 192
    with_add = orc.g2_add(plain, addend_pt * n, 192)
    for addend, exp192 in ((None, plain), (addend_pt, with_add)):
        for fmt in (192, 97):
            exp = exp192 if fmt == 192 else to97(orc, exp192)
            assert differing(ctx.g2_mul_fixed_sum(bases, sc, addend, fmt), exp, fmt)[:8] == [], (tag, addend is not None, fmt)
    if dev:
        got, rc = dev_call(ctx, bases, sc, addend_pt, 97)
        assert rc == 0 and differing(got, to97(orc, with_add), 97)[:8] == [], tag


@pytest.mark.parametrize("nb,n", [(2, 1), (2, 63), (2, 64), (2, 65), (2, 257), (5, 300), (NBMAX, 65)])
def test_parity_against_the_oracle(ctx, oracle_port, nb, n):
    """the wavefront boundary, the block boundary (one block and a lane), several blocks, the largest table array"""
    bases, sc = seeded(oracle_port, nb, n, 9800 + nb + n)
    check_all_forms(ctx, oracle_port, bases, sc, subgroup_pool(oracle_port, 9730, 1)[0], (nb, n), dev=(nb, n) == (2, 257))


def test_one_base_equals_g2_mul_fixed(ctx, oracle_port):
    """an element of G2 (table route) and bases without a table (generic route), seeded and edge scalars"""
    bases, sc = seeded(oracle_port, 1, 100, 9810)
    sc += edge_case(oracle_port, 1, 0)[1]
    for base in [bases] + [pt for _, pt in special_bases()]:
        for fmt in (97, 192):
            assert ctx.g2_mul_fixed_sum(base, sc, None, fmt) == ctx.g2_mul_fixed(base, sc, fmt)
    assert ctx.g2_mul_fixed_sum(bases, sc, None, 192) == expected(oracle_port, bases, sc)


@pytest.mark.parametrize("nb", (2, 3))
def test_related_bases_and_cancellations(ctx, oracle_port, nb):
    """H2 = H1, -H1, 2 H1, psi(H1) run from the tables like any other set; lanes that cancel are 192 / 97 zero bytes"""
    for kind, bases, sc, cancel in related_cases(oracle_port, nb):
        exp = expected(oracle_port, bases, sc)
        got192, got97 = ctx.g2_mul_fixed_sum(bases, sc, None, 192), ctx.g2_mul_fixed_sum(bases, sc, None, 97)
        assert differing(got192, exp, 192) == [] and differing(got97, to97(oracle_port, exp), 97) == [], kind
        assert len(cancel) >= 5
        for j in cancel:
            assert exp[192 * j:192 * j + 192] == bytes(192), (kind, j)
            assert got192[192 * j:192 * j + 192] == bytes(192) and got97[97 * j:97 * j + 97] == bytes(97), (kind, j)


def test_addends(ctx, oracle_port):
    """absent, infinity, an element of G2, the negative of lane 0's sum (97 / 192 zero bytes there), a twist point of order 13"""
    bases, sc = seeded(oracle_port, 3, 70, 9830)
    for name, addend in addends(oracle_port, bases, sc):
        exp = expected(oracle_port, bases, sc, addend)
        assert differing(ctx.g2_mul_fixed_sum(bases, sc, addend, 192), exp, 192) == [], name
        assert differing(ctx.g2_mul_fixed_sum(bases, sc, addend, 97), to97(oracle_port, exp), 97) == [], name
        if name == "-sum0":
            assert exp[:192] == bytes(192)


@pytest.mark.parametrize("name", [name for name, _ in special_bases()])
def test_generic_route(ctx, oracle_port, name):
    """a base that no table serves — of order 13, of order 13 r, infinity — at the first, middle and last position among elements of G2, its
    column holding the edge scalars (zero odd GS digits owe the reference's [r]psi^i(Q) terms): the oracle's bytes"""
    special = dict(special_bases())[name]
    t13 = dict(special_bases())["t13a"]
    for pos in range(3):
        bases, sc = generic_case(oracle_port, 3, pos, special)
        addend = t13 if pos == 1 else None
        exp = expected(oracle_port, bases, sc, addend)
        assert differing(ctx.g2_mul_fixed_sum(bases, sc, addend, 192), exp, 192)[:8] == [], (name, pos)
        got, rc = dev_call(ctx, bases, sc, addend, 97)
        assert rc == 0 and differing(got, to97(oracle_port, exp), 97)[:8] == [], (name, pos)


def _ps_batch(orc):
    """a PS batch of four with nmsg = 2 (signed as examples/ps/src/ps.cpp signs: s1 = h, s2 = h^(x + sum y_i m_i)): lanes 1 and 3 carry a
    wrong message.  -> (arguments of ps_verify, expected verdicts)"""
    nmsg, n = 2, 4
    x, y = prng(9841, 0) % R, [prng(9841, 1 + i) % R for i in range(nmsg)]
    X2 = orc.g2_mul(G2GEN, b32(x), 192, 1)
    Y2 = b"".join(orc.g2_mul(G2GEN, b32(v), 192, 1) for v in y)
    g = g1_generator()
    s1, s2, m = b"", b"", [b""] * nmsg
    for j in range(n):
        msgs = [prng(9842 + i, j) % R for i in range(nmsg)]
        h = g1_ec_mul(prng(9845, j) % R or 1, g)
        s1 += g1_enc(h)
        s2 += g1_enc(g1_ec_mul((x + sum(a * b for a, b in zip(y, msgs))) % R, h))
        if j % 2:
            msgs[j % nmsg] = (msgs[j % nmsg] + 1) % R
        for i in range(nmsg):
            m[i] += b32(msgs[i])
    return (G2GEN, X2, Y2, s1, s2, b"".join(m)), b"\x01\x00\x01\x00"


def test_table_cache(ctx, oracle_port):
    """one table per base position, rebuilt when its base changes: a set of bases, base j replaced, put back, the set permuted, fewer bases,
    a base without a table in between — every result is the oracle's; g2_mul_fixed and a PS verification in between keep their results
    (the table slots do not collide); and after c12381_trim the next call rebuilds what it needs"""
    nb, n = 4, 70
    bases, sc = seeded(oracle_port, nb, n, 9850)
    other = subgroup_pool(oracle_port, 9851, 2)
    exp = expected(oracle_port, bases, sc)
    ps_args, ps_ok = _ps_batch(oracle_port)
    fixed_sc = scalars(9852, 50)
    fixed_want = oracle_port.g2_mul(other[1] * 50, fixed_sc, 192, 8)
    assert ctx.g2_mul_fixed(other[1], fixed_sc, 192) == fixed_want
    assert ctx.ps_verify(*ps_args) == ps_ok
    assert ctx.g2_mul_fixed_sum(bases, sc, None, 192) == exp
    assert ctx.g2_mul_fixed_sum(bases, sc, None, 192) == exp                     # every table cached
    for j in (0, 2, 3):
        changed = bases[:192 * j] + other[0] + bases[192 * (j + 1):]
        assert ctx.g2_mul_fixed_sum(changed, sc, None, 192) == expected(oracle_port, changed, sc), j
        assert ctx.g2_mul_fixed(other[1], fixed_sc, 192) == fixed_want
        assert ctx.g2_mul_fixed_sum(bases, sc, None, 192) == exp, j
        assert ctx.ps_verify(*ps_args) == ps_ok
    perm = bases[192 * 3:] + bases[192:192 * 3] + bases[:192]
    assert ctx.g2_mul_fixed_sum(perm, sc, None, 192) == expected(oracle_port, perm, sc)
    assert ctx.g2_mul_fixed_sum(bases[:192 * 2], sc[:32 * n * 2], None, 192) == expected(oracle_port, bases[:192 * 2], sc[:32 * n * 2])     # fewer bases
    assert ctx.g2_mul_fixed_sum(bases, sc, None, 192) == exp
    # a base without a table in between: the generic route, then the tables again
    mixed = bases[:192] + dict(special_bases())["t13a"] + bases[192 * 2:]
    assert ctx.g2_mul_fixed_sum(mixed, sc, None, 192) == expected(oracle_port, mixed, sc)
    assert ctx.g2_mul_fixed_sum(bases, sc, None, 192) == exp
    ctx.trim()
    assert ctx.g2_mul_fixed_sum(bases, sc, None, 192) == exp
    assert ctx.g2_mul_fixed(other[1], fixed_sc, 192) == fixed_want
    assert ctx.ps_verify(*ps_args) == ps_ok


# ---------------------------------------------------------------- the argument contract (the shape of test_gpu_g1_fixed_sum.py)
def test_argument_errors(ctx, oracle_port):
    from crypto12381_amd.capi import E_ARG, _p
    bases, sc = seeded(oracle_port, NBMAX, 4, 9860)
    bases += bases[:192]                                                         # room for nb = 33
    sc += sc[:32 * 4]
    out = ctypes.create_string_buffer(192 * 4)
    for name in ("c12381_g2_mul_fixed_sum_batch", "c12381_g2_mul_fixed_sum_batch_dev"):
        f = getattr(ctx.lib, name)
        assert f(ctx.h, 4, 0, _p(bases), None, _p(sc), _p(out), 192) == E_ARG             # nb = 0
        assert f(ctx.h, 4, NBMAX + 1, _p(bases), None, _p(sc), _p(out), 192) == E_ARG     # nb > C12381_G2_FIXED_SUM_MAX
        assert f(ctx.h, 4, 2, _p(bases), None, _p(sc), _p(out), 96) == E_ARG              # out_fmt
        assert f(ctx.h, 4, 2, _p(bases), None, _p(sc), _p(out), 49) == E_ARG
        assert f(ctx.h, 4, 2, None, None, _p(sc), _p(out), 192) == E_ARG
        assert f(ctx.h, 4, 2, _p(bases), None, None, _p(out), 192) == E_ARG
        assert f(ctx.h, 4, 2, _p(bases), None, _p(sc), None, 192) == E_ARG
        assert f(None, 4, 2, _p(bases), None, _p(sc), _p(out), 192) == E_ARG
        assert f(ctx.h, 0, 0, _p(bases), None, _p(sc), _p(out), 192) == E_ARG             # checks before the empty-batch rule
        assert f(ctx.h, 0, 2, _p(bases), None, _p(sc), None, 192) == E_ARG
    assert ctx.sync() == 0


def test_empty_batch_leaves_the_output(ctx, oracle_port):
    from crypto12381_amd.capi import _p
    bases, sc = seeded(oracle_port, 3, 4, 9861)
    out = ctypes.create_string_buffer(b"\xab" * 192, 192)
    for name in ("c12381_g2_mul_fixed_sum_batch", "c12381_g2_mul_fixed_sum_batch_dev"):
        f = getattr(ctx.lib, name)
        assert f(ctx.h, 0, 3, _p(bases), None, _p(sc), _p(out), 192) == 0
        assert f(ctx.h, 0, 3, _p(bases), _p(bases), _p(sc), _p(out), 97) == 0
    assert out.raw == b"\xab" * 192
    assert ctx.sync() == 0
    assert ctx.g2_mul_fixed_sum(bases, b"", None, 192) == b""


def test_host_form_equals_dev_form(ctx, oracle_port):
    bases, sc = seeded(oracle_port, 6, 130, 9862)
    addend = subgroup_pool(oracle_port, 9730, 1)[0]
    for a in (None, addend):
        for fmt in (97, 192):
            got, rc = dev_call(ctx, bases, sc, a, fmt)
            assert rc == 0 and got == ctx.g2_mul_fixed_sum(bases, sc, a, fmt)


def test_a_point_off_the_twist_poisons_the_batch(ctx, oracle_port):
    """an off-twist base (first, last) or addend: every output byte 0xff, C12381_E_POINT from the host form or from c12381_sync — once —
    and the next clean call is right"""
    from crypto12381_amd.capi import C12381Error, E_POINT
    nb, n = 3, 70
    bases, sc = seeded(oracle_port, nb, n, 9863)
    addend = subgroup_pool(oracle_port, 9730, 1)[0]
    exp = expected(oracle_port, bases, sc, addend)
    t13 = dict(special_bases())["t13a"]
    bad = [(OFF_TWIST + bases[192:], addend), (bases[:192 * 2] + OFF_TWIST, None), (bases, OFF_TWIST), (bases[:192] + t13 + OFF_TWIST, OFF_TWIST)]
    for b, a in bad:
        with pytest.raises(C12381Error) as e:
            ctx.g2_mul_fixed_sum(b, sc, a, 192)
        assert e.value.code == E_POINT
        for fmt in (192, 97):
            assert ctx.g2_mul_fixed_sum(b, sc, a, fmt, strict=False) == b"\xff" * (fmt * n)
            got, rc = dev_call(ctx, b, sc, a, fmt)
            assert rc == E_POINT and got == b"\xff" * (fmt * n)
            assert ctx.sync() == 0                                                 # the status was collected once
        assert ctx.g2_mul_fixed_sum(bases, sc, addend, 192) == exp
    got, rc = dev_call(ctx, bases, sc, addend, 192)
    assert rc == 0 and got == exp
