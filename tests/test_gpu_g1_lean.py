"""The leaner single G1 product (g1.hpp: the nine-reduction mixed addition of the window loop, beta^2 x of the table as a sum) on the
device, through c12381_g1_mul_batch (Context.g1_mul): batches of 1, 63, 64, 65 and 4059 lanes in both output formats, random subgroup
lanes with the special lanes among them — points of order 3, 11 and 10177, a point outside G1 under scalars below x^2, the scalars 0, 1,
r - 1, r and 2^256 - 1 — placed in the last wavefront and in a full one.  Every output byte is compared with the CPU oracle, computed once
per lane and format for all batches; one call each with F_IN_SUBGROUP and F_COMPRESSED_IN is compared with the plain call's bytes."""
import pytest

from g1_torsion import eigenpoint, enc, generator, point_of_order
from util import P, R, golden, prng

pytestmark = pytest.mark.gpu

W = 64
NMAX = 4059


def _b32(k):
    return (k % (1 << 256)).to_bytes(32, "big")


@pytest.fixture(scope="module")
def cases(oracle_port):
    """special, fill: lists of (point, scalar, {96: expected bytes, 49: expected bytes}, in the subgroup)"""
    g = golden("g1")
    gen = enc(generator())
    ks = [prng(45001, i) % (1 << 256) for i in range(2)]
    special = [(pt, _b32(k), False) for pt in (enc((0, 2)), enc((0, P - 2)), enc(point_of_order(11)), enc(eigenpoint(10177)[0])) for k in ks]
    special += [(bytes.fromhex(p), _b32(int(s, 16)), False) for p, s in zip(g["offsubgroup_small_points"][:2], g["offsubgroup_small_scalars"][:2])]
    special += [(gen, _b32(k), True) for k in (0, 1, R - 1, R, (1 << 256) - 1)]
    special += [(bytes(96), _b32(ks[0]), True)]
    fill_p = oracle_port.g1_mul(gen * NMAX, b"".join(_b32(prng(45002, i) % R or 1) for i in range(NMAX)), 96, 8)
    fill = [(fill_p[96 * i:96 * i + 96], _b32(prng(45003, i)), True) for i in range(NMAX)]
    lanes = special + fill
    P_, S_ = b"".join(l[0] for l in lanes), b"".join(l[1] for l in lanes)
    exp = {f: oracle_port.g1_mul(P_, S_, f, 8) for f in (96, 49)}
    lanes = [(l[0], l[1], {f: exp[f][f * i:f * i + f] for f in (96, 49)}, l[2]) for i, l in enumerate(lanes)]
    return lanes[:len(special)], lanes[len(special):]


def _batch(cases, n):
    """n lanes: the fill with the special lanes on the last lanes (the last wavefront, as far as it reaches) and, where there is a full
    wavefront in front of it, on every third lane of the first one"""
    special, fill = cases
    lanes = list(fill[:n])
    for i, lane in enumerate(special):
        if n - 1 - i >= (n - 1) // W * W:
            lanes[n - 1 - i] = lane
        if n > W and 3 * i < W:
            lanes[3 * i] = lane
    return lanes


def _check(got, lanes, fmt):
    bad = [i for i in range(len(lanes)) if got[fmt * i:fmt * i + fmt] != lanes[i][2][fmt]]
    assert bad == [], (len(lanes), fmt, bad[:8], [lanes[i][1].hex() for i in bad[:4]])


@pytest.mark.parametrize("fmt", [96, 49])
@pytest.mark.parametrize("n", [1, 63, 64, 65, NMAX])
def test_batches_with_special_lanes(cases, n, fmt):
    from crypto12381_amd import Context
    ctx = Context(0)
    batches = [[lane] for lane in cases[0]] if n == 1 else [_batch(cases, n)]
    for lanes in batches:
        assert len(lanes) == n
        got = ctx.g1_mul(b"".join(l[0] for l in lanes), b"".join(l[1] for l in lanes), fmt)
        _check(got, lanes, fmt)
    if n > 1:
        assert sum(1 for l in batches[0] if not l[3]) >= 10
    ctx.close()


def test_flags_against_the_plain_call(cases, oracle_port):
    """F_COMPRESSED_IN on the 65-lane batch with its special lanes; F_IN_SUBGROUP on 65 lanes all in the subgroup (the special ones among
    them: the edge scalars and infinity)"""
    from crypto12381_amd import Context
    from crypto12381_amd.capi import F_COMPRESSED_IN, F_IN_SUBGROUP
    ctx = Context(0)
    lanes = _batch(cases, 65)
    P_, S_ = b"".join(l[0] for l in lanes), b"".join(l[1] for l in lanes)
    plain = ctx.g1_mul(P_, S_, 96)
    _check(plain, lanes, 96)
    assert ctx.g1_mul_flags(oracle_port.g1_compress(P_), S_, 96, F_COMPRESSED_IN) == plain
    special, fill = cases
    sub = [l for l in special if l[3]] + list(fill[:65])
    sub = sub[:65]
    P_, S_ = b"".join(l[0] for l in sub), b"".join(l[1] for l in sub)
    plain = ctx.g1_mul(P_, S_, 49)
    _check(plain, sub, 49)
    assert ctx.g1_mul_flags(P_, S_, 49, F_IN_SUBGROUP) == plain
    ctx.close()
