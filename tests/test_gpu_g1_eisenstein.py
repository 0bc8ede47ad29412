"""g1_scalar_mul_eis (g1.hpp: base-8 Eisenstein digits) on the device, through c12381_g1_mul_batch (Context.g1_mul): batches of 1, 63, 64, 65 and 130
lanes whose lanes 0, 31, 32, 63 and 64 carry the edge scalars (tests/g1_eisenstein.py edge_scalars) on the generator, a second subgroup
point, the point at infinity, the two points of order 3 (which take the complete path) and a point off the subgroup; the other lanes
carry random subgroup points.  Every output byte is compared with the CPU oracle, computed once for all batches."""
import pytest

from g1_eisenstein import edge_scalars
from g1_torsion import enc, generator
from util import P, R, golden, prng

pytestmark = pytest.mark.gpu

SPECIAL = (0, 31, 32, 63, 64)
OFF_CURVE = (1).to_bytes(48, "big") + (1).to_bytes(48, "big")


def _b32(k):
    return (k % (1 << 256)).to_bytes(32, "big")


@pytest.fixture(scope="module")
def cases(oracle_port):
    """combos = every (edge point, edge scalar) with its expected 96 and 49 bytes; fill = 130 random subgroup lanes with theirs"""
    g = golden("g1")
    pts = [enc(generator()), bytes.fromhex(g["points"][3]), bytes(96), enc((0, 2)), enc((0, P - 2)), bytes.fromhex(g["offsubgroup_points"][1])]
    ks = edge_scalars()
    combos = [(pb, _b32(k)) for k in ks for pb in pts]
    fill_p = oracle_port.g1_mul(enc(generator()) * 130, b"".join(_b32(prng(44101, i) % R) for i in range(130)), 96, 8)
    fill = [(fill_p[96 * i:96 * i + 96], _b32(prng(44102, i))) for i in range(130)]
    allp = b"".join(c[0] for c in combos + fill)
    alls = b"".join(c[1] for c in combos + fill)
    exp = {fmt: oracle_port.g1_mul(allp, alls, fmt, 8) for fmt in (96, 49)}
    m = len(combos)
    cut = lambda fmt, i: exp[fmt][fmt * i:fmt * i + fmt]
    return ([c + (cut(96, i), cut(49, i)) for i, c in enumerate(combos)],
            [c + (cut(96, m + i), cut(49, m + i)) for i, c in enumerate(fill)])


def _batch(n, combos, fill, first):
    """n lanes: fill lanes, with combos[first], combos[first + 1], ... on the special lanes below n"""
    lanes = list(fill[:n])
    for j, lane in enumerate(l for l in SPECIAL if l < n):
        lanes[lane] = combos[(first + j) % len(combos)]
    return lanes


def _check(ctx, lanes, fmt):
    got = ctx.g1_mul(b"".join(l[0] for l in lanes), b"".join(l[1] for l in lanes), fmt)
    exp = b"".join(l[2 if fmt == 96 else 3] for l in lanes)
    bad = [i for i in range(len(lanes)) if got[fmt * i:fmt * i + fmt] != exp[fmt * i:fmt * i + fmt]]
    assert bad == [], (len(lanes), fmt, bad[:8], [lanes[i][1].hex() for i in bad[:4]])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_edge_lanes_in_batches(cases, n):
    """n = 130 walks through every (point, scalar) combination, five per batch; the smaller sizes take a stride through them"""
    from crypto12381_amd import Context
    combos, fill = cases
    per = sum(1 for l in SPECIAL if l < n)
    starts = range(0, len(combos), per) if n == 130 else range(n % 7, len(combos), 97)
    ctx = Context(0)
    for b, first in enumerate(starts):
        _check(ctx, _batch(n, combos, fill, first), 96 if b % 2 == 0 else 49)
    ctx.close()


def test_rejected_input_leaves_the_invalid_mark(cases):
    """a point off the curve on lane 31 of 65, between an order-3 lane and subgroup lanes: E_POINT in strict mode, 0xff bytes on that lane
    otherwise and every other lane unchanged"""
    from crypto12381_amd import Context
    from crypto12381_amd.capi import C12381Error, E_POINT
    combos, fill = cases
    lanes = _batch(65, combos, fill, 9)                       # lane 0 = the first order-3 point with scalar 1
    pts = b"".join(OFF_CURVE if i == 31 else l[0] for i, l in enumerate(lanes))
    sc = b"".join(l[1] for l in lanes)
    ctx = Context(0)
    for fmt in (96, 49):
        with pytest.raises(C12381Error) as e:
            ctx.g1_mul(pts, sc, fmt)
        assert e.value.code == E_POINT
        got = ctx.g1_mul(pts, sc, fmt, strict=False)
        exp = b"".join(b"\xff" * fmt if i == 31 else l[2 if fmt == 96 else 3] for i, l in enumerate(lanes))
        assert got == exp
    ctx.close()
