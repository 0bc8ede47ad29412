"""The seed of g1_scalar_mul_eis (g1.hpp: the accumulator starts from the top two digits, 42 windows follow) on the device, through
c12381_g1_mul_batch (Context.g1_mul): batches of 1, 63, 64, 65 and 130 lanes that carry all sixteen values of what is left of the scalar
after 42 digits (tests/g1_eisenstein_seed.py), both values that occupy position 43 on a second point, the scalars 0, 1, r - 1, r and
2^256 - 1, and one lane each of infinity, order 3 and order 11; the other lanes carry random subgroup points.  Every output byte is compared
with the CPU oracle, computed once for all batches."""
import pytest

from g1_eisenstein_seed import occupied_scalars, one_scalar_per_top_value, top_value
from g1_torsion import enc, generator, point_of_order
from util import R, golden, prng

pytestmark = pytest.mark.gpu


def _b32(k):
    return (k % (1 << 256)).to_bytes(32, "big")


@pytest.fixture(scope="module")
def cases(oracle_port):
    """special = the lanes named above, fill = 130 random subgroup lanes, each (point, scalar, expected 96 bytes)"""
    g = golden("g1")
    gen, second = enc(generator()), bytes.fromhex(g["points"][3])
    tops = one_scalar_per_top_value()
    occ = occupied_scalars(1)
    assert [top_value(k) for k in occ] == [(3, 2), (3, 3)]
    special = [(gen, _b32(tops[t])) for t in sorted(tops)] + [(second, _b32(k)) for k in occ]
    special += [(gen, _b32(k)) for k in (0, 1, R - 1, R, (1 << 256) - 1)]
    special += [(bytes(96), _b32(occ[0])), (enc((0, 2)), _b32(occ[0])), (enc(point_of_order(11)), _b32(occ[0]))]
    fill_p = oracle_port.g1_mul(gen * 130, b"".join(_b32(prng(44111, i) % R) for i in range(130)), 96, 8)
    fill = [(fill_p[96 * i:96 * i + 96], _b32(prng(44112, i))) for i in range(130)]
    lanes = special + fill
    exp = oracle_port.g1_mul(b"".join(l[0] for l in lanes), b"".join(l[1] for l in lanes), 96, 8)
    lanes = [l + (exp[96 * i:96 * i + 96],) for i, l in enumerate(lanes)]
    return lanes[:len(special)], lanes[len(special):]


def _check(ctx, lanes):
    got = ctx.g1_mul(b"".join(l[0] for l in lanes), b"".join(l[1] for l in lanes), 96)
    bad = [i for i in range(len(lanes)) if got[96 * i:96 * i + 96] != lanes[i][2]]
    assert bad == [], (len(lanes), bad[:8], [lanes[i][1].hex() for i in bad[:4]])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_every_top_value_in_batches(cases, n):
    """n = 1: one batch per special lane.  Otherwise one batch that holds them all: on every fifth lane of 130 (lanes 0 and 65 among them),
    on every second lane counted from the last one of 63, 64 and 65"""
    from crypto12381_amd import Context
    special, fill = cases
    assert len(special) == 26
    ctx = Context(0)
    if n == 1:
        for lane in special:
            _check(ctx, [lane])
    else:
        lanes = list(fill[:n])
        for i, lane in enumerate(special):
            lanes[5 * i if n == 130 else n - 1 - 2 * i] = lane
        _check(ctx, lanes)
    ctx.close()
