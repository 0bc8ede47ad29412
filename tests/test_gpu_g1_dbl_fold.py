"""The folded Jacobian doubling (g1.hpp g1j_dbl) on the device, through the entry points whose window loops run it:
c12381_g1_mul_batch on 4096 lanes (sixteen workgroups) and on 4096 - 37 (a partial last wavefront), c12381_g1_mul_sum_batch with
k = 2 and 4 on 1024 lanes.  Inputs: random subgroup points with random scalars, the edge scalars (0, 1, r - 1, r, 2^256 - 1 and the rest
of g1_torsion.edge_scalars), scalars below x^2, the point at infinity, (0, +-2) and the other torsion points of g1_torsion.py.  Every
lane is byte-equal to the CPU oracle in the 96-byte and the 49-byte output; every input is computed on the CPU."""
import pytest

from g1_mul_sum_cases import edge_lanes, expected, pack, related_lanes, seeded_lanes, special_points, subgroup_pool
from g1_torsion import X2, edge_scalars
from util import P, prng

pytestmark = pytest.mark.gpu

N = 4096
TAIL = 37
NSUM = 1024


def _b32(k):
    return (k % (1 << 256)).to_bytes(32, "big")


@pytest.fixture(scope="module")
def ctx():
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch(oracle_port):
    """(points, scalars, tags, {fmt: expected}) of N lanes; special lanes are spread over the batch (every fifth lane) so that every
    workgroup holds some, and the last TAIL lanes — the ones the shorter run drops — are ordinary ones"""
    pool = subgroup_pool(oracle_port, 9951, 256)
    special = [(name, pt, k) for name, pt in special_points() + [("o3b", (0).to_bytes(48, "big") + (P - 2).to_bytes(48, "big"))] for k in edge_scalars()]
    assert {0, 1} <= set(edge_scalars()) and len(special) <= (N - TAIL) // 5
    lanes = []
    for i in range(N):
        if i % 5 == 3 and i // 5 < len(special):
            lanes.append(special[i // 5])
        elif i % 5 == 0:                                    # below x^2: the [r]phi(P) term of the reference
            lanes.append(("below", pool[i % 256], prng(9952, i) % X2))
        else:
            lanes.append(("sub", pool[(i * 31) % 256], prng(9953, i) % (1 << 256)))
    pts = b"".join(ln[1] for ln in lanes)
    sc = b"".join(_b32(ln[2]) for ln in lanes)
    exp = {fmt: oracle_port.g1_mul(pts, sc, fmt, 8) for fmt in (96, 49)}
    return pts, sc, [(ln[0], ln[2]) for ln in lanes], exp


@pytest.mark.parametrize("n", (N, N - TAIL))
def test_g1_mul_every_lane_equals_the_oracle(ctx, batch, n):
    pts, sc, tags, exp = batch
    assert n % 64 in (0, 64 - TAIL) and n // 256 >= 15
    for fmt in (96, 49):
        got = ctx.g1_mul(pts[:96 * n], sc[:32 * n], fmt)
        want = exp[fmt][:fmt * n]
        bad = [i for i in range(n) if got[fmt * i:fmt * i + fmt] != want[fmt * i:fmt * i + fmt]]
        assert bad == [] and len(got) == len(want), [(i, tags[i]) for i in bad[:8]]


@pytest.mark.parametrize("k", (2, 4))
def test_g1_mul_sum_every_lane_equals_the_oracle(ctx, oracle_port, k):
    edge, tags = edge_lanes(oracle_port, k)
    related = related_lanes(oracle_port, k, reps=2)[0]
    step = len(edge) // 600 + 1                              # every special point with a spread of edge scalars and term positions
    lanes = edge[::step] + related
    assert {t[0] for t in tags[::step]} == {t[0] for t in tags} and {0, 1} <= {t[1] for t in tags[::step]}
    lanes += seeded_lanes(oracle_port, k, NSUM - len(lanes), 9960 + k)
    assert len(lanes) == NSUM
    pts, sc = pack(lanes, k)
    for fmt in (96, 49):
        want = expected(oracle_port, pts, sc, k, fmt)
        got = ctx.g1_mul_sum(pts, sc, k, fmt)
        bad = [i for i in range(NSUM) if got[fmt * i:fmt * i + fmt] != want[fmt * i:fmt * i + fmt]]
        assert bad == [] and len(got) == len(want), bad[:8]
