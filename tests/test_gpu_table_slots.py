"""The device-built tables that several entry points share (csrc/host.hpp cached_tables): the four G1 fixed-base slots (g1_mul_fixed, the
BBS+ message columns, bbs04's u, v, h, g1), the two line tables of BBS+ with their gate, and the line tables of the k-way product that bbs04
uses.  A table is rebuilt exactly when its point (or rule) changes, whoever asked for it last: calls of different owners are interleaved
here, routes are flipped inside one slot, and every result is the port oracle's.  n = 65 (one wavefront and one lane), nmsg = 5 (two
columns beyond the four table slots), bbs04 messages of 33 bytes."""
import pytest

import g2_twist
from g1_mul_sum_cases import subgroup_pool
from g1_torsion import ec_add, enc, generator, point_of_order
from test_gpu_bbs04 import Keys, Ops, expected_verify, sign
from util import R, golden, prng, scalars

pytestmark = pytest.mark.gpu

N, NMSG, MSG_LEN = 65, 5, 33
G1GEN = bytes.fromhex(golden("g1")["generator"])
G2GEN = bytes.fromhex(golden("g2")["generator"])
OFF_G1 = enc(ec_add(generator(), point_of_order(3)))        # order 3 r: on the curve, no table
OFF_G2 = g2_twist.enc192(g2_twist.point_of_order(13))       # on the twist, outside G2


@pytest.fixture(scope="module")
def ctx():
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


class Bbs:
    """N BBS+ signatures over NMSG messages, signed as examples/bbs-plus/src/bbs+.cpp:38-55 signs; `forged` = the same with a wrong message
    in every fourth lane.  args(m, w) are the arguments of bbs_plus_verify."""

    def __init__(self, orc, seed):
        gs = orc.g1_mul(G1GEN * (NMSG + 2), scalars(seed, NMSG + 2), 96)
        self.g1, self.h0, self.h = gs[:96], gs[96:192], gs[192:]
        self.g2 = orc.g2_mul(G2GEN, scalars(seed + 1, 1), 192)
        gamma = prng(seed + 2, 0) % R
        self.w = orc.g2_mul(self.g2, gamma.to_bytes(32, "big"), 192)
        A, cols = b"", [[] for _ in range(NMSG)]
        self.x, self.r = scalars(seed + 3, N), scalars(seed + 4, N)
        for j in range(N):
            msgs = [prng(seed + 5 + i, j) % R for i in range(NMSG)]
            sc = (1).to_bytes(32, "big") + self.r[32 * j:32 * j + 32] + b"".join(m.to_bytes(32, "big") for m in msgs)
            B = orc.g1_msm(self.g1 + self.h0 + self.h, sc, 96, 1)
            x = int.from_bytes(self.x[32 * j:32 * j + 32], "big")
            A += orc.g1_mul(B, pow((gamma + x) % R, -1, R).to_bytes(32, "big"), 96)
            for i in range(NMSG):
                cols[i].append(msgs[i])
        self.A = A
        self.m = b"".join(v.to_bytes(32, "big") for col in cols for v in col)
        for j in range(0, N, 4):
            cols[j % NMSG][j] = (cols[j % NMSG][j] + 1) % R
        self.forged = b"".join(v.to_bytes(32, "big") for col in cols for v in col)

    def args(self, m, w=None):
        return (self.g1, self.g2, self.h0, self.h, self.w if w is None else w, self.A, self.x, self.r, m)


class World:
    def __init__(self, orc):
        self.orc = orc
        self.op = Ops(orc)
        self.P = subgroup_pool(orc, 9101, 1)[0]
        self.sc = scalars(9102, N)
        self.want_P = orc.g1_mul(self.P * N, self.sc, 96, 8)
        self.want_off = orc.g1_mul(OFF_G1 * N, self.sc, 96, 8)
        self.bbs = Bbs(orc, 9110)
        assert self.bbs.h0 != self.P
        self.want_bbs = orc.bbs_plus_verify(*self.bbs.args(self.bbs.forged), 8)
        self.want_bbs_valid = orc.bbs_plus_verify(*self.bbs.args(self.bbs.m), 8)
        self.want_bbs_off = orc.bbs_plus_verify(*self.bbs.args(self.bbs.forged, OFF_G2), 8)
        assert self.want_bbs_valid == b"\x01" * N and self.want_bbs.count(0) == len(range(0, N, 4))
        self.keys = Keys(self.op, 9130)
        self.msgs = [prng(9131, i, MSG_LEN).to_bytes(MSG_LEN, "big") for i in range(N)]
        sigs = [sign(self.op, self.keys, i % 3, self.msgs[i], 9200 + i) for i in range(N)]
        for i in range(0, N, 5):                                                 # forged: another lane's T3
            sigs[i] = sigs[i][:98] + sigs[(i + 1) % N][98:147] + sigs[i][147:]
        self.sigs = b"".join(sigs)
        self.want_04 = bytes(expected_verify(self.op, self.keys.gpk, s, m) for s, m in zip(sigs, self.msgs))
        assert self.want_04.count(0) == len(range(0, N, 5)) and self.want_04.count(1) == N - len(range(0, N, 5))

    def mul_P(self, ctx):
        assert ctx.g1_mul_fixed(self.P, self.sc, 96) == self.want_P

    def bbs_verify(self, ctx):
        assert ctx.bbs_plus_verify(*self.bbs.args(self.bbs.forged)) == self.want_bbs

    def bbs04_verify(self, ctx):
        assert ctx.bbs04_verify(self.keys.gpk, self.sigs, b"".join(self.msgs), MSG_LEN) == self.want_04


@pytest.fixture(scope="module")
def world(oracle_port):
    return World(oracle_port)


def test_interleaved_owners_of_slot_0(ctx, world):
    """g1_mul_fixed's P, BBS+'s h0 and bbs04's u take turns in slot 0"""
    world.mul_P(ctx)
    world.bbs_verify(ctx)
    world.mul_P(ctx)
    world.bbs04_verify(ctx)
    world.mul_P(ctx)


def test_route_flips_in_one_slot(ctx, world):
    """a base off the subgroup (generic route), a subgroup base (table route), the first one again"""
    assert ctx.g1_mul_fixed(OFF_G1, world.sc, 96) == world.want_off
    world.mul_P(ctx)
    assert ctx.g1_mul_fixed(OFF_G1, world.sc, 96) == world.want_off
    world.mul_P(ctx)


def test_bbs_plus_gate_is_recomputed(ctx, world):
    """w outside G2 (generic route), a valid w (both line tables), the first w again; then the aggregate form on the same two tables"""
    b = world.bbs
    assert ctx.bbs_plus_verify(*b.args(b.forged, OFF_G2)) == world.want_bbs_off
    world.bbs_verify(ctx)
    assert ctx.bbs_plus_verify(*b.args(b.forged, OFF_G2)) == world.want_bbs_off
    assert ctx.bbs_plus_verify(*b.args(b.m)) == world.want_bbs_valid
    rho = scalars(9140, N, 1 << 128)
    assert ctx.bbs_plus_verify_aggregate(*b.args(b.m), rho) is True
    assert ctx.bbs_plus_verify_aggregate(*b.args(b.forged), rho) is False
    assert ctx.bbs_plus_verify_aggregate(*b.args(b.m, OFF_G2), rho) is False
    assert ctx.bbs_plus_verify_aggregate(*b.args(b.m), rho) is True


def test_bbs04_and_bbs_plus_alternate_on_their_line_tables(ctx, world):
    """bbs04's k = 2 product (rule 0) and BBS+'s w, g2 tables (rule 1) in turn under fixed keys: neither leaves the other a table built for
    another point or rule.  (Results alone cannot show whether a table was rebuilt in between: a rebuilt table gives the same booleans.)"""
    for _ in range(2):
        world.bbs04_verify(ctx)
        world.bbs_verify(ctx)


def test_after_trim(ctx, world):
    """the interleaved sequence with the workspaces handed back in the middle: every table is rebuilt by the call that needs it"""
    world.mul_P(ctx)
    world.bbs_verify(ctx)
    world.bbs04_verify(ctx)
    ctx.trim()
    world.mul_P(ctx)
    world.bbs04_verify(ctx)
    world.bbs_verify(ctx)
    world.mul_P(ctx)
