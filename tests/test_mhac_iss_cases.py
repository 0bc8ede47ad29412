"""CPU test of the expected functions of the MHAC-bbs issuance entries (tests/mhac_iss_cases.py), so that the GPU tests cannot hide behind a wrong
oracle: on honest inputs they equal the builders of tests/mhac_bbs_cases.py (which restate the reference with its own grouping); their outputs fed to
cred_pres and expected_verify give 1 for the reference's own world (m = 4, Prv = (0, 2), Rev = (1), t = 3, 6 parties, S = (0, 2, 5)); any t shares of
e and of each private attribute reconstruct the constant term; and the throwing cases are where the reference throws."""
import itertools

import pytest

import mhac_bbs_cases as mh
import mhac_iss_cases as mi
from util import R, prng

M, PRV, REV, T, NP, S = mh.M_MAIN, mh.PRV_MAIN, mh.REV_MAIN, mh.T_MAIN, 6, (0, 2, 5)


@pytest.fixture(scope="module")
def op(oracle_port):
    return mh.Ops(oracle_port)


@pytest.fixture(scope="module")
def world(op):
    return mh.World(op, 6000, M)


def builder_rnd(seed, m, Prv, t):
    """the randomness generate_attributes / cred_iss of mhac_bbs_cases draw, as the entries take it"""
    attr = [prng(seed, i) % R for i in range(m)] + [prng(seed + 1, i) % R for i in range(len(Prv) * (t - 1))]
    iss = [prng(seed + 7, i) % R for i in range(t)]
    return mi.rnd_bytes(attr), mi.rnd_bytes(iss)


def chain(op, wd, Prv, Rev, t, nparties, S, seed):
    """attr -> iss -> group -> type by the expected functions; returns the four results"""
    Pub = mh.sets(wd.m, Prv, Rev)[0]
    ra, ri = builder_rnd(seed, wd.m, Prv, t)
    a = mi.expected_attr(op, wd.pp, wd.h49, Prv, t, nparties, ra)
    i = mi.expected_iss(op, wd.pp, wd.h49, mh.b48(wd.gamma), Pub, t, nparties, a[2], a[0], ri)
    g = mi.expected_group(op, S, nparties, len(Prv), i[2], i[1], a[1])
    ty = mi.expected_type(op, wd.pp, wd.h49, Prv, Rev, a[0])
    return a, i, g, ty


@pytest.mark.parametrize("m,Prv,Rev,t,nparties,S", [(M, PRV, REV, T, NP, S), (4, (2, 0), (), 2, 3, (2, 0)), (3, (), (0, 2), 1, 1, (0,)), (4, (0, 1, 2, 3), (), 5, 6, (5, 1, 0, 3, 2))])
def test_the_expected_functions_equal_the_builders(op, m, Prv, Rev, t, nparties, S):
    wd = mh.World(op, 6000 + m, m)
    seed = 8100
    Pub = mh.sets(m, Prv, Rev)[0]
    a, i, g, ty = chain(op, wd, Prv, Rev, t, nparties, S, seed)
    pub_a, share, C = mh.generate_attributes(op, wd, t, nparties, Prv, seed)
    assert a == (b"".join(map(mh.b48, pub_a)), b"".join(mh.b48(v) for row in share for v in row), b"".join(map(op.enc, C)))
    A, e_share, D = mh.cred_iss(op, wd, t, C, Pub, pub_a, seed + 7)
    assert i == (op.enc(A), b"".join(map(mh.b48, e_share)), b"".join(map(op.enc, D)), 0)
    lam, Dg = mh.make_pres_group(op, D, S)
    assert g == (b"".join(map(mh.b48, lam)), op.enc(Dg), b"".join(mh.b48(e_share[k]) for k in S), b"".join(mh.b48(v) for k in S for v in share[k]), 0)
    C_rev, C_pub = mh.make_pres_type(op, wd, Rev, Prv, pub_a)
    assert ty == (op.enc(C_rev), op.enc(C_pub), 0)


def test_the_chain_of_the_reference_world_verifies(op, world):
    a, i, g, ty = chain(op, world, PRV, REV, T, NP, S, 8200)
    nP = len(PRV)
    f = lambda b, count: [int.from_bytes(b[48 * k:48 * k + 48], "big") for k in range(count)]
    pub_a, lam, e_S = f(a[0], M - nP), f(g[0], T), f(g[2], T)
    a_S = [f(g[3][48 * nP * k:], nP) for k in range(T)]
    dec = lambda rec: op.dec(rec)[0]
    rnd = mh.draw(8250, mh.rnd_count(M, PRV, REV, T))
    fixed, z, zhp = mh.cred_pres(op, world, dec(i[0]), e_S, lam, dec(g[1]), dec(ty[0]), dec(ty[1]), PRV, REV, pub_a, a_S, rnd)
    rev48 = b"".join(mh.b48(pub_a[k]) for k in mh.sets(M, PRV, REV)[3])
    assert mh.expected_verify(op, world.pp, world.h49, world.pk, PRV, REV, ty[0], fixed, z, zhp, rev48) == 1
    # the e_share rows of another credential: the hash half still holds, the pairing half does not
    other = chain(op, world, PRV, REV, T, NP, S, 8300)[2][2]
    fixed, z, zhp = mh.cred_pres(op, world, dec(i[0]), f(other, T), lam, dec(g[1]), dec(ty[0]), dec(ty[1]), PRV, REV, pub_a, a_S, rnd)
    assert mh.expected_verify(op, world.pp, world.h49, world.pk, PRV, REV, ty[0], fixed, z, zhp, rev48) == 0


def test_any_t_shares_reconstruct_the_constant_term(op, world):
    ra, ri = builder_rnd(8400, M, PRV, T)
    a, i, _, _ = chain(op, world, PRV, REV, T, NP, S, 8400)
    attr, e = mi.rnd_values(ra)[:M], mi.rnd_values(ri)[0]
    es = [int.from_bytes(i[1][48 * k:48 * k + 48], "big") for k in range(NP)]
    sh = [[int.from_bytes(a[1][48 * (len(PRV) * k + ii):][:48], "big") for ii in range(len(PRV))] for k in range(NP)]
    for sub in itertools.permutations(range(NP), T):
        xs = [k + 1 for k in sub]
        lam = [mh.lagrange(xs, k) for k in range(T)]
        assert lam == [mi.lam_at(xs, k) for k in range(T)] and sum(lam) % R == 1
        assert sum(l * es[k] for l, k in zip(lam, sub)) % R == e
        for ii, idx in enumerate(PRV):
            assert sum(l * sh[k][ii] for l, k in zip(lam, sub)) % R == attr[idx]


def test_where_the_reference_throws(op, world):
    Pub = mh.sets(M, PRV, REV)[0]
    ra, ri = builder_rnd(8500, M, PRV, T)
    a, i, g, ty = chain(op, world, PRV, REV, T, NP, S, 8500)
    sk = mh.b48(world.gamma)
    bad_pp = b"\x05" + world.pp[1:]
    assert mi.expected_attr(op, bad_pp, world.h49, PRV, T, NP, ra) is None
    assert mi.expected_attr(op, world.pp, mh.off_curve_x() + world.h49[49:], PRV, T, NP, ra) is None
    assert mi.expected_attr(op, world.pp, world.h49[:49] + mh.off_curve_x() + world.h49[98:], PRV, T, NP, ra) == a          # h[1] is public: not read
    assert mi.expected_iss(op, world.pp, world.h49, mh.b48(R), Pub, T, NP, a[2], a[0], ri) is None
    assert mi.expected_iss(op, world.pp, mh.off_curve_x() + world.h49[49:], sk, Pub, T, NP, a[2], a[0], ri) == i            # h[0] is private: not read
    last = a[2][:49 * (NP - 1)] + mh.off_curve_x()
    assert mi.expected_iss(op, world.pp, world.h49, sk, Pub, T, NP, last, a[0], ri)[3] == 0xff                              # a record beyond the first t
    assert mi.expected_iss(op, world.pp, world.h49, sk, Pub, T, NP, a[2], mh.field(a[0], 1, R), ri)[3] == 0xff
    outside = i[2][:49] + mh.off_curve_x() + i[2][98:]
    assert mi.expected_group(op, S, NP, len(PRV), outside, i[1], a[1]) == g                                               # party 1 is not in S
    assert mi.expected_group(op, (0, 1, 5), NP, len(PRV), outside, i[1], a[1])[4] == 0xff
    assert mi.expected_type(op, world.pp, world.h49, PRV, REV, mh.field(a[0], 0, (1 << 384) - 1)) == (b"\xff" * 49, b"\xff" * 49, 0xff)
    assert mi.expected_type(op, bad_pp, world.h49, PRV, REV, a[0]) is None


def test_gamma_plus_e_zero_gives_infinity(op, world):
    Pub = mh.sets(M, PRV, REV)[0]
    ra, ri = builder_rnd(8600, M, PRV, T)
    a = mi.expected_attr(op, world.pp, world.h49, PRV, T, NP, ra)
    ri = mi.rnd_bytes([(R - world.gamma) % R]) + ri[32:]
    A, _, D, st = mi.expected_iss(op, world.pp, world.h49, mh.b48(world.gamma), Pub, T, NP, a[2], a[0], ri)
    assert st == 0 and A == bytes(49) and D == a[2]
