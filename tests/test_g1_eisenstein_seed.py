"""CPU tests, plain Python, of the facts on which g1_scalar_mul_eis (g1.hpp) seeds its accumulator from the top two digits and runs 42
windows: the range of t = 8 d_43 + d_42, the fourteen values that are nothing or one digit, the two that are a table element plus one,
the only (digit 43, digit 42) pairs, and a predictor of the seeded schedule that agrees with g1_eisenstein.exceptional on every point the
suite multiplies."""
import pytest

from g1_eisenstein import CLASSES, DIGITS, REPS, edge_scalars, exceptional, mul_unit, norm, recode, split, value
from g1_eisenstein_seed import LOW, SUMS, corner_scalars, exact_digit, exceptional_seeded, one_scalar_per_top_value, seed_scalars, top_value
from g1_torsion import X2, crt, eigenvalues
from util import R, prng

ALL_T = [(a, b) for a in range(4) for b in range(4)]


@pytest.fixture(scope="module")
def expansions():
    return [(k, recode(*split(k))) for k in seed_scalars()]


def test_corner_of_the_split():
    assert R == X2 * X2 - X2 + 1 and R // X2 == X2 - 1
    assert split(R - 1) == (0, X2 - 1) and split(R - 2) == (X2 - 1, X2 - 2)
    # both bounds of the coefficients are 2.6917... 8^42, and a coefficient c becomes at most (c + 5) / 8 per digit: c_42 < 2.6918 + 5 / 7 < 4
    assert 26917 * 8 ** 42 < 10000 * (X2 - 1) < 26918 * 8 ** 42
    assert all(-5 <= c <= 5 for _, _, d in CLASSES for c in d)


def test_range_of_the_top_value(expansions):
    seen = set()
    for k, digs in expansions:
        assert len(digs) <= DIGITS
        t = value(digs[LOW:])
        assert t in ALL_T, (hex(k), t)
        seen.add(t)
        k0, k1 = split(k)
        lo = value(digs[:LOW])
        assert (k0 - lo[0], k1 - lo[1]) == (t[0] * 8 ** LOW, t[1] * 8 ** LOW)
    assert sorted(seen) == ALL_T                               # (3, 3) needs the corner
    assert sorted(one_scalar_per_top_value()) == ALL_T
    assert {top_value(k) for k in corner_scalars()} >= {(3, 3), (3, 2)}


def test_fourteen_values_are_nothing_or_one_digit(expansions):
    for t in ALL_T:
        if t in SUMS or t == (0, 0):
            assert exact_digit(t) is None
        else:
            assert exact_digit(t) is not None, t                # (2, 3), of norm 19 like (3, 2), is the digit of its class; (3, 2) is not
    assert sorted(norm(t) for t in SUMS) == [19, 27]
    assert max(norm(t) for t in ALL_T if t not in SUMS) == 19
    for k, digs in expansions:
        t = value(digs[LOW:])
        if t in SUMS:
            continue
        assert len(digs) <= LOW + 1, hex(k)
        if t == (0, 0):
            assert len(digs) <= LOW
        else:
            e, u, d = digs[LOW]
            assert d == t == mul_unit(REPS[e], u) and (e, u) == exact_digit(t)


def test_two_values_are_a_table_element_plus_one():
    assert sorted(SUMS) == [(3, 2), (3, 3)]
    for t, (s, top, low) in SUMS.items():
        assert (s[0] + 1, s[1]) == t
        assert (8 * top[0] + low[0], 8 * top[1] + low[1]) == t
        assert exact_digit(s) is not None and exact_digit(low) is not None
        e, u = exact_digit(s)
        assert mul_unit(REPS[e], u) == s
    assert exact_digit((2, 2)) == (7, 2) and exact_digit((2, 3)) == (8, 2)
    assert exact_digit((1, 0)) == (0, 0) and exact_digit((0, 1)) == (0, 1)


def test_pairs_of_the_top_two_digits(expansions):
    seen = set()
    for k, digs in expansions:
        if len(digs) < DIGITS:
            continue
        t = value(digs[LOW:])
        assert t in SUMS, (hex(k), t)
        pair = (digs[LOW + 1][2], digs[LOW][2])
        assert pair == SUMS[t][1:], (hex(k), pair)
        seen.add(pair)
    assert seen == {((1, 0), (-5, 2)), ((0, 1), (3, -5))}
    # and conversely: t in SUMS always fills position 43
    assert all(len(digs) == DIGITS for _, digs in expansions if value(digs[LOW:]) in SUMS)


def test_predictor_of_the_seeded_schedule_agrees_on_every_point_of_the_suite(expansions):
    """subgroup points, the points of order 3, a point of order 11 (inert), the eigenpoint of order 10177 and G + T_3 of order 3 r: the
    seed's addition fails only where [(1, 2)]P, [(3, 2)]P, [(1, 3)]P or [(3, 3)]P vanishes (norms 7, 19, 13, 27), the step it replaces
    where 8 d_43 = +-d_42; neither happens on these points beyond what the table already rejects"""
    ks = [k for k, _ in expansions][:len(edge_scalars()) + 3000] + corner_scalars()
    ks += [prng(44005, i) % (1 << 256) for i in range(1500)]   # the scalars of the torsion lanes of tests/test_host_sim_g1_eisenstein.py
    points = [(R, X2 % R), (3, 2), (11, None), (10177, eigenvalues(10177)[0]), (10177, eigenvalues(10177)[1]), (3 * R, crt(X2, R, -1, 3))]
    for q, lam in points:
        got = [exceptional_seeded(k, q, lam) for k in ks]
        want = [exceptional(k, q, lam) for k in ks]
        assert got == want, (q, [hex(k) for k, g, w in zip(ks, got, want) if g != w][:4])
    assert any(len(recode(*split(k))) == DIGITS for k in ks)
