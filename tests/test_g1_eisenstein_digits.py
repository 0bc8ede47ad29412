"""CPU tests of the base-8 Eisenstein digit set (tests/g1_eisenstein.py, the Python reference of g1.hpp's recoder): the classes mod 8 and
their orbits under the six units, the unit-step order of the table's chain, exactness of the expansion and the bound on its length."""
import random

from g1_eisenstein import CHAIN_UNITS, CLASSES, DIGITS, NONE, REPS, UNITS, digit_bound, mul_unit, norm, packed, recode, value
from g1_torsion import X2


def test_classes_and_orbits():
    """64 classes; the 63 non-zero ones fall into 10 unit-orbits of six and one of three (the class of 4); every class is unit x entry, with
    a representative of minimal norm in its class and coefficients in [-5, 5]"""
    assert len(CLASSES) == 64 and all(c is not None for c in CLASSES)
    assert CLASSES[0][0] == NONE
    orbits = {}
    for c in range(1, 64):
        e, u, d = CLASSES[c]
        assert 0 <= e < 11 and 0 <= u < 6 and d == mul_unit(REPS[e], u)
        assert ((d[0] & 7) + 8 * (d[1] & 7)) == c
        assert abs(d[0]) <= 5 and abs(d[1]) <= 5
        least = min(norm((a, b)) for a in range(-13, 14) for b in range(-13, 14) if (a - d[0]) % 8 == 0 and (b - d[1]) % 8 == 0)
        assert norm(d) == least, (c, d, least)
        orbits.setdefault(e, set()).add(c)
    sizes = sorted(len(v) for v in orbits.values())
    assert len(orbits) == 11 and sizes == [3] + [6] * 10
    assert len(orbits[REPS.index((4, -4))]) == 3
    # the orbit of a class is the set of its unit multiples
    for e, cls in orbits.items():
        assert cls == {(mul_unit(REPS[e], u)[0] & 7) + 8 * (mul_unit(REPS[e], u)[1] & 7) for u in range(6)}


def test_chain_uses_unit_steps_only():
    assert REPS[0] == (1, 0) and len(REPS) == 11 and len(set(REPS)) == 11
    assert len(CHAIN_UNITS) == 10
    for i, u in enumerate(CHAIN_UNITS):
        assert (REPS[i][0] + UNITS[u][0], REPS[i][1] + UNITS[u][1]) == REPS[i + 1]
    assert CHAIN_UNITS[-1] == 0                                # the running addend ends as P itself: entry 0 on the table's Z
    assert [mul_unit((1, 0), u) for u in range(6)] == UNITS


def _check(a, b):
    digs = recode(a, b, limit=64)
    assert value(digs) == (a, b)
    assert len(digs) <= DIGITS, (a, b, len(digs))
    return len(digs)


def test_small_pairs_exhaustively():
    """all |a|, |b| <= 64: the expansion is exact and ends (negative coefficients too, which the product path never sees)"""
    for a in range(-64, 65):
        for b in range(-64, 65):
            assert _check(a, b) <= 4


def test_extreme_and_patterned_pairs():
    top0, top1 = X2 - 1, (1 << 128) - 1
    pairs = [(top0 + i, top1 + j) for i in (-2, -1, 0) for j in (-2, -1, 0)]
    pairs += [(top0, 0), (0, top1), (top1, top1), (1 << 127, 1 << 127), (X2, X2)]
    words = [0xffffffff, 0xaaaaaaaa, 0x55555555, 0x00000000, 0x92492492, 0x6db6db6d, 0x24924924]
    pats = [sum(w << (32 * i) for i in range(4)) for w in words] + [0xaaaaaaaa55555555aaaaaaaa55555555, 0xffffffff00000000ffffffff00000000]
    pairs += [(a, b) for a in pats for b in pats]
    assert max(_check(a, b) for a, b in pairs) == DIGITS       # the bound is reached: the constant cannot be lowered
    for a, b in pairs[:9]:
        w = packed(a, b)
        assert len(w) == 10 and w[9] < (1 << (7 * DIGITS - 288))


def test_random_pairs_and_the_bound():
    assert digit_bound() == DIGITS
    rng = random.Random(44001)
    hist = {}
    for _ in range(100000):
        n = _check(rng.randrange(X2), rng.randrange(1 << 128))
        hist[n] = hist.get(n, 0) + 1
    print("digit count histogram:", sorted(hist.items()))
    assert max(hist) <= DIGITS
