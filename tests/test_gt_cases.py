"""CPU checks of the references the GT tests use, against each other: the Fp12 tower on Python integers (gt_cases.py) and the plain-C oracle must
agree byte for byte wherever both define the operation, and the element classes must be able to see what they are there for — the reference's
FP12_pow is the true power exactly on the cyclotomic subgroup (and on zero and one), and NOT on a unitary element outside it, on -1 or on a
Miller value, so a power that took the windowed ladder for such an element returns other bytes than the oracle's.  The last test holds the
plain-C oracle against the compiled reference on these classes; it asserts nothing on a machine without the compiled reference (nothing
here uses its recorded answers)."""
import pytest

import gt_cases as gc
from util import P, R


@pytest.fixture(scope="module")
def el():
    return gc.elements()


def test_tower_laws_and_layout(el):
    x, y = gc.dec(el["dense"]), gc.dec(el["unitary"])
    assert gc.mul(x, gc.inv(x)) == gc.ONE and gc.mul(y, gc.inv(y)) == gc.ONE
    assert gc.conj(x) == gc.power(x, P ** 6)                                     # conj is the Frobenius map of order two
    assert gc.mul(gc.add(x, y), x) == gc.add(gc.mul(x, x), gc.mul(y, x))
    assert gc.power(x, 5) == gc.mul(gc.mul(gc.mul(x, x), gc.mul(x, x)), x) and gc.power(x, 0) == gc.ONE
    assert gc.dec(gc.enc(x)) == x and gc.enc(gc.ONE) == bytes(575) + b"\x01" and el["e11"] == el["one"]
    # w^3 = s, s^2 = 1 + i, i^2 = -1 in the byte layout: w = e7 (b.a.a), w^2 = e3 (c.a.a), s = e9 (a.b.a), i = e10 (a.a.b)
    w, s, i = gc.dec(el["e7"]), gc.dec(el["e9"]), gc.dec(el["e10"])
    assert gc.mul(w, w) == gc.dec(el["e3"]) and gc.mul(gc.mul(w, w), w) == s
    assert gc.mul(s, s) == gc.add(gc.ONE, i) and gc.mul(i, i) == gc.dec(el["minus_one"])
    # every label of every class exists once
    assert sorted(gc.all_labels() + ["gt2"]) == sorted(el)


def test_tower_against_oracle_mul_and_conj(oracle_port, el):
    pairs = gc.mul_pairs()
    assert len(pairs) >= 144 + 64 and len({p[0] for p in pairs[:144]}) == 144
    a, b = b"".join(p[1] for p in pairs), b"".join(p[2] for p in pairs)
    assert gc.differs(oracle_port.gt_op("mul", a, b), gc.mul_expected(pairs), 576, [p[0] for p in pairs]) == ""
    labels = gc.all_labels()
    assert gc.differs(oracle_port.gt_op("conj", b"".join(el[l] for l in labels)), gc.conj_expected(labels), 576, labels) == ""
    # decoding mod p: a non-canonical encoding and its canonical form are the same operand
    for l in gc.classes()["noncanonical"]:
        canon = gc.enc(gc.dec(el[l]))
        assert canon != el[l] and oracle_port.gt_op("mul", el[l], el["dense"]) == oracle_port.gt_op("mul", canon, el["dense"]), l


def test_tower_against_oracle_fexp(oracle_port, el):
    """PAIR_fexp(x) = x^(3 (p^12 - 1) / r) on one element of every class; zero, which has no inverse, gives the oracle's own bytes (zero)"""
    tower = gc.fexp_tower()
    labels = gc.all_labels()
    got = gc.split(oracle_port.fexp(b"".join(el[l] for l in labels)))
    bad = [l for l, g in zip(labels, got) if l in tower and g != tower[l]]
    assert bad == [], bad
    zeros = [l for l in labels if l not in tower]
    assert sorted(zeros) == ["zero", "zero_p"]
    assert all(got[labels.index(l)] == el["zero"] for l in zeros)
    # the values are in GT: of order dividing r, and 1 for the subfield elements (killed by the easy part)
    assert all(gc.power(gc.dec(tower[l]), R) == gc.ONE for l in ("dense", "b_only", "nc_plus_p"))
    assert tower["a_fp"] == el["one"] and tower["minus_one"] == el["one"] and tower["dense"] != el["one"]
    # x^(3 h), not x^h: the cube of the first power
    x = gc.dec(el["gt"])
    assert gc.fexp_true(x) == gc.power(gc.power(x, (P ** 12 - 1) // R), 3) != gc.power(x, (P ** 12 - 1) // R)


def test_pow_is_the_true_power_exactly_on_the_cyclotomic_subgroup(oracle_port, el):
    labels, a, e = gc.pow_cases()
    got = gc.split(oracle_port.gt_op("pow", a, e))
    agree = {}
    for (l, x), g in zip(labels, got):
        agree.setdefault(l, []).append(g == gc.true_power(l, x))
    for l in gc.WINDOWED:                                  # members, of order dividing r or not, their + p encodings, zero and one
        assert all(agree[l]), l
    for l in ("unitary", "minus_one", "miller"):           # the exponents 0 and 1 run no squaring; every other chosen exponent shows the route
        assert agree[l] == [x in (0, 1) for x in gc.POW_EXPS], (l, agree[l])
    assert set(gc.WINDOWED) | set(gc.GENERIC) == set(gc.POW_LABELS)


def test_near_one_list_has_both_verdicts():
    items = gc.near_one()
    want = gc.unity_expected(items)
    ones = [l for (l, _), v in zip(items, want) if v]
    assert ones == ["one", "one as (p + 1, p, ...)", "one as p + 1", "one as 2p + 1, p in c"]
    assert len(items) == len({b for _, b in items}) and want.count(0) >= 12 + 11


def test_lane_patterns():
    for at in gc.SPECIAL_AT:
        p = gc.pattern(["gt", "cyclotomic"], "unitary", at)
        assert len(p) == 63 and p[at] == "unitary" and p.count("unitary") == 1
    assert gc.SPECIAL_AT == (0, 20, 30, 62)                 # first and last triple of a wavefront (lane 63 shadows the last), mid-wavefront, last of the batch
    for n in gc.RAGGED:
        r = gc.ragged(["gt"], "unitary", n)
        assert len(r) == n and r[-1] == "unitary" and r.count("unitary") == 1
    assert [n % 21 for n in gc.RAGGED] == [1, 20, 0, 1, 1, 1]


def test_compiled_reference_agrees_where_present(oracle_port, el):
    """the plain-C oracle against the reference's own FP12_fromOctet / FP12_mul / FP12_pow / PAIR_fexp on these classes; empty (it passes
    without asserting anything) where the compiled reference is absent"""
    from oracle.bindings import Oracle, have_reference
    if not have_reference():
        return
    ref = Oracle("reference")
    labels, a, e = gc.pow_cases()
    assert gc.differs(ref.gt_op("pow", a, e), oracle_port.gt_op("pow", a, e), 576, labels) == ""
    pairs = gc.mul_pairs()
    a, b = b"".join(p[1] for p in pairs), b"".join(p[2] for p in pairs)
    assert gc.differs(ref.gt_op("mul", a, b), oracle_port.gt_op("mul", a, b), 576, [p[0] for p in pairs]) == ""
    fl = gc.all_labels()
    f = b"".join(el[l] for l in fl)
    assert gc.differs(ref.fexp(f), oracle_port.fexp(f), 576, fl) == ""
