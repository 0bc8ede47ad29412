"""CPU test of the AC-rbbs builders (tests/ac_rbbs_cases.py) against themselves, so that the GPU tests cannot hide behind a wrong oracle: the honest
chain issue -> redact -> pres -> verify gives 1 on every shape of the GPU tests, every tampered field gives 0, each of the three equations fails
alone where a lane says so, every malformed lane is where the reference would throw, verify parses only the key records it uses while redact
parses all of pk.Y, and the oracle's multiply does NOT send a point off the subgroup to infinity under the scalar 0 (no zero-padded sums)."""
import pytest

import ac_rbbs_cases as rc
from g1_torsion import enc as enc96, point_of_order
from util import R


@pytest.fixture(scope="module")
def op(oracle_port):
    return rc.Ops(oracle_port)


@pytest.fixture(scope="module")
def main(op):
    key = rc.Key(op, 5000, rc.NATTR)
    lanes = rc.main_lanes(op, key)
    return key, lanes, rc.expect(op, key, rc.I_MAIN, lanes)


def test_main_lanes(main):
    key, lanes, want = main
    by = {}
    for ln, w in zip(lanes, want):
        by.setdefault(ln.kind, set()).add(w)
    assert set(by) == set(rc.ONE_KINDS + rc.ZERO_KINDS + rc.BAD_KINDS + ("A at infinity",))
    for kind in rc.ONE_KINDS:
        assert by[kind] == {1}, kind
    for kind in rc.ZERO_KINDS:
        assert by[kind] == {0}, kind
    for kind in rc.BAD_KINDS:
        assert by[kind] == {0xff}, kind
    assert by["A at infinity"] == {0}


def test_equations_fail_separately(op, main):
    key, lanes, _ = main
    by = {ln.kind: ln for ln in lanes}
    eq = lambda kind: rc.equations(op, key, rc.I_MAIN, by[kind].pres, by[kind].attr, by[kind].msg)
    assert eq("valid") == (True, True, True)
    assert eq("eq1 only fails") == (False, True, True)
    assert eq("s+1") == (True, False, True)
    assert eq("eq3 only fails") == (True, True, False)


@pytest.mark.parametrize("nattr,I", rc.SHAPES + rc.VERIFY_ONLY_SHAPES + [rc.SUM_SHAPE])
def test_honest_chain_on_every_shape(op, nattr, I):
    key = rc.Key(op, 5200 + nattr, nattr)
    lanes = rc.valid_lanes(op, key, I, 2, 5300)
    assert rc.expect(op, key, I, lanes) == b"\x01\x01"
    other = rc.Key(op, 5250 + nattr, nattr)
    assert rc.expect(op, other, I, lanes) == b"\x00\x00"


def test_kept_is_the_set_of_sums():
    """K_D = { nattr - i + j : i in I, j in J }"""
    for nattr, I in rc.SHAPES + rc.VERIFY_ONLY_SHAPES:
        J = rc.hidden(nattr, I)
        assert [k for k, _ in rc.kept(nattr, I)] == sorted({nattr - i + j for i in I for j in J})
        assert all(sorted(valid) == sorted(i for i in I if (k - nattr + i) in J) and k != nattr for k, valid in rc.kept(nattr, I))


def test_multiply_by_zero_is_not_infinity_off_the_subgroup(op):
    """why redact sums exactly K_D and pads no range with zero scalars: the reference's multiply sends a point of G1 to infinity under the scalar
    0, but not the point of order 3 — a term Y[k]^0 the reference never forms would change D for a key outside G1"""
    t3 = enc96(point_of_order(3))
    for p in (rc.G1GEN, bytes(96)):
        assert op.mul(p, 0) == bytes(96)
    assert op.mul(t3, 0) != bytes(96)


def test_verify_is_lazy_and_redact_is_not(op, main):
    key, lanes, _ = main
    ln = lanes[0]
    bad49, bad97 = rc.off_curve_x(), b"\x04" + key.tY97[1:97]
    verify = lambda Y, tY: rc.expected_verify(op, key.pk, Y, tY, rc.NATTR, rc.I_MAIN, ln.pres, ln.attr, ln.msg)
    put = lambda b, k, rec: b[:len(rec) * k] + rec + b[len(rec) * (k + 1):]
    for k in (1, 2, 4, 5, 6, 7):                                         # Y records verify never reads
        assert verify(put(key.Y49, k, bad49), key.tY97) == 1
    for k in (0, 3):
        assert verify(put(key.Y49, k, bad49), key.tY97) is None
    for k in (1, 2):                                                     # tilde_Y[n-1-i], i in (0, 3): records 3 and 0 are used
        assert verify(key.Y49, put(key.tY97, k, bad97)) == 1
    for k in (0, 3):
        assert verify(key.Y49, put(key.tY97, k, bad97)) is None
    cr = rc.Cred(op, key, rc.I_MAIN, 5100, 0)
    assert rc.expected_redact(op, key.pk, key.Y49, rc.NATTR, rc.I_MAIN, cr.attr_all, cr.sig) == (cr.cache, 0)
    for k in range(8):
        assert rc.expected_redact(op, key.pk, put(key.Y49, k, bad49), rc.NATTR, rc.I_MAIN, cr.attr_all, cr.sig) is None


def test_expected_pres_and_redact_refusals(op):
    key = rc.Key(op, 5000, rc.NATTR)
    cr = rc.Cred(op, key, rc.I_MAIN, 5400, 0)
    rnd = b"".join(v.to_bytes(32, "big") for v in (R, (1 << 256) - 1, R + 7))              # reduced mod r first
    p, st = rc.expected_pres(op, cr.sig, cr.cache, cr.msg, rnd)
    assert st == 0 and len(p) == 341
    assert p == rc.pres(op, cr.msg, cr.sig, cr.cache, [0, ((1 << 256) - 1) % R, 7])
    assert rc.expected_verify(op, key.pk, key.Y49, key.tY97, rc.NATTR, rc.I_MAIN, p, cr.attr, cr.msg) == 1
    for sig, cache in ((cr.sig[:49] + rc.b48(R), cr.cache), (b"\x05" + cr.sig[1:], cr.cache), (cr.sig, cr.cache[:98] + rc.off_curve_x() + cr.cache[147:])):
        assert rc.expected_pres(op, sig, cache, cr.msg, rnd) == (b"\xff" * 341, 0xff)
    for attr, sig in ((cr.attr_all[:48] + rc.b48(R) + cr.attr_all[96:], cr.sig), (cr.attr_all, cr.sig[:49] + rc.b48(R)), (cr.attr_all, b"\x05" + cr.sig[1:])):
        assert rc.expected_redact(op, key.pk, key.Y49, rc.NATTR, rc.I_MAIN, attr, sig) == (b"\xff" * 196, 0xff)
