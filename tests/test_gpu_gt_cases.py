"""GPU parity of the GT entries (Context.gt_op mul / conj / pow, fexp, gt_is_unity and their _dev forms) on ARBITRARY elements of Fp12
(gt_cases.py; run with -m gpu): byte equality with the Fp12 tower on Python integers and, for FP12_pow, with the plain-C oracle — the two
are held against each other by test_gt_cases.py, and the same lists run through the host simulation under the bounds checker in
test_host_sim_gt_cases.py.  What the rest of the suite cannot see: one coefficient route of the three-lane product at a time, operands with
zero coefficients, non-canonical encodings through gt_load_coeff, single-coordinate misses of one, and the power's WAVE-WIDE route choice —
one unitary element outside the cyclotomic subgroup (or -1, or a Miller value) sends its whole wavefront of 21 through the reference's digit
sequence, at the first and last triple of a wavefront, mid-wavefront, alone in a ragged last group, in whole and in queued groups of the
work-queue kernel — where a membership test degraded to "unitary" would return other bytes for that element."""
import os
import subprocess
import sys

import pytest

import gt_cases as gc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLERS = ("gt", "cyclotomic", "gt2")                   # members of the cyclotomic subgroup: pairing values and one of order not dividing r


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()             # torch brings its own HIP runtime: let it load first when both live in one process
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def el():
    return gc.elements()


def _cat(el, labels):
    return b"".join(el[l] for l in labels)


def _exps(n, seed=7150):
    return gc.pattern_exps(seed, n)


def _eb(exps):
    return b"".join(int(x).to_bytes(32, "big") for x in exps)


@pytest.fixture(scope="module")
def lists(oracle_port):
    """the mul, is_unity, fexp and pow lists of the host-simulation tests with their expected bytes, computed once (gt_cases.entry_lists)"""
    return gc.entry_lists(oracle_port)


@pytest.mark.parametrize("name", ("mul", "is_unity", "fexp", "pow"))
def test_gt_lists_of_the_host_simulation(ctx, lists, name):
    """mul: the 144 basis products, sparse x sparse, x . 0 / 1 / -1, non-canonical operands; is_unity: the near-one list; fexp: every class;
    pow: every group-theoretic class, -1, zero, one and the + p forms with the edge exponents, then sparse and subfield bases"""
    assert gc.run_entry_lists(ctx, {name: lists[name]}) == []


def test_gt_conj_on_every_class(ctx, el):
    labels = gc.all_labels()
    assert gc.differs(ctx.gt_op("conj", _cat(el, labels)), gc.conj_expected(labels), 576, labels) == ""


@pytest.fixture(scope="module")
def members(ctx, el, oracle_port):
    """the all-member pattern of 63 elements: its exponents, what the GPU gives for it, the oracle's bytes and the tower's true powers"""
    labels = gc.pattern(FILLERS, FILLERS[0], 0)
    exps = _exps(63)
    a, e = _cat(el, labels), _eb(exps)
    want = oracle_port.gt_op("pow", a, e)
    true = b"".join(gc.true_power(l, x) for l, x in zip(labels, exps))
    assert want == true                                   # on members FP12_pow is the power
    got = ctx.gt_op("pow", a, e)
    assert gc.differs(got, want, 576, list(zip(labels, exps))) == ""
    return labels, exps, gc.split(got)


@pytest.mark.parametrize("special", ("unitary", "minus_one", "miller", "gt_p"))
def test_gt_pow_route_is_chosen_per_wavefront(ctx, el, oracle_port, members, special):
    """one special element among members, at the first and the last triple of the first wavefront, inside the second and at the end of the
    batch: unitary, minus_one and miller force the generic ladder on their 21, the + p encoded pairing value does not.  Every element against
    the oracle; the other 62 also against what the all-member pattern gave (= the tower's true powers, fixture `members`)"""
    base_labels, exps, base = members
    e = _eb(exps)
    for at in gc.SPECIAL_AT:
        labels = gc.pattern(FILLERS, special, at)
        assert [l for i, l in enumerate(labels) if i != at] == [l for i, l in enumerate(base_labels) if i != at]
        a = _cat(el, labels)
        got = ctx.gt_op("pow", a, e)
        assert gc.differs(got, oracle_port.gt_op("pow", a, e), 576, list(zip(labels, exps))) == "", at
        got = gc.split(got)
        assert [i for i in range(63) if i != at and got[i] != base[i]] == [], at
        if special == "gt_p":
            assert got[at] == gc.true_power("gt", exps[at]), at
        else:
            assert exps[at] > 1 and got[at] != gc.true_power(special, exps[at]), at      # the reference's value is not the power there: the route shows


@pytest.mark.parametrize("n", gc.RAGGED)
def test_gt_ragged_sizes_with_a_unitary_last_element(ctx, el, oracle_port, n):
    """n = 1, 20, 21, 22, 43, 64: the unitary element outside the subgroup alone in the batch, last of a full wavefront, alone in a ragged
    last group; mul, pow, fexp and is_unity"""
    labels = gc.ragged(FILLERS[:2], "unitary", n)
    a = _cat(el, labels)
    b = _cat(el, labels[::-1])
    assert gc.differs(ctx.gt_op("mul", a, b), b"".join(gc.enc(gc.mul(gc.dec(el[x]), gc.dec(el[y]))) for x, y in zip(labels, labels[::-1])), 576, labels) == ""
    e = _eb(_exps(n, 7151)[::-1])                          # the unitary element gets a random exponent at every n
    assert gc.differs(ctx.gt_op("pow", a, e), oracle_port.gt_op("pow", a, e), 576, labels) == ""
    tower = gc.fexp_tower()
    assert gc.differs(ctx.fexp(a), b"".join(tower[l] for l in labels), 576, labels) == ""
    ul = gc.ragged(("one", "gt", "one_p"), "unitary", n)
    assert ctx.gt_is_unity(_cat(el, ul)) == bytes(1 if gc.dec(el[l]) == gc.ONE else 0 for l in ul)


def _mixed(el):
    """three wavefronts: a unitary element in the first, members only in the second, -1 in the third"""
    labels = gc.pattern(FILLERS, "unitary", 5)
    labels[42 + 4] = "minus_one"
    exps = _exps(63, 7152)
    return labels, _cat(el, labels), _eb(exps)


def test_gt_dev_forms_equal_the_host_forms(ctx, el):
    import torch
    dev = torch.device("cuda", 0)
    labels, a, e = _mixed(el)
    n = len(labels)
    b = _cat(el, labels[::-1])
    da, db, de = (torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev) for x in (a, b, e))
    out = torch.zeros(576 * n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    for op, second, host in (("mul", db, b), ("conj", None, None), ("pow", de, e), ("fexp", None, None)):
        out.fill_(0xa5)
        torch.cuda.synchronize(dev)
        ctx.gt_op_dev(op, n, da.data_ptr(), second.data_ptr() if second is not None else None, out.data_ptr())
        assert ctx.sync() == 0
        assert gc.differs(bytes(out.cpu().numpy()), ctx.gt_op(op, a, host), 576, labels) == "", op
    ul = gc.pattern(("one", "gt", "one_p"), "unitary", 20)
    ua = _cat(el, ul)
    du = torch.frombuffer(bytearray(ua), dtype=torch.uint8).to(dev)
    ok = torch.full((n,), 0xa5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ctx.gt_is_unity_dev(n, du.data_ptr(), ok.data_ptr())
    assert ctx.sync() == 0
    assert bytes(ok.cpu().numpy()) == ctx.gt_is_unity(ua) == bytes(1 if gc.dec(el[l]) == gc.ONE else 0 for l in ul)


def test_gt_pow_queue_with_unitary_elements_outside_the_subgroup(ctx, el, oracle_port):
    """the mixed pattern tiled to 4096 * 21 + 100 elements (gt3_pow_queue_kernel, as test_gpu_pairing.py::test_gt_power_routes sizes it): a
    unitary element outside the subgroup and -1 in the groups taken whole and in the queued groups, whose route travels through the state word"""
    labels, a, e = _mixed(el)
    want = oracle_port.gt_op("pow", a, e)
    big = 4096 * 21 + 100
    reps = big // 63 + 1
    got = ctx.gt_op("pow", (a * reps)[:576 * big], (e * reps)[:32 * big])
    exp = (want * reps)[:576 * big]
    if got != exp:
        bad = [i for i in range(big) if got[576 * i:576 * i + 576] != exp[576 * i:576 * i + 576]]
        raise AssertionError("%d elements differ, first %s" % (len(bad), [(i, labels[i % 63]) for i in bad[:8]]))


CHILD = r"""
import sys
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')
import tools.libsel  # C12381_LIB -> capi.use_library
import gt_cases as gc
from oracle.bindings import Oracle
from crypto12381_amd import Context
lists = gc.entry_lists(Oracle('port'))
c = Context(0)
bad = gc.run_entry_lists(c, lists)
c.close()
assert not bad, bad
print('one-lane ok', sorted(lists))
"""


def test_gt_lists_through_the_one_lane_kernels():
    """the experiments library with C12381_PAIR_LANES=1 (gt_op_kernel / gt_is_unity_kernel of k_g2gt.hip on fp12.hpp) in a child process,
    the switch being read once per process: the same lists with the same expected bytes, which the child works out again from gt_cases"""
    from test_gpu_variants import exp_env
    r = subprocess.run([sys.executable, "-c", CHILD], env=exp_env({"C12381_PAIR_LANES": "1"}), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "one-lane ok ['fexp', 'is_unity', 'mul', 'pow']" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
