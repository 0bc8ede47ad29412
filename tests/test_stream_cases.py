"""CPU test of tests/stream_cases.py: every _dev entry that include/c12381_hip.h and include/c12381_ac.h declare has a row (or is listed with the
reason why not), and the premises of tests/test_gpu_stream_contract.py that need no GPU hold for every row — A and B have equal shapes, every
input buffer of A differs from B's, the expected bytes of A differ from those of B, and a verdict row has both verdicts in A."""
import os
import re

import pytest

import stream_cases as sc
from stream_cases import In, Out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [r.id for r in sc.ROWS]


def _declared():
    names = set()
    for h in ("c12381_hip.h", "c12381_ac.h"):
        names |= set(re.findall(r"\bc12381_([a-z0-9_]+_dev)\s*\(", open(os.path.join(ROOT, "include", h)).read()))
    return names


def test_every_dev_entry_has_a_row_or_is_listed():
    declared = _declared()
    assert len(declared) > 50
    covered = {r.dev for r in sc.ROWS}
    assert covered <= declared, sorted(covered - declared)
    for name in sorted(declared):
        assert name in covered or name in sc.NO_CASE, name
    for name in sc.NO_CASE:
        assert name in declared and name not in covered, name


def test_enum_variants_and_the_two_stream_sort_are_rows(oracle_port):
    ops = {(r.dev, int(sc.case(oracle_port, r)[0][0])) for r in sc.ROWS if r.dev in ("zp_op_batch_dev", "gt_op_batch_dev")}
    assert ops == {("zp_op_batch_dev", 0), ("zp_op_batch_dev", 4)} | {("gt_op_batch_dev", op) for op in range(4)}
    for id in ("gt_op[mul]", "gt_op[conj]", "gt_op[pow]", "gt_op[fexp]", "ps_sign[encode]", "ps_sign[hash]", "ps_verify_wire[encode]",
               "ps_verify_wire[hash]", "g1_msm", "g1_msm[2^15]"):
        assert id in sc.BY_ID, id
    assert sc.BY_ID["g1_msm[2^15]"].n == 1 << 15 and sc.BY_ID["g1_msm"].n == sc.N


@pytest.mark.parametrize("id", IDS)
def test_premises(oracle_port, id):
    row = sc.BY_ID[id]
    a, want_a, st_a = sc.case(oracle_port, row, v=0)
    b, want_b, st_b = sc.case(oracle_port, row, v=1)
    assert st_a == 0 and st_b == 0
    # equal shapes: the same kinds, counts, modes and buffer sizes, argument by argument
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert type(x) is type(y), id
        if isinstance(x, In):
            assert len(x) == len(y) and len(x) > 0 and bytes(x) != bytes(y), id
        else:
            assert x == y, id
    outs = [int(x) for x in a if isinstance(x, Out)]
    assert [len(w) for w in want_a] == outs and [len(w) for w in want_b] == outs, id
    assert want_a != want_b, id
    assert all(isinstance(a[i], In) for i in row.unread), id
    if row.verdict:
        verdicts = [w for w, size in zip(want_a, outs) if size == row.n]
        assert len(verdicts) == 1 and set(verdicts[0]) == {0, 1}, (id, verdicts)
    assert row.source in ("integers", "oracle", "builders")
