"""CPU tests of the K-way table-driven Miller loop (pairing3.hpp miller3_rangek_fixed) under the bounds checker (tests/host_sim/fixed_k.cpp,
C12381_CHECK_BOUNDS).  For K = 1 .. 8 tables, run in the work queue's task ranges (64 .. 1 in MILLER_ITERS_PER_TASK = 16 steps):
- with raw tables the value is the product of the oracle's Miller values (the reference's pair_ate), G1 and G2 points at infinity included;
- with normalised tables (the GT entry points' default) it is the product of the K single-table loops as field elements."""
import ctypes
import os
import subprocess

import pytest

from util import cat, golden

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t
STEP = 16                                    # k_pair3.hip / k_pairk.hip: MILLER_ITERS_PER_TASK


@pytest.fixture(scope="module")
def fk():
    so = os.path.join(SIM_DIR, "libsim_fixedk.so")
    src = os.path.join(SIM_DIR, "fixed_k.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-pthread", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def run(fk, g1s, g2s, k, raw, step=STEP, single=0):
    n = len(g1s) // (96 * k)
    out = ctypes.create_string_buffer(576 * n)
    assert fk.sim_fixedk_miller(sz(n), k, g1s, g2s, raw, step, single, out) == 0
    return out.raw


@pytest.fixture(scope="module")
def inputs():
    """8 G2 points (row 7 of the golden pairing set is infinity) and, per column, 3 G1 points; column c has infinity in lane c % 3"""
    g = golden("pairing")
    g1, g2 = cat(g["g1"]), cat(g["g2"])
    n1 = len(g1) // 96
    q = [g2[192 * j:192 * j + 192] for j in range(8)]
    assert q[7] == bytes(192)
    n = 3
    cols = []
    for c in range(8):
        lanes = [g1[96 * ((c * n + i) % n1):96 * ((c * n + i) % n1) + 96] for i in range(n)]
        lanes[c % n] = bytes(96)
        cols.append(b"".join(lanes))
    return cols, q, n


def _prod(oracle, vals):
    acc = vals[0]
    for v in vals[1:]:
        acc = oracle.gt_op("mul", acc, v)
    return acc


@pytest.mark.parametrize("k", range(1, 9))
def test_rangek_raw_equals_oracle_miller_product(fk, oracle_port, inputs, k):
    cols, q, n = inputs
    order = list(range(8))[::-1] if k == 8 else list(range(k))        # k = 8: the G2 infinity column first
    g1s = b"".join(cols[c] for c in order)
    g2s = b"".join(q[c] for c in order)
    got = run(fk, g1s, g2s, k, raw=1)
    want = _prod(oracle_port, [oracle_port.miller_t(cols[c], q[c] * n) for c in order])
    assert got == want


@pytest.mark.parametrize("k", range(1, 9))
def test_rangek_normalised_equals_single_table_product(fk, oracle_port, inputs, k):
    cols, q, n = inputs
    g1s, g2s = b"".join(cols[:k]), b"".join(q[:k])
    got = run(fk, g1s, g2s, k, raw=0)
    singles = [run(fk, g1s, g2s, k, raw=0, single=c + 1) for c in range(k)]
    assert got == _prod(oracle_port, singles)
    # after the final exponentiation: the GT product of the pairings
    assert oracle_port.fexp_t(got) == _prod(oracle_port, [oracle_port.pair(cols[c], q[c] * n) for c in range(k)])


def test_rangek_task_split_does_not_matter(fk, inputs):
    cols, q, n = inputs
    g1s, g2s = b"".join(cols[:3]), b"".join(q[:3])
    ref = run(fk, g1s, g2s, 3, raw=1, step=64)
    for step in (1, 7, 16, 32):
        assert run(fk, g1s, g2s, 3, raw=1, step=step) == ref
