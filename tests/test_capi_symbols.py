"""CPU test: the C-ABI library builds, loads and exports every symbol include/c12381_hip.h declares
(no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from crypto12381_amd.build import build
    lib_path = build()
    lib = ctypes.CDLL(lib_path)
    names = set()
    for fn in os.listdir(os.path.join(ROOT, "include")):
        if fn.endswith(".h"):
            text = open(os.path.join(ROOT, "include", fn)).read()
            names |= set(re.findall(r"\b(c12381_[a-z0-9_]+)\s*\(", text))
    assert len(names) >= 10
    for n in sorted(names):
        assert hasattr(lib, n), f"symbol {n} declared in include/ but not exported"
    assert lib.c12381_version() >= 1


def test_create_fails_loudly_without_gpu():
    """No CPU fallback: on a box without a HIP device the context constructor raises."""
    import torch
    from crypto12381_amd import C12381Error, Context
    if torch.cuda.is_available():
        return
    try:
        Context(0)
    except C12381Error:
        return
    raise AssertionError("Context() succeeded without a GPU")


def test_profile_metadata_the_bench_line_reads():
    """profiles/traffic.json and profiles/issue.json carry, for every dominant kernel the bench line names, what bench.py computes its
    `traffic` and `roofline.issue` fields from (counter passes of tools/pmc_r03.sh, clock probe) — and bench.py names no kernel they lack."""
    import json
    t = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
    i = json.load(open(os.path.join(ROOT, "profiles", "issue.json")))
    assert t["units_per_launch"] > 0 and t["g1_mul_kernel_hbm_bytes_per_launch"] > 0
    for key in ("pair_kernel", "pair3_prod_fixed_queue_kernel", "msm_bucket_kernel", "g2_mul2_kernel"):
        assert t[key]["hbm_bytes_per_launch"] > 0 and t[key]["units_per_launch"] > 0, key
    assert abs(i["cycles_per_valu_inst"] - 4.06) < 0.2 and i["simds"] == 1024
    src = open(os.path.join(ROOT, "bench.py")).read()
    for kern in ("g1_mul_kernel", "g2_mul2_kernel", "pair3_queue_kernel", "miller3_queue_kernel", "fexp3_queue_kernel", "msm_bucket_kernel",
                 "pair3_prod_fixed_queue_kernel"):
        k = i["kernels"][kern]
        assert k["valu_insts_per_launch"] > 1e8 and 1.5 < k["clock_GHz"] < 2.6 and k["units_per_launch"] > 0, kern
        assert kern in src, kern
        # the issue time of the counter pass's launch is a plausible kernel time (0.5 ms .. 100 ms)
        ms = k["valu_insts_per_launch"] * i["cycles_per_valu_inst"] / i["simds"] / (k["clock_GHz"] * 1e9) * 1e3
        assert 0.5 < ms < 100, (kern, ms)


def test_bench_gpus_flag_without_a_gpu():
    """No compute here (there is no GPU): `bench.py --gpus 2` started plainly must turn into the launcher of two ranks — each of which then
    stops for want of a HIP device — and under a launcher whose world size contradicts --gpus it must refuse before doing anything."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    # this is the "not gpu" suite: the devices are hidden, so that on a box WITH GPUs the two ranks stop at the same place as here instead of
    # running a full-size 2-rank benchmark from a CPU test
    env.update({"HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""})
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert "starting 2 ranks" in r.stderr
    assert r.returncode != 0 and r.stderr.count("needs a HIP device") >= 2, r.stderr[-2000:]
    env.update({"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "refusing" in r.stderr + r.stdout


def test_bench_all_configs_needs_full():
    """The extra configurations are part of the --full run: asked for in a plain run, bench.py stops before it touches a device."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update({"HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""})
    r = subprocess.run([sys.executable, "bench.py", "--all-configs"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "needs --full" in r.stderr and "HIP device" not in r.stderr, r.stderr[-2000:]
    r = subprocess.run([sys.executable, "bench.py", "--all-configs", "--full"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "needs a HIP device" in r.stderr, r.stderr[-2000:]


def test_build_refuses_a_compiler_it_was_not_validated_with(monkeypatch):
    """crypto12381_amd/build.py: 3-4 % of every kernel hang on an LLVM pass gate of one compiler and the wrong-lanes event of round 1 was a build-variant
    effect, so another `hipcc --version` stops the build unless the caller says it will run the every-lane tests; the pass gate is probed."""
    from crypto12381_amd import build as b
    if b._hipcc_version() is None:
        pytest.skip("no hipcc on this machine")
    monkeypatch.setattr(b, "_HIPCC_VERSION", None)
    monkeypatch.setattr(b, "VALIDATED_COMPILER", "a compiler that does not exist")
    monkeypatch.delenv("C12381_ALLOW_UNVALIDATED_COMPILER", raising=False)
    with pytest.raises(RuntimeError, match="not the compiler this library was validated with"):
        b._hipcc_version()
    monkeypatch.setattr(b, "_HIPCC_VERSION", None)
    monkeypatch.setenv("C12381_ALLOW_UNVALIDATED_COMPILER", "1")
    assert b._hipcc_version()
    monkeypatch.setattr(b, "_HIPCC_VERSION", None)
    monkeypatch.undo()
    b._check_pass_gate()
    assert b._PASS_GATE_OK is True
