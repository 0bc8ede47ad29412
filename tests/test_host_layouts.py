"""CPU test of the host API's slab layouts (crypto12381_amd/csrc/host_layouts.hpp): tests/host_sim/host_layouts.cpp, a stand-alone program built
with -fsanitize=address,undefined, carves every layout on a malloc of exactly its size and writes every field with the byte count the entry's
kernels write — fields 256-byte aligned, pairwise disjoint, inside the slab; n in {1, 3, 64, 65, 257}, msg_len in {0, 1, 31, 32, 40}, units /
nblk / nmsg in {0, 1, 2}, k up to C12381_FIXED_G2_MAX.  The pairing work queue's slab (pair_queue_layout) is checked for n at and beside 21 x
{1, 2047, 2048, 2049, 3121, 6144, 6145, 12484} groups under overrides {0, 1, 1024, above the group count}, tagged and fenced: ndirect + nq ==
groups, the split equal to a literal transcription of the rule, every queued group's block inside `bytes`, a head of groups + 2 words."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "crypto12381_amd", "csrc")


def test_every_layout_is_aligned_disjoint_and_inside_its_slab():
    exe = os.path.join(SIM_DIR, "host_layouts")
    srcs = [os.path.join(SIM_DIR, "host_layouts.cpp"), os.path.join(CSRC, "host_layouts.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, srcs[0]], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host layouts ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


def test_the_program_knows_the_public_bound_of_k():
    header = open(os.path.join(ROOT, "include", "c12381_hip.h")).read()
    prog = open(os.path.join(SIM_DIR, "host_layouts.cpp")).read()
    assert re.search(r"#define C12381_FIXED_G2_MAX (\d+)", header).group(1) == re.search(r"FIXED_G2_MAX = (\d+);", prog).group(1)


def test_no_entry_spells_a_slab_by_offsets():
    """the host units take their workspace fields from host_layouts.hpp: no `o_x = round_up(...)` chain, and the HIP launch macro in host.hpp alone"""
    for fn in os.listdir(CSRC):
        if fn.endswith(".hip") and not fn.startswith("k_"):
            text = open(os.path.join(CSRC, fn)).read()
            assert not re.search(r"\bo_\w+ = round_up\(", text), fn
            assert "hipLaunchKernelGGL" not in text, fn


def test_the_queue_split_is_stated_on_the_host():
    """one rule (host_layouts.hpp queue_direct_groups), evaluated by pair_queue_setup; the one kernel that still evaluates the split itself
    (gt3_pow_queue_kernel, k_pair3.hip gt_pow_direct_groups) carries the same lines, and no other unit has a rule or reads the device override"""
    body = lambda text, name: re.search(name + r"\(size_t ngroups, size_t nwaves[^)]*\) \{\n(.*?)\n\}", text, re.S).group(1)
    host = body(open(os.path.join(CSRC, "host_layouts.hpp")).read(), "inline size_t queue_direct_groups")
    dev = body(open(os.path.join(CSRC, "k_pair3.hip")).read(), "size_t gt_pow_direct_groups")
    dev = dev.replace("    const int ov = g_queue_groups_override;\n", "").replace("ov", "override_groups")
    assert [l.split("//")[0].rstrip() for l in dev.split("\n")] == [l.split("//")[0].rstrip() for l in host.split("\n")]
    for fn in os.listdir(CSRC):
        if not os.path.isfile(os.path.join(CSRC, fn)):
            continue
        text = open(os.path.join(CSRC, fn)).read()
        if fn not in ("host_layouts.hpp", "k_pair3.hip"):       # a call or a second definition; a comment may name the rule
            assert not re.search(r"^[^/\n]*\b\w*direct_groups\w*\(", text, re.M), fn
            assert "g_queue_groups_override" not in text, fn
    assert open(os.path.join(CSRC, "k_pair3.hip")).read().count("gt_pow_direct_groups(") == 2       # its definition and gt3_pow_queue_kernel
