#!/usr/bin/env python3
"""Compare the kernel launches of two builds of the C ABI, leg by leg, from two rocprofv3 --kernel-trace runs of
`tools/host_tables_ab.py --trace` (one per library).  Each trace is cut at the marker launches (fp_mulchain_kernel on 256 (i + 1) threads in front
of and behind the traced call of leg i); within a leg the launches are taken per stream in start order — streams run beside each other, so the order ACROSS
streams is not a property of the library — as (kernel name, grid size, workgroup size).  Equal means the same ordered list on every stream, not
an equal count.  Exit status 1 when a leg differs.

    python tools/launch_compare.py <trace dir A> <trace dir B> <traced stdout of either run> [--out profiles/host_split_launches.txt]"""
import argparse
import collections
import csv
import glob
import re
import sys


def legs_of(trace_dir):
    path = glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    legs, cur = {}, None
    for r in rows:
        name = re.sub(r"^void ", "", r["Kernel_Name"]).split("(")[0]
        shape = tuple(int(r[k]) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X") if k in r) or (int(r["Grid_Size"]),)
        if "fp_mulchain_kernel" in name:                       # the first marker of a size opens its leg, the second one closes it
            cur = None if cur is not None else shape[0] // 256 - 1
            if cur is not None:
                legs[cur] = collections.OrderedDict()
            continue
        if cur is None:
            continue
        stream = r.get("Stream_Id") or r.get("Queue_Id") or "?"
        legs[cur].setdefault(stream, []).append((name, shape))
    # streams by order of first use: their ids differ between processes
    return {i: list(v.values()) for i, v in legs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a"), ap.add_argument("b"), ap.add_argument("traced")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    names = {int(m.group(1)): m.group(2) for m in re.finditer(r"^TRACED (\d+) (\S+)", open(args.traced).read(), re.M)}
    A, B = legs_of(args.a), legs_of(args.b)
    lines = ["%-22s %9s %9s %8s   %s" % ("leg", "A kernels", "B kernels", "streams", "ordered (kernel, grid, workgroup) lists per stream")]
    bad = False
    for i in sorted(set(A) | set(B)):
        a, b = A.get(i, []), B.get(i, [])
        same = a == b
        bad |= not same
        lines.append("%-22s %9d %9d %8d   %s" % (names.get(i, "leg %d" % i), sum(map(len, a)), sum(map(len, b)), len(a), "equal" if same else "DIFFER"))
        if not same:
            for sa, sb in zip(a, b):
                for k, (x, y) in enumerate(zip(sa, sb)):
                    if x != y:
                        lines.append("    first difference at launch %d of a stream: %s %s  |  %s %s" % (k, x[0][:60], x[1], y[0][:60], y[1]))
                        break
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        open(args.out, "w").write(text)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
