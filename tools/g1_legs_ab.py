#!/usr/bin/env python3
"""A/B of two or more builds of the C ABI on the G1 scalar-multiplication legs, in ONE GPU session: the plain G1 leg of bench.py (2^20 lanes, its
inputs and seeds, 96-byte output, `--steps` calls per measurement bracketed by a synchronise: ms_per_step) with the g1_mul_kernel launch
time of the same steps (c12381_profile), and c12381_g1_mul_sum_batch_dev at k = 2, 3 and 4 on 2^20 lanes (inputs of tools/ab_bench.py).
One child process per library stays alive with its inputs resident on the device (the pattern of tools/host_tables_ab.py); the parent lets
them run one measurement at a time, alternately (A B C A B C ...), so that clock drift of the box hits both alike.  Per leg and library: median
and min - max over --rounds measurements, a SHA-256 of the output, and — where lib/libc12381_probe.so is built — the clock the chip holds
inside the G1 leg (bench.ClockProbe), taken once per library after the rounds.
Every further library is set against the first (A, the baseline): it counts as FASTER (SLOWER) on a leg only when the medians differ by
more than the larger of the two min - max spreads.
Exit status 1 when a digest differs or a child fails.

    python tools/g1_legs_ab.py [--rounds 7] [--steps 5] [--legs g1,g1sum2] [--out profiles/x.txt] <A.so | default> <B.so | default> [<C.so> ...]"""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(steps):
    import torch
    torch.cuda.init()
    import tools.libsel  # noqa: F401  (C12381_LIB -> capi.use_library)
    import bench
    from crypto12381_amd import Context
    from tools.prof_driver import G1, sc
    c = Context(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    c.set_stream(stream.cuda_stream)
    d = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    n = 1 << 20
    # bench.py's plain G1 leg: P_i = G^(s_i), seeds 1000 / 2000 (rank 0), edge scalars in front
    base_sc, ksc = torch.from_numpy(bench.make_scalars(1000, n)).to(dev), torch.from_numpy(bench.make_scalars(2000, n)).to(dev)
    gen1, pts, out = d(bench.G1_GEN), torch.empty(n * 96, dtype=torch.uint8, device=dev), torch.empty(n * 96, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    c.g1_mul_fixed_dev(n, gen1.data_ptr(), base_sc.data_ptr(), pts.data_ptr(), 96)
    assert c.sync() == 0
    legs = {"g1": (lambda: c.g1_mul_dev(n, pts.data_ptr(), ksc.data_ptr(), out.data_ptr(), 96), out)}
    p1k = c.g1_mul(G1 * 1024, sc(3, 1024), 96)
    keep = []
    for k in (2, 3, 4):                  # as rows g1sum2, g1sum4 of tools/ab_bench.py: term j takes the points rotated by 37 j records
        dp = d(b"".join((p1k[96 * 37 * j:] + p1k[:96 * 37 * j]) * (n // 1024) for j in range(k)))
        dk, o = d(b"".join(sc(20 + j, n) for j in range(k))), torch.empty(96 * n, dtype=torch.uint8, device=dev)
        keep.append((dp, dk, o))
        legs["g1sum%d" % k] = (lambda k=k, dp=dp, dk=dk, o=o: c.g1_mul_sum_dev(n, k, dp.data_ptr(), dk.data_ptr(), o.data_ptr(), 96), o)
    probe = bench.ClockProbe(0, dev)
    torch.cuda.synchronize(dev)
    print("READY " + "|".join(legs), flush=True)
    for line in sys.stdin:
        name = line.strip()
        if name == "quit":
            break
        if name == "clock":
            ghz = probe.during(legs["g1"][0], c.sync)
            print("C %s" % ("%.4f" % ghz if ghz else "none"), flush=True)
            continue
        fn, res = legs[name]
        torch.cuda.synchronize(dev)
        c.profile(True)
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        kms, launches = c.profile_read(0)
        c.profile(False)
        rc = c.sync()
        print("T %.4f %.4f %d %s" % (dt / steps * 1e3, kms / max(launches, 1), rc, hashlib.sha256(res.cpu().numpy().tobytes()).hexdigest()[:16]), flush=True)
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--legs", default=None, help="comma separated subset of g1,g1sum2,g1sum3,g1sum4 (default: all)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("libs", nargs="*")
    a = ap.parse_args()
    if a.child:
        child(a.steps)
        return
    assert len(a.libs) >= 2, "at least two libraries: A (the baseline), B, ..."
    kids = []
    for lib in a.libs:
        env = dict(os.environ)
        env.pop("C12381_LIB", None)
        if lib != "default":
            env["C12381_LIB"] = os.path.abspath(lib)
        kids.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps)], cwd=ROOT, env=env,
                                     stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1))

    def answer(k, tag):
        while True:
            line = k.stdout.readline()
            if not line:
                raise SystemExit("a child ended early (rc %s): nothing further is started" % k.poll())
            if line.startswith(tag):
                return line.split()[1:]
    legs = [" ".join(answer(k, "READY")) for k in kids][0].split("|")
    if a.legs:
        legs = [leg for leg in legs if leg in a.legs.split(",")]

    def call(k, leg):
        k.stdin.write(leg + "\n")
        k.stdin.flush()
        ms, kms, rc, dig = answer(k, "T ")
        if int(rc) != 0:
            raise SystemExit("%s: status %s" % (leg, rc))
        return float(ms), float(kms), dig
    fmt = lambda x: "%.3f (%.3f - %.3f)" % (statistics.median(x), min(x), max(x))
    tags = [chr(ord("A") + i) for i in range(len(kids))]
    lines = ["%s; one MI355X, one child process per library, %d alternated measurements per leg after one warm-up each;"
             % (", ".join("%s = %s" % tl for tl in zip(tags, a.libs)), a.rounds),
             "ms_per_step = wall ms of %d back-to-back calls / %d, synchronised before and after; kernel = mean g1_mul_kernel launch of the same steps;" % (a.steps, a.steps),
             "median (min - max); verdict against A: the medians differ by more than the larger of the two min - max spreads, or not"]
    bad = False
    for leg in legs:
        digs = [call(k, leg)[2] for k in kids]                  # warm-up: workspaces grown, code objects loaded
        t, kt = [[] for _ in kids], [[] for _ in kids]
        for _ in range(a.rounds):
            for i, k in enumerate(kids):
                ms, kms, dig = call(k, leg)
                t[i].append(ms)
                kt[i].append(kms)
                digs.append(dig)
        same = len(set(digs)) == 1
        bad |= not same
        for name, v in (("ms_per_step", t),) + ((("kernel ms", kt),) if leg == "g1" else ()):
            lines.append("%-7s %-12s A %s   digests %s" % (leg, name, fmt(v[0]), "equal" if same else "DIFFER"))
            for i in range(1, len(kids)):
                ma, mb = statistics.median(v[0]), statistics.median(v[i])
                spread = max(max(v[0]) - min(v[0]), max(v[i]) - min(v[i]))
                verdict = "FASTER" if ma - mb > spread else ("SLOWER" if mb - ma > spread else "no difference beyond the spread")
                lines.append("%-7s %-12s %s %s   %+.2f %% (%s - A %+.3f ms, spread %.3f ms): %s"
                             % ("", "", tags[i], fmt(v[i]), (mb / ma - 1) * 100, tags[i], mb - ma, spread, verdict))
            print("\n".join(lines[-len(kids):]), flush=True)
    clocks = []
    for k in kids:
        k.stdin.write("clock\n")
        k.stdin.flush()
        clocks.append(answer(k, "C ")[0])
    lines.append("in-kernel clock during the g1 leg (GHz, mean over the XCDs; one 0.25 s run per library after the rounds): "
                 + "  ".join("%s %s" % tc for tc in zip(tags, clocks)))
    for k in kids:
        k.stdin.write("quit\n")
        k.stdin.flush()
        k.wait(timeout=60)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
