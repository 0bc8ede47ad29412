"""A/B of the per-lane sum of k G1 products (c12381_g1_mul_sum_batch) against the entry points a caller has without it, in ONE process:
inputs resident on the device, every shape warmed, HIP events on the context's stream, the sides ALTERNATED in the same run, median and
min-max per side; the outputs of the sides are compared on all lanes before anything is timed.

  A   c12381_g1_mul_sum_batch_dev, 96-byte output
  B   k x c12381_g1_mul_batch_dev, 96-byte output, the k - 1 additions LEFT OUT: a lower bound no entry offers today
  Ah  c12381_g1_mul_sum_batch (host pointers)
  C   k x c12381_g1_mul_batch + (k - 1) x c12381_g1_add_batch (host pointers): what a caller composes today

A beats B when median(B) - median(A) exceeds the larger min-max spread of the two sides.

    python tools/g1_mul_sum_ab.py [--reps 10] [--sizes 18,20] [--ks 2,3,4] [--out profiles/g1_mul_sum_ab.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sizes", default="18,20")
    ap.add_argument("--ks", default="2,3,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g1_mul_sum_ab.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    from util import golden
    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    torch.cuda.set_stream(stream)
    g = torch.frombuffer(bytearray(bytes.fromhex(golden("g1")["generator"])), dtype=torch.uint8).cuda()
    lines = ["# tools/g1_mul_sum_ab.py: ms per call on one MI355X; device rows: HIP events on the context's stream, %d alternated repetitions after a warm-up of"
             % args.reps, "# every side; host rows: wall clock around the synchronous host forms, %d alternated repetitions.  median [min .. max]" % args.host_reps,
             "# A = g1_mul_sum_batch_dev   B = k x g1_mul_batch_dev (additions left out)   Ah = g1_mul_sum_batch   C = k x g1_mul_batch + (k-1) x g1_add_batch"]

    def ev(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    fmt = lambda ts: "%8.2f [%8.2f .. %8.2f]" % (statistics.median(ts), min(ts), max(ts))
    for lg in [int(v) for v in args.sizes.split(",")]:
        n = 1 << lg
        kmax = max(int(v) for v in args.ks.split(","))
        rng = np.random.Generator(np.random.PCG64(9950 + lg))
        base = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        base[:, 0] &= 0x3f
        col = torch.empty(96 * n, dtype=torch.uint8, device="cuda")
        ctx.g1_mul_fixed_dev(n, g.data_ptr(), torch.from_numpy(base.reshape(-1)).cuda().data_ptr(), col.data_ptr(), 96)
        ctx.sync()
        pts = torch.cat([torch.roll(col.view(n, 96), 7919 * j, 0).reshape(-1) for j in range(kmax)]).contiguous()
        sc = torch.from_numpy(rng.integers(0, 256, size=(kmax * n * 32,), dtype=np.uint8)).cuda()
        out_a = torch.empty(96 * n, dtype=torch.uint8, device="cuda")
        out_b = torch.empty(96 * n * kmax, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        h_pts, h_sc = pts.cpu().numpy().tobytes(), sc.cpu().numpy().tobytes()
        for k in [int(v) for v in args.ks.split(",")]:
            def side_a():
                ctx.g1_mul_sum_dev(n, k, pts.data_ptr(), sc.data_ptr(), out_a.data_ptr(), 96)

            def side_b():
                for j in range(k):
                    ctx.g1_mul_dev(n, pts.data_ptr() + 96 * n * j, sc.data_ptr() + 32 * n * j, out_b.data_ptr() + 96 * n * j, 96)

            def side_ah():
                return ctx.g1_mul_sum(h_pts[:96 * n * k], h_sc[:32 * n * k], k, 96)

            def side_c():
                acc = ctx.g1_mul(h_pts[:96 * n], h_sc[:32 * n], 96)
                for j in range(1, k):
                    acc = ctx.g1_add(acc, ctx.g1_mul(h_pts[96 * n * j:96 * n * (j + 1)], h_sc[32 * n * j:32 * n * (j + 1)], 96), 96)
                return acc

            # all lanes equal before anything is timed (these calls are the warm-up of every shape)
            side_a(); side_b()
            assert ctx.sync() == 0
            ra, rc_ = side_ah(), side_c()
            same = ra == rc_ and out_a.cpu().numpy().tobytes() == ra
            cols = out_b.cpu().numpy().tobytes()
            acc = cols[:96 * n]
            for j in range(1, k):
                acc = ctx.g1_add(acc, cols[96 * n * j:96 * n * (j + 1)], 96)
            same = same and acc == ra
            ta, tb, tah, tc = [], [], [], []
            for _ in range(args.reps):
                ta.append(ev(side_a)); tb.append(ev(side_b))
            assert ctx.sync() == 0
            for _ in range(args.host_reps):
                tah.append(wall(side_ah)); tc.append(wall(side_c))
            spread = max(max(ta) - min(ta), max(tb) - min(tb))
            gain = statistics.median(tb) - statistics.median(ta)
            lines.append("n=2^%d k=%d  A %s | B %s | A/B %.3f | B-A %.2f vs spread %.2f: %s | Ah %s | C %s | Ah/C %.3f | all lanes %s"
                         % (lg, k, fmt(ta), fmt(tb), statistics.median(ta) / statistics.median(tb), gain, spread,
                            "A FASTER" if gain > spread else "NOT FASTER", fmt(tah), fmt(tc), statistics.median(tah) / statistics.median(tc),
                            "EQUAL" if same else "DIFFER"))
            print(lines[-1], flush=True)
        del pts, sc, out_a, out_b, col
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
