#!/usr/bin/env python3
"""c12381_g1_mul_fixed_sum_batch against what a caller composes without it, in ONE GPU session: 2^20 lanes, nb = 2, 4, 8, 16, 32 subgroup
bases, the legs interleaved repeat by repeat (A B A B ...), median / min / max wall ms per call, SHA-256 of the outputs.

    python tools/g1_fixed_sum_bench.py [--log2n 20] [--nb 2,4,8,16,32] [--reps 5] [--host-reps 5] [--out profiles/g1_fixed_sum_ab.txt]

Legs, inputs resident on the device for the first two:
  fused      c12381_g1_mul_fixed_sum_batch_dev
  columns    nb x c12381_g1_mul_fixed_batch_dev into one buffer, WITHOUT the nb - 1 additions (c12381_g1_add_batch has no _dev form): all a
             device-side caller can compose, and a lower bound for that route
  host       c12381_g1_mul_fixed_sum_batch (host buffers) against nb x c12381_g1_mul_fixed_batch + (nb - 1) x c12381_g1_add_batch
Parity: the digests of fused, host and composed-host outputs must be equal (the columns leg has no sum to compare).  Exit status 1 when
they differ.  A line "EXCESS" marks an nb at which the fused median exceeds the columns median by more than the spread (max - min) of that
nb's own repeats."""
import argparse
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--nb", default="2,4,8,16,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("g1_fixed_sum_bench: needs a HIP device")
    torch.cuda.init()
    from crypto12381_amd import Context
    from tools.prof_driver import G1, sc
    c = Context(0)
    dev = torch.device("cuda", 0)
    n = 1 << a.log2n
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def d(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def digest(b):
        return hashlib.sha256(b).hexdigest()[:16]

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        c.sync()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ts):
        return "%8.2f %8.2f %8.2f" % (statistics.median(ts), min(ts), max(ts))

    say("g1_mul_fixed_sum: n = 2^%d lanes, %d device repeats, %d host repeats; wall ms per call: median min max" % (a.log2n, a.reps, a.host_reps))
    bad = False
    for nb in [int(x) for x in a.nb.split(",")]:
        red = bytearray(sc(70 + nb, nb))
        for i in range(nb):
            red[32 * i] &= 0x3f
        bases = c.g1_mul_fixed(G1, bytes(red), 96)                       # nb subgroup points
        gen = torch.Generator(device=dev)
        gen.manual_seed(7100 + nb)
        dsc = torch.randint(0, 256, (nb * n * 32,), dtype=torch.uint8, device=dev, generator=gen)
        dbases = d(bases)
        out = torch.empty(96 * n, dtype=torch.uint8, device=dev)
        col = torch.empty(96 * n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

        def fused():
            c.g1_mul_fixed_sum_dev(n, nb, dbases.data_ptr(), dsc.data_ptr(), out.data_ptr(), None, 96)

        def columns():
            for i in range(nb):
                c.g1_mul_fixed_dev(n, dbases.data_ptr() + 96 * i, dsc.data_ptr() + 32 * n * i, col.data_ptr(), 96)

        timed(fused); timed(columns)                                     # warm-up: tables, workspaces
        t_f, t_c = [], []
        for _ in range(a.reps):
            t_f.append(timed(fused)[0])
            t_c.append(timed(columns)[0])
        dg_fused = digest(out.cpu().numpy().tobytes())
        # the columns leg rebuilds its one table nb times per call (every base through one slot); the fused leg's tables are cached
        say("nb %2d  fused   %s   digest %s" % (nb, stats(t_f), dg_fused))
        say("nb %2d  columns %s   (no additions)" % (nb, stats(t_c)))
        excess = statistics.median(t_f) - statistics.median(t_c)
        spread = max(max(t_f) - min(t_f), max(t_c) - min(t_c))
        say("nb %2d  fused - columns = %+.2f ms, spread %.2f ms, ratio %.3f  %s" % (nb, excess, spread, statistics.median(t_f) / statistics.median(t_c),
                                                                                 "EXCESS" if excess > spread else "ok"))
        if a.host_reps > 0:
            hsc = dsc.cpu().numpy().tobytes()

            def host_fused():
                return c.g1_mul_fixed_sum(bases, hsc, None, 96)

            def host_composed():
                acc = c.g1_mul_fixed(bases[:96], hsc[:32 * n], 96)
                for i in range(1, nb):
                    acc = c.g1_add(acc, c.g1_mul_fixed(bases[96 * i:96 * i + 96], hsc[32 * n * i:32 * n * (i + 1)], 96), 96)
                return acc

            t_hf, t_hc = [], []
            for _ in range(a.host_reps):
                t, r_f = timed(host_fused)
                t_hf.append(t)
                t, r_c = timed(host_composed)
                t_hc.append(t)
            dg_hf, dg_hc = digest(r_f), digest(r_c)
            say("nb %2d  host fused    %s   digest %s" % (nb, stats(t_hf), dg_hf))
            say("nb %2d  host composed %s   digest %s" % (nb, stats(t_hc), dg_hc))
            same = dg_fused == dg_hf == dg_hc
            say("nb %2d  digests %s" % (nb, "equal" if same else "DIFFER"))
            bad |= not same
            del hsc, r_f, r_c
        del dsc, out, col
    c.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
