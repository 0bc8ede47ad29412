"""A/B of the K-way fixed-G2 entry points against what a caller composes today, in one process, device-event timing on the
context's stream, warm-up, interleaved A/B/A/B; the outputs of both sides are compared for equality (SHA-256 digests).

  ps_verify:  c12381_ps_verify_batch_dev  vs  the composed route:  g2_mul_fixed per message column, g2_add (host form: the
              ABI has no _dev twin), pair_eq.  `composed_dev` leaves the g2_add step out: a lower bound for a caller with a
              device-side addition of its own.
  product:    c12381_pair_product_fixed_g2_batch_dev  vs  c12381_pair_product_batch_dev on replicated G2 points.

    python tools/ps_verify_bench.py [--rounds 3] [--out profiles/ps_verify_ab.txt]"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ps_verify_ab.txt"))
    ap.add_argument("--sizes", default="16,18")
    ap.add_argument("--nmsgs", default="0,1,3,6")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    from crypto12381_amd.capi import _p
    from util import golden, prng
    ctx = Context(0)
    stream = torch.cuda.Stream()                     # not the null stream: c12381_set_stream(0) would give the context a stream of its own
    ctx.set_stream(stream.cuda_stream)
    torch.cuda.set_stream(stream)                    # the tensors' copies run in the same stream order as the library's kernels
    G1 = bytes.fromhex(golden("g1")["generator"])
    G2 = bytes.fromhex(golden("g2")["generator"])
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    b32 = lambda k: (k % (1 << 256)).to_bytes(32, "big")
    lines = ["# tools/ps_verify_bench.py: ms per call, one MI355X, device events on the context's stream; %d interleaved rounds after one warm-up"
             % args.rounds, "# digest = first 12 hex digits of SHA-256 over the outputs; equal digests on both sides of a row"]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def ab(fa, fb, oa, ob):
        fa(); fb()
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(fa)); tb.append(timed(fb))
        ctx.sync()
        da = hashlib.sha256(bytes(oa().cpu().numpy())).hexdigest()[:12]
        db = hashlib.sha256(bytes(ob().cpu().numpy())).hexdigest()[:12]
        return ta, tb, da, db

    fmt = lambda ts: "min %8.2f mean %8.2f" % (min(ts), sum(ts) / len(ts))
    for lg in [int(v) for v in args.sizes.split(",")]:
        n = 1 << lg
        g1s = ctx.g1_mul(G1 * n, b"".join(b32(prng(9900 + lg, j) % R) for j in range(n)), 96)
        for nmsg in [int(v) for v in args.nmsgs.split(",")]:
            x = prng(9800, 0) % R
            y = [prng(9800, 1 + i) % R for i in range(nmsg)]
            X2 = ctx.g2_mul(G2, b32(x), 192)
            Y2 = b"".join(ctx.g2_mul(G2, b32(v), 192) for v in y)
            m = [[prng(9700 + i, j) % R for j in range(n)] for i in range(nmsg)]
            mb = b"".join(b32(m[i][j]) for i in range(nmsg) for j in range(n))
            e = b"".join(b32((x + sum(y[i] * m[i][j] for i in range(nmsg))) % R) for j in range(n))
            s2 = ctx.g1_mul(g1s, e, 96)
            if n > 64:                                        # a few wrong signatures, so the digests see both answers
                s2 = g1s[:96 * 64] + s2[96 * 64:]
            t_g2, t_X2, t_Y2, t_s1, t_s2 = dev(G2), dev(X2), dev(Y2 or b"\0"), dev(g1s), dev(s2)
            t_m = dev(mb or b"\0")
            t_g2n = dev(G2 * n)
            ok_a = torch.zeros(n, dtype=torch.uint8, device="cuda")
            ok_b = torch.zeros(n, dtype=torch.uint8, device="cuda")
            cols = torch.zeros(max(nmsg, 1) * 192 * n, dtype=torch.uint8, device="cuda")
            W = torch.zeros(192 * n, dtype=torch.uint8, device="cuda")

            def fast():
                ctx.ps_verify_dev(n, nmsg, t_g2.data_ptr(), t_X2.data_ptr(), t_Y2.data_ptr() if nmsg else None, t_s1.data_ptr(),
                                  t_s2.data_ptr(), t_m.data_ptr() if nmsg else None, ok_a.data_ptr())

            def composed_muls():
                for i in range(nmsg):
                    ctx.g2_mul_fixed_dev(n, t_Y2.data_ptr() + 192 * i, t_m.data_ptr() + 32 * n * i, cols.data_ptr() + 192 * n * i, 192)

            def composed_adds():
                w = X2 * n
                if nmsg:
                    c = bytes(cols.cpu().numpy())
                    for i in range(nmsg):
                        w = ctx.g2_add(w, c[192 * n * i:192 * n * (i + 1)], 192)
                W.copy_(torch.frombuffer(bytearray(w), dtype=torch.uint8))

            def composed_pair():
                ctx.pair_eq_dev(n, t_s1.data_ptr(), W.data_ptr(), t_s2.data_ptr(), t_g2n.data_ptr(), ok_b.data_ptr())

            def composed():
                composed_muls(); composed_adds(); composed_pair()

            ta, tb, da, db = ab(fast, composed, lambda: ok_a, lambda: ok_b)
            tm = [timed(composed_muls) for _ in range(args.rounds)]
            tp = [timed(composed_pair) for _ in range(args.rounds)]
            ctx.sync()
            dev_only = [a + b for a, b in zip(tm, tp)]
            ones = int(ok_a.sum().item())
            lines.append("ps_verify n=2^%d nmsg=%d  fast %s | composed %s | composed_dev %s | speed-up %.2fx (vs composed_dev %.2fx) | "
                         "digest %s %s %s | ok=1 lanes %d" % (lg, nmsg, fmt(ta), fmt(tb), fmt(dev_only), min(tb) / min(ta),
                                                             min(dev_only) / min(ta), da, db, "EQUAL" if da == db else "DIFFER", ones))
            print(lines[-1], flush=True)
            del t_g2, t_X2, t_Y2, t_s1, t_s2, t_m, t_g2n, cols, W
    # the GT product against pair_product_batch on replicated points
    n = 1 << 16
    g1s = ctx.g1_mul(G1 * n, b"".join(b32(prng(9600, j) % R) for j in range(n)), 96)
    for k in (2, 3):
        qs = [ctx.g2_mul(G2, b32(prng(9500, j) % R), 192) for j in range(k)]
        t_p = dev(b"".join(g1s[96 * ((j * 7919) % n):] + g1s[:96 * ((j * 7919) % n)] for j in range(k)))
        t_q, t_qn = dev(b"".join(qs)), dev(b"".join(q * n for q in qs))
        ga = torch.zeros(576 * n, dtype=torch.uint8, device="cuda")
        gb = torch.zeros(576 * n, dtype=torch.uint8, device="cuda")
        ta, tb, da, db = ab(lambda: ctx.pair_product_fixed_g2_dev(n, k, t_p.data_ptr(), t_q.data_ptr(), ga.data_ptr()),
                            lambda: ctx._ck(ctx.lib.c12381_pair_product_batch_dev(ctx.h, n, k, _p(t_p.data_ptr()), _p(t_qn.data_ptr()), _p(gb.data_ptr()), 0)), lambda: ga, lambda: gb)
        ctx.sync()
        lines.append("pair_product n=2^16 k=%d  fixed_g2 %s | pair_product %s | speed-up %.2fx | digest %s %s %s"
                     % (k, fmt(ta), fmt(tb), min(tb) / min(ta), da, db, "EQUAL" if da == db else "DIFFER"))
        print(lines[-1], flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
