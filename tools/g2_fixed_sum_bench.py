#!/usr/bin/env python3
"""c12381_g2_mul_fixed_sum_batch against what a caller composes without it, and PS verification with many messages against the parent
commit's library, in ONE GPU session: 2^18 lanes, nb = 2, 4, 8, 16, 32 elements of G2, the legs interleaved repeat by repeat (A B A B ...),
median / min / max wall ms per call, SHA-256 of the outputs.

    python tools/g2_fixed_sum_bench.py [--log2n 18] [--nb 2,4,8,16,32] [--reps 5] [--host-reps 3] [--ps-nmsg 8,16] [--parent-lib <.so>]
                                       [--out profiles/g2_fixed_sum_ab.txt]

Legs, inputs resident on the device for the first two:
  fused      c12381_g2_mul_fixed_sum_batch_dev
  columns    nb x c12381_g2_mul_fixed_batch_dev into one buffer, WITHOUT the nb - 1 additions (c12381_g2_add_batch has no _dev form): all a
             device-side caller can compose, and a lower bound for that route
  host       c12381_g2_mul_fixed_sum_batch (host buffers) against nb x c12381_g2_mul_fixed_batch + (nb - 1) x c12381_g2_add_batch
  ps         c12381_ps_verify_batch_dev at the given nmsg, this build against --parent-lib (the parent commit's csrc built by
             tools/build_variant.sh with CSRC=<parent checkout>/crypto12381_amd/csrc): one child process per library, called alternately;
             both children go through ctypes directly, since the parent library has no symbol for the binding's new entry
Parity: the digests of fused, host and composed-host outputs must be equal (the columns leg has no sum to compare), and so must the two
libraries' verdict arrays.  Exit status 1 when they differ.  A line "EXCESS" marks an nb at which the fused median exceeds the columns
median by more than the spread (max - min) of that nb's own repeats: the condition of this entry is that no nb >= 2 shows it."""
import argparse
import ctypes
import hashlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
DISTINCT = 1024


def digest(b):
    return hashlib.sha256(b).hexdigest()[:16]


def stats(ts):
    return "%8.2f %8.2f %8.2f" % (statistics.median(ts), min(ts), max(ts))


def ps_child(lib_path, log2n, nmsgs):
    """one library, plain ctypes: PS batches of 2^log2n lanes (1024 distinct signatures, tiled; every 7th of them carries a wrong message)"""
    import numpy as np
    import torch
    torch.cuda.init()
    from tools.prof_driver import G1, G2, sc
    lib = ctypes.CDLL(lib_path)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.c12381_create.argtypes = [ci, ctypes.POINTER(vp)]
    lib.c12381_destroy.argtypes = [vp]
    lib.c12381_destroy.restype = None
    lib.c12381_sync.argtypes = [vp]
    lib.c12381_g1_mul_batch.argtypes = [vp, sz, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ci]
    lib.c12381_g2_mul_batch.argtypes = [vp, sz, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ci]
    lib.c12381_ps_verify_batch_dev.argtypes = [vp, sz, sz] + [vp] * 7
    h = vp()
    assert lib.c12381_create(0, ctypes.byref(h)) == 0
    dev = torch.device("cuda", 0)
    n = 1 << log2n
    d = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    b32 = lambda k: (k % R).to_bytes(32, "big")

    def ints(seed, m):
        b = sc(seed, m)
        return [int.from_bytes(b[32 * i:32 * i + 32], "big") % R for i in range(m)]

    def mul(fn, w, pts, ks):
        m = len(ks) // 32
        o = ctypes.create_string_buffer(w * m)
        assert fn(h, m, pts, ks, o, w) == 0
        return o.raw
    legs = {}
    for nmsg in nmsgs:
        x, y = ints(80 + nmsg, 1)[0], ints(81 + nmsg, nmsg)
        X2 = mul(lib.c12381_g2_mul_batch, 192, G2, b32(x))
        Y2 = mul(lib.c12381_g2_mul_batch, 192, G2 * nmsg, b"".join(b32(v) for v in y))
        msgs = [ints(90 + 40 * nmsg + i, DISTINCT) for i in range(nmsg)]
        s1 = mul(lib.c12381_g1_mul_batch, 96, G1 * DISTINCT, b"".join(b32(v or 1) for v in ints(82 + nmsg, DISTINCT)))
        s2 = mul(lib.c12381_g1_mul_batch, 96, s1, b"".join(b32(x + sum(y[i] * msgs[i][j] for i in range(nmsg))) for j in range(DISTINCT)))
        for j in range(0, DISTINCT, 7):
            msgs[j % nmsg][j] = (msgs[j % nmsg][j] + 1) % R
        tile = lambda b, w: np.tile(np.frombuffer(b, dtype=np.uint8).reshape(DISTINCT, w), (n // DISTINCT, 1)).tobytes()
        t = [d(G2), d(X2), d(Y2), d(tile(s1, 96)), d(tile(s2, 96)), d(b"".join(tile(b"".join(b32(v) for v in col), 32) for col in msgs))]
        ok = torch.zeros(n, dtype=torch.uint8, device=dev)
        legs["ps nmsg=%d" % nmsg] = (lambda nmsg=nmsg, t=t, ok=ok: lib.c12381_ps_verify_batch_dev(h, n, nmsg, *[v.data_ptr() for v in t], ok.data_ptr()), ok)
    torch.cuda.synchronize(dev)
    assert lib.c12381_sync(h) == 0
    print("READY " + "|".join(legs), flush=True)
    for line in sys.stdin:
        name = line.strip()
        if name == "quit":
            break
        fn, res = legs[name]
        t0 = time.perf_counter()
        rc = fn()
        rc = rc or lib.c12381_sync(h)
        dt = time.perf_counter() - t0
        r = res.cpu().numpy()
        print("T %.4f %d %s %d" % (dt * 1e3, rc, digest(r.tobytes()), int((r == 1).sum())), flush=True)
    lib.c12381_destroy(h)


def ps_ab(a, say):
    """the two children, one call at a time, alternately; -> True when a digest differs"""
    libs = [("this build", os.path.join(ROOT, "crypto12381_amd", "lib", "libc12381_hip.so"))]
    if a.parent_lib:
        libs.insert(0, ("parent", os.path.abspath(a.parent_lib)))
    else:
        say("ps: no --parent-lib given: this build alone")
    kids = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--ps-child", path, "--log2n", str(a.log2n), "--ps-nmsg", a.ps_nmsg], cwd=ROOT,
                             stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1) for _, path in libs]

    def answer(k, tag):
        while True:
            line = k.stdout.readline()
            if not line:
                raise SystemExit("a child ended early (rc %s): nothing further is started" % k.poll())
            if line.startswith(tag):
                return line[len(tag):].strip()
    legs = [answer(k, "READY ") for k in kids][0].split("|")

    def call(k, leg):
        k.stdin.write(leg + "\n")
        k.stdin.flush()
        ms, rc, dig, ones = answer(k, "T ").split()
        if int(rc) != 0:
            raise SystemExit("%s: status %s" % (leg, rc))
        return float(ms), dig, int(ones)
    bad = False
    for leg in legs:
        digs = [call(k, leg)[1] for k in kids]                  # warm-up: tables built, workspaces grown
        t = [[] for _ in kids]
        ones = 0
        for _ in range(a.reps):
            for i, k in enumerate(kids):
                ms, dig, ones = call(k, leg)
                t[i].append(ms)
                digs.append(dig)
        same = len(set(digs)) == 1
        bad |= not same
        for (name, _), ts in zip(libs, t):
            say("%-10s %-11s %s" % (leg, name, stats(ts)))
        if len(kids) == 2:
            say("%-10s this build / parent = %.3f, verdicts %s (%d of %d lanes valid)" % (leg, statistics.median(t[1]) / statistics.median(t[0]),
                                                                                        "equal" if same else "DIFFER", ones, 1 << a.log2n))
    for k in kids:
        k.stdin.write("quit\n")
        k.stdin.flush()
        k.wait(timeout=60)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--nb", default="2,4,8,16,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--ps-nmsg", default="8,16")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ps-child", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.ps_child:
        ps_child(a.ps_child, a.log2n, [int(x) for x in a.ps_nmsg.split(",")])
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("g2_fixed_sum_bench: needs a HIP device")
    torch.cuda.init()
    from crypto12381_amd import Context
    from tools.prof_driver import G2, sc
    c = Context(0)
    dev = torch.device("cuda", 0)
    n = 1 << a.log2n
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def d(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        c.sync()
        return (time.perf_counter() - t0) * 1e3, r

    say("g2_mul_fixed_sum: n = 2^%d lanes, %d device repeats, %d host repeats; wall ms per call: median min max" % (a.log2n, a.reps, a.host_reps))
    bad = False
    for nb in [int(x) for x in a.nb.split(",") if x]:
        red = bytearray(sc(70 + nb, nb))
        for i in range(nb):
            red[32 * i] &= 0x3f
        bases = c.g2_mul_fixed(G2, bytes(red), 192)                      # nb elements of G2
        gen = torch.Generator(device=dev)
        gen.manual_seed(7100 + nb)
        dsc = torch.randint(0, 256, (nb * n * 32,), dtype=torch.uint8, device=dev, generator=gen)
        dbases = d(bases)
        out = torch.empty(192 * n, dtype=torch.uint8, device=dev)
        col = torch.empty(192 * n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

        def fused():
            c.g2_mul_fixed_sum_dev(n, nb, dbases.data_ptr(), dsc.data_ptr(), out.data_ptr(), None, 192)

        def columns():
            for i in range(nb):
                c.g2_mul_fixed_dev(n, dbases.data_ptr() + 192 * i, dsc.data_ptr() + 32 * n * i, col.data_ptr(), 192)

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
                return c.g2_mul_fixed_sum(bases, hsc, None, 192)

            def host_composed():
                acc = c.g2_mul_fixed(bases[:192], hsc[:32 * n], 192)
                for i in range(1, nb):
                    acc = c.g2_add(acc, c.g2_mul_fixed(bases[192 * i:192 * i + 192], hsc[32 * n * i:32 * n * (i + 1)], 192), 192)
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
    del c
    torch.cuda.empty_cache()
    if a.ps_nmsg:
        say("ps_verify_dev: n = 2^%d lanes (%d distinct signatures, tiled), %d interleaved repeats; wall ms per call: median min max" % (a.log2n, DISTINCT, a.reps))
        bad |= ps_ab(a, say)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
