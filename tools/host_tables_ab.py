#!/usr/bin/env python3
"""A/B of two builds of the C ABI on the entry points that go through the host's table cache (csrc/host.hpp cached_tables), in ONE GPU
session.  One child process per library stays alive with its inputs resident on the device; the parent lets them run one call at a time,
alternately (A B A B ...), so that clock drift of the box hits both alike.  Per leg: median / min / max wall ms of --reps calls per
library and a SHA-256 of the output.  A leg is marked OUTSIDE when B's median is not within the min-max spread of A's own repeats
(the criterion of profiles/g1_fixed_sum_ab.txt).  Exit status 1 when a digest differs or a child fails.

    python tools/host_tables_ab.py [--reps 5] [--out profiles/host_tables_refactor_ab.txt] <A.so | default> <B.so | default>

Legs (sizes of tools/fixed_base_bench.py, g1_fixed_sum_bench.py, g2_fixed_sum_bench.py, fixed_g2_bench.py, bbs04_bench.py --tiled and bench.py):
  g1_mul_fixed 2^20 | g1_mul_fixed_sum 2^20, nb = 2 and 32 | pair_fixed_g2 2^16 | bbs04 verify, sign 2^18 (1024 distinct, tiled)
  | BBS+ verify 2^18 (one message block) | BBS+ verify from the wire formats 2^18 (16 h_i, 12-byte messages)
  | g2_mul_fixed 2^18 | g2_mul_fixed_sum 2^18, nb = 2 and 32 | PS verify 2^18, 8 messages (the sizes of g2_fixed_sum_bench.py)
  | PS sign and PS verify from the wire formats 2^18 (the sizes of tools/ps_bench.py: 32-byte messages, C12381_PS_MSG_ENCODE, nY = 3)

    python tools/host_tables_ab.py --trace [--legs a,b]      (under rocprofv3 --kernel-trace, one library per run)
makes one call of each leg after a warm-up call, between two marker launches (fp_mulchain_kernel, which no leg uses, on 256 (i + 1) threads
for leg i); tools/launch_compare.py cuts two such traces at the markers and compares the launches of every leg."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(trace=None):
    """trace: None = serve the legs named on stdin; a list = one traced call of each of these legs (all when empty)"""
    import numpy as np
    import torch
    torch.cuda.init()
    import tools.libsel  # noqa: F401  (C12381_LIB -> capi.use_library)
    from crypto12381_amd import Context
    from tools.bbs04_bench import MSG_LEN, make
    from tools.prof_driver import G1, G2, sc
    c = Context(0)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261018)
    d = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    rand = lambda nbytes: torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=dev, generator=gen)
    out = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    legs = {}

    n = 1 << 20
    base, k20, o20 = d(G1), rand(32 * n), out(96 * n)
    legs["g1_mul_fixed"] = (lambda: c.g1_mul_fixed_dev(n, base.data_ptr(), k20.data_ptr(), o20.data_ptr(), 96), o20)
    bases, k32 = d(c.g1_mul_fixed(G1, sc(61, 32), 96)), rand(32 * 32 * n)
    legs["g1_fixed_sum nb=2"] = (lambda: c.g1_mul_fixed_sum_dev(n, 2, bases.data_ptr(), k32.data_ptr(), o20.data_ptr(), None, 96), o20)
    legs["g1_fixed_sum nb=32"] = (lambda: c.g1_mul_fixed_sum_dev(n, 32, bases.data_ptr(), k32.data_ptr(), o20.data_ptr(), None, 96), o20)

    np_ = 1 << 16
    p16, q1, gt = d(c.g1_mul(G1 * 1024, sc(3, 1024), 96) * (np_ // 1024)), d(c.g2_mul(G2, sc(4, 1), 192)), out(576 * np_)
    legs["pair_fixed_g2"] = (lambda: c.pair_fixed_g2_dev(np_, p16.data_ptr(), q1.data_ptr(), gt.data_ptr()), gt)
    # the work-queue entries with per-element G2 arguments, the split forms and the GT power (3121 groups: 2081 whole, 1040 queued)
    q16 = d(c.g2_mul(G2 * 1024, sc(4, 1024), 192) * (np_ // 1024))
    gtp, mil, gtf, gtw, e16, ok16 = out(576 * np_), out(576 * np_), out(576 * np_), out(576 * np_), rand(32 * np_), out(np_)
    legs["pair"] = (lambda: c.pair_dev(np_, p16.data_ptr(), q16.data_ptr(), gtp.data_ptr()), gtp)
    legs["pair_eq"] = (lambda: c.pair_eq_dev(np_, p16.data_ptr(), q16.data_ptr(), p16.data_ptr(), q16.data_ptr(), ok16.data_ptr()), ok16)
    legs["miller"] = (lambda: c.miller_dev(np_, p16.data_ptr(), q16.data_ptr(), mil.data_ptr()), mil)
    legs["fexp"] = (lambda: c.gt_op_dev("fexp", np_, mil.data_ptr(), None, gtf.data_ptr()), gtf)                # of the Miller values the leg before left
    legs["gt_pow"] = (lambda: c.gt_op_dev("pow", np_, gtp.data_ptr(), e16.data_ptr(), gtw.data_ptr()), gtw)     # of the pairing values

    nb = 1 << 18
    gpk, gsk, msgs, rnd224, sig = make(c, 1024)
    d_gpk, d_gsk, d_msg, d_rnd, d_sig = (d(b) for b in (gpk, gsk * (nb // 1024), msgs * (nb // 1024), rnd224 * (nb // 1024), sig * (nb // 1024)))
    ok04, sig_out, st04 = out(nb), out(435 * nb), out(nb)
    legs["bbs04_verify"] = (lambda: c.bbs04_verify_dev(nb, MSG_LEN, d_gpk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), ok04.data_ptr()), ok04)
    legs["bbs04_sign"] = (lambda: c.bbs04_sign_dev(nb, MSG_LEN, d_gpk.data_ptr(), d_gsk.data_ptr(), d_msg.data_ptr(), d_rnd.data_ptr(), sig_out.data_ptr(),
                                                   st04.data_ptr()), sig_out)

    def red(seed, m):
        a = np.frombuffer(sc(seed, m), dtype=np.uint8).reshape(m, 32).copy()
        a[:, 0] &= 0x3f
        return a
    NH, RAW = 16, 12
    pub = c.g1_mul_fixed(G1, red(51, 2 + NH).tobytes(), 96)
    g1p, h0, h1, h_all = pub[:96], pub[96:192], pub[192:288], pub[192:]
    g2p = c.g2_mul_fixed(G2, red(52, 1).tobytes(), 192)
    gamma = red(53, 1).tobytes()
    w = c.g2_mul_fixed(g2p, gamma, 192)
    xs, rs = red(54, nb), red(55, nb)
    raw = np.random.Generator(np.random.PCG64(56)).integers(0, 256, size=(nb, RAW), dtype=np.uint8)

    def encode(r):                       # encode_to<Zp> of one unit: 0x01 || message || zero padding
        mm = np.zeros((nb, 32), dtype=np.uint8)
        mm[:, 0] = 1
        mm[:, 1:1 + RAW] = r
        return mm
    A = c.bbs_plus_sign(g1p, h0, h1, gamma, xs.tobytes(), rs.tobytes(), encode(raw).tobytes())
    raw[7::1009, RAW - 1] ^= 1
    dA, dx, dr, dm = d(A), d(xs.tobytes()), d(rs.tobytes()), d(encode(raw).tobytes())
    dpub = [d(b) for b in (g1p, g2p, h0, h1, w)]
    okb, okw = out(nb), out(nb)
    legs["bbs_plus_verify"] = (lambda: c.bbs_plus_verify_dev(nb, 1, dpub[0].data_ptr(), dpub[1].data_ptr(), dpub[2].data_ptr(), dpub[3].data_ptr(),
                                                             dpub[4].data_ptr(), dA.data_ptr(), dx.data_ptr(), dr.data_ptr(), dm.data_ptr(), okb.data_ptr()), okb)
    one = (1).to_bytes(32, "big")
    A49 = np.frombuffer(c.g1_mul(A, one * nb, 49), dtype=np.uint8).reshape(nb, 49)
    s145 = np.zeros((nb, 145), dtype=np.uint8)
    s145[:, 0:49], s145[:, 65:97], s145[:, 113:145] = A49, xs, rs
    dwire = [d(b) for b in (c.g1_mul(g1p, one, 49) + c.g2_mul(g2p, one, 97) + c.g1_mul(h0, one, 49), c.g1_mul(h_all, one * NH, 49), c.g2_mul(w, one, 97))]
    dsig, draw = d(s145.tobytes()), d(raw.tobytes())
    legs["bbs_plus_wire"] = (lambda: c.bbs_plus_verify_wire_dev(nb, NH, RAW, dwire[0].data_ptr(), dwire[1].data_ptr(), dwire[2].data_ptr(), dsig.data_ptr(),
                                                                draw.data_ptr(), okw.data_ptr()), okw)
    # the G2 legs at the sizes of tools/g2_fixed_sum_bench.py: 2^18 lanes; PS with 8 messages (1024 distinct signatures, tiled, every 7th with a wrong message)
    R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
    q2, kq, o2 = d(G2), rand(32 * 32 * nb), out(192 * nb)
    legs["g2_mul_fixed"] = (lambda: c.g2_mul_fixed_dev(nb, q2.data_ptr(), kq.data_ptr(), o2.data_ptr(), 192), o2)
    bases2 = d(c.g2_mul_fixed(G2, red(57, 32).tobytes(), 192))
    legs["g2_fixed_sum nb=2"] = (lambda: c.g2_mul_fixed_sum_dev(nb, 2, bases2.data_ptr(), kq.data_ptr(), o2.data_ptr(), None, 192), o2)
    legs["g2_fixed_sum nb=32"] = (lambda: c.g2_mul_fixed_sum_dev(nb, 32, bases2.data_ptr(), kq.data_ptr(), o2.data_ptr(), None, 192), o2)
    NM, DIST = 8, 1024
    b32 = lambda k: (k % R).to_bytes(32, "big")
    ints = lambda seed, m: [int.from_bytes(bytes(r), "big") % R for r in red(seed, m)]
    px, py = ints(58, 1)[0], ints(59, NM)
    X2, Y2 = c.g2_mul(G2, b32(px), 192), c.g2_mul(G2 * NM, b"".join(b32(v) for v in py), 192)
    pm = [ints(60 + i, DIST) for i in range(NM)]
    s1 = c.g1_mul(G1 * DIST, b"".join(b32(v or 1) for v in ints(70, DIST)), 96)
    s2 = c.g1_mul(s1, b"".join(b32(px + sum(py[i] * pm[i][j] for i in range(NM))) for j in range(DIST)), 96)
    for j in range(0, DIST, 7):
        pm[j % NM][j] = (pm[j % NM][j] + 1) % R
    tile = lambda b, w: np.tile(np.frombuffer(b, dtype=np.uint8).reshape(DIST, w), (nb // DIST, 1)).tobytes()
    dps = [d(G2), d(X2), d(Y2), d(tile(s1, 96)), d(tile(s2, 96)), d(b"".join(tile(b"".join(b32(v) for v in col), 32) for col in pm))]
    okp = out(nb)
    legs["ps_verify nmsg=8"] = (lambda: c.ps_verify_dev(nb, NM, *[v.data_ptr() for v in dps], okp.data_ptr()), okp)
    # PS from the wire formats at the sizes of tools/ps_bench.py; the key is (g2, x g2, y_i g2) on the generator, so every signature verifies
    from crypto12381_amd.capi import PS_MSG_ENCODE
    NY, ML = 3, 32
    kx, ky = ints(80, 1)[0], ints(81, NY)
    pk97 = (c.g2_mul(G2, b32(1), 97), c.g2_mul(G2, b32(kx), 97), c.g2_mul(G2 * NY, b"".join(b32(v) for v in ky), 97))
    dkey = [d(kx.to_bytes(48, "big")), d(b"".join(v.to_bytes(48, "big") for v in ky))] + [d(b) for b in pk97]
    dmsg, dt32, sig_ps, ok_ps = rand(ML * nb), rand(32 * nb), out(98 * nb), out(nb)
    legs["ps_sign"] = (lambda: c.ps_sign_dev(nb, NY, ML, PS_MSG_ENCODE, dkey[0].data_ptr(), dkey[1].data_ptr(), dmsg.data_ptr(), dt32.data_ptr(),
                                             sig_ps.data_ptr()), sig_ps)
    legs["ps_verify_wire"] = (lambda: c.ps_verify_wire_dev(nb, NY, ML, PS_MSG_ENCODE, dkey[2].data_ptr(), dkey[3].data_ptr(), dkey[4].data_ptr(),
                                                           sig_ps.data_ptr(), dmsg.data_ptr(), ok_ps.data_ptr()), ok_ps)      # on ps_sign's signatures
    torch.cuda.synchronize(dev)
    assert c.sync() == 0
    if trace is not None:
        mark = out(48 * 256 * (len(legs) + 1))
        for i, name in enumerate(legs):
            if trace and name not in trace:
                continue
            fn, res = legs[name]
            fn()
            assert c.sync() == 0
            marker = lambda: c.lib.c12381_fp_mulchain_dev(c.h, 256 * (i + 1), 0, mark.data_ptr(), mark.data_ptr(), mark.data_ptr())
            assert marker() == 0
            fn()
            assert marker() == 0 and c.sync() == 0
            print("TRACED %d %s %s" % (i, name.replace(" ", "_"), hashlib.sha256(res.cpu().numpy().tobytes()).hexdigest()[:16]), flush=True)
        c.close()
        return
    print("READY " + "|".join(legs), flush=True)
    for line in sys.stdin:
        name = line.strip()
        if name == "quit":
            break
        fn, res = legs[name]
        t0 = time.perf_counter()
        fn()
        rc = c.sync()
        dt = time.perf_counter() - t0
        print("T %.4f %d %s" % (dt * 1e3, rc, hashlib.sha256(res.cpu().numpy().tobytes()).hexdigest()[:16]), flush=True)
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace", action="store_true", help="one marked call of each leg after a warm-up call, for a kernel trace of this library")
    ap.add_argument("--legs", default="", help="with --trace: comma-separated leg names (default: all)")
    ap.add_argument("libs", nargs="*")
    a = ap.parse_args()
    if a.child or a.trace:
        child([x for x in a.legs.split(",") if x] if a.trace else None)
        return
    assert len(a.libs) == 2, "two libraries: A (the baseline) and B"
    kids = []
    for lib in a.libs:
        env = dict(os.environ)
        env.pop("C12381_LIB", None)
        if lib != "default":
            env["C12381_LIB"] = os.path.abspath(lib)
        kids.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], cwd=ROOT, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                     text=True, bufsize=1))

    def answer(k, tag):
        while True:
            line = k.stdout.readline()
            if not line:
                raise SystemExit("a child ended early (rc %s): nothing further is started" % k.poll())
            if line.startswith(tag):
                return line.split()[1:]
    names = [answer(k, "READY")[0:] for k in kids]
    legs = " ".join(names[0]).split("|")

    def call(k, leg):
        k.stdin.write(leg + "\n")
        k.stdin.flush()
        ms, rc, dig = answer(k, "T ")
        if int(rc) != 0:
            raise SystemExit("%s: status %s" % (leg, rc))
        return float(ms), dig
    lines = ["A = %s, B = %s; %d interleaved repeats per leg after one warm-up call each; wall ms per call (c12381_sync included)" % (a.libs[0], a.libs[1], a.reps),
             "%-20s %30s %30s   %s" % ("leg", "A median (min - max)", "B median (min - max)", "B median within A's spread / digests")]
    bad = False
    for leg in legs:
        digs = [call(k, leg)[1] for k in kids]                  # warm-up: tables built, workspaces grown
        t = [[], []]
        for _ in range(a.reps):
            for i, k in enumerate(kids):
                ms, dig = call(k, leg)
                t[i].append(ms)
                digs.append(dig)
        med = [statistics.median(x) for x in t]
        same = len(set(digs)) == 1
        bad |= not same
        inside = min(t[0]) <= med[1] <= max(t[0])
        verdict = "inside" if inside else ("OUTSIDE (B faster)" if med[1] < min(t[0]) else "OUTSIDE (B slower)")
        lines.append("%-20s %30s %30s   %s / %s" % (leg, "%.2f (%.2f - %.2f)" % (med[0], min(t[0]), max(t[0])), "%.2f (%.2f - %.2f)" % (med[1], min(t[1]), max(t[1])),
                                                   verdict, "equal" if same else "DIFFER"))
        print(lines[-1], flush=True)
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
