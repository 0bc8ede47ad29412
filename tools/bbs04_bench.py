#!/usr/bin/env python3
"""bbs04 signing and verification of 2^18 distinct signatures (32-byte messages) on one MI355X:
  - c12381_bbs04_sign_batch_dev: warm-up and timed steps, median; its signatures are what the verify leg checks (all 1);
  - A/B: the same signatures composed as make() composed them before c12381_bbs04_sign_batch existed (fourteen host-form calls and a
    Python loop with hashlib), on the same keys, messages and randomness — the signature bytes must be equal;
  - c12381_bbs04_verify_batch_dev: warm-up and timed steps, median (--tiled: on 1024 distinct signatures tiled to 2^18, the inputs
    profiles/bbs04_bench.txt was measured with);
  - A/B: the same check composed from the public entries that existed before it (per-call g1_decompress, g1_mul, g1_mul_fixed, g1_add,
    pair_product_fixed_g2 with k = 2, GT bytes hashed on the host with hashlib, zp_from_hash) — the ok bytes must be equal;
  - SHA3-512 throughput of c12381_sha3_512_batch_dev on 2^18 x 1 KB;
  - a CPU figure: 256 signatures verified by the same composition over the compiled reference's primitives (Oracle("reference")) on ONE
    thread, where oracle/_ref exists.
Keys and signatures are made on the device by c12381_bbs04_issue_batch / c12381_bbs04_sign_batch, as key_gen / sign
(examples/bbs04/src/bbs.cpp) make them.

    python tools/bbs04_bench.py [--steps 10] [--warmup 2] [--tiled] [--compose-log2n 18]"""
import argparse
import hashlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tools.libsel  # noqa: E402,F401  (C12381_LIB -> capi.use_library)
from crypto12381_amd import Context  # noqa: E402
from tools.prof_driver import G1, G2  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
MSG_LEN = 32


def rnd(tag, i):
    return int.from_bytes(hashlib.sha512(b"bbs04 bench|%s|%d" % (tag.encode(), i)).digest(), "big") % R


def col(vals):
    return b"".join((v % R).to_bytes(32, "big") for v in vals)


def neg96(pts):
    out = bytearray(pts)
    for j in range(len(pts) // 96):
        p = pts[96 * j:96 * j + 96]
        if p != bytes(96):
            out[96 * j + 48:96 * j + 96] = ((P - int.from_bytes(p[48:], "big")) % P).to_bytes(48, "big")
    return bytes(out)


def keys(c):
    """gpk (390 B), the 96-byte / 192-byte public points and gamma"""
    g1 = c.g1_mul_fixed(G1, col([rnd("g1", 0)]), 96)
    h = c.g1_mul_fixed(G1, col([rnd("h", 0)]), 96)
    g2 = c.g2_mul(G2, col([rnd("g2", 0)]), 192)
    xi1, xi2, gamma = rnd("xi1", 0), rnd("xi2", 0), rnd("gamma", 0)
    u = c.g1_mul_fixed(h, col([pow(xi1, -1, R)]), 96)
    v = c.g1_mul_fixed(h, col([pow(xi2, -1, R)]), 96)
    w = c.g2_mul(g2, col([gamma]), 192)
    gpk = c.g1_mul_fixed(g1, col([1]), 49) + c.g2_mul(g2, col([1]), 97) + b"".join(c.g1_mul_fixed(p, col([1]), 49) for p in (h, u, v)) + c.g2_mul(w, col([1]), 97)
    return gpk, (g1, g2, h, u, v, w), gamma


def inputs(nd):
    """per signature: the member's x, the seven random scalars of sign (alpha, beta, r_alpha, r_beta, r_x, r_delta1, r_delta2), the message"""
    x = [rnd("x", i) for i in range(nd)]
    seven = [[rnd(t, i) for i in range(nd)] for t in ("a", "b", "ra", "rb", "rx", "rd1", "rd2")]
    msgs = [hashlib.sha256(b"msg|%d" % i).digest()[:MSG_LEN] for i in range(nd)]
    return x, seven, msgs


def make(c, nd):
    """gpk, nd member keys (97 B), messages, randomness (224 B) and the nd valid signatures (435 B) c12381_bbs04_sign_batch makes of them"""
    gpk, _, gamma = keys(c)
    x, seven, msgs = inputs(nd)
    gsk = c.bbs04_issue(gpk, col([gamma]), col(x))
    rnd224 = b"".join(col(s[i] for s in seven) for i in range(nd))
    sig, st = c.bbs04_sign(gpk, gsk, b"".join(msgs), rnd224, MSG_LEN)
    assert st == bytes(nd)
    return gpk, gsk, b"".join(msgs), rnd224, sig


def make_composed(c, nd):
    """gpk and nd valid signatures composed from the G1 / pairing entries with host hashing: what make() did before the signing entry existed;
    the seconds are those of the composition alone (host-form calls and the Python loop), without drawing the keys and the inputs"""
    gpk, (g1, g2, h, u, v, w), gamma = keys(c)
    x, (a, b, ra, rb, rx, rd1, rd2), msgs = inputs(nd)
    t0 = time.perf_counter()
    A = c.g1_mul_fixed(g1, col([pow((gamma + xi) % R, -1, R) for xi in x]), 96)
    T1, T2 = c.g1_mul_fixed(u, col(a), 96), c.g1_mul_fixed(v, col(b), 96)
    T3 = c.g1_add(A, c.g1_mul_fixed(h, col([p + q for p, q in zip(a, b)]), 96), 96)
    R1, R2 = c.g1_mul_fixed(u, col(ra), 49), c.g1_mul_fixed(v, col(rb), 49)
    P1 = c.g1_add(c.g1_mul(T3, col(rx), 96), c.g1_mul_fixed(h, col([-(p + q) for p, q in zip(rd1, rd2)]), 96), 96)
    P2 = c.g1_mul_fixed(h, col([-(p + q) for p, q in zip(ra, rb)]), 96)
    R3 = c.pair_product_fixed_g2(P1 + P2, g2 + w, 2)
    R4 = c.g1_add(c.g1_mul(T1, col(rx), 96), c.g1_mul_fixed(u, col([-d for d in rd1]), 96), 49)
    R5 = c.g1_add(c.g1_mul(T2, col(rx), 96), c.g1_mul_fixed(v, col([-d for d in rd2]), 96), 49)
    one = col([1] * nd)
    e1, e2, e3 = (c.g1_mul(T, one, 49) for T in (T1, T2, T3))
    sigs = []
    for j in range(nd):
        g = lambda s, k=49: s[k * j:k * j + k]
        tr = msgs[j] + g(e1) + g(e2) + g(e3) + g(R1) + g(R2) + g(R3, 576) + g(R4) + g(R5)
        cc = int.from_bytes(hashlib.sha3_512(tr).digest(), "big") % R
        cx = cc * x[j] % R
        f = [cc, ra[j] + cc * a[j], rb[j] + cc * b[j], rx[j] + cx, rd1[j] + a[j] * cx, rd2[j] + b[j] * cx]
        sigs.append(g(e1) + g(e2) + g(e3) + b"".join((v % R).to_bytes(48, "big") for v in f))
    return gpk, b"".join(sigs), time.perf_counter() - t0


def composed(c, gpk, sig, msgs, n):
    """verify from the public entries that existed before c12381_bbs04_verify_batch (host forms, host hashing)"""
    pub96, _ = c.g1_decompress(gpk[0:49] + gpk[146:195] + gpk[195:244] + gpk[244:293])
    g1, h, u, v = (pub96[96 * i:96 * i + 96] for i in range(4))
    g2w, _ = c.g2_decompress(gpk[49:146] + gpk[293:390])
    T49 = [b"".join(sig[435 * j + 49 * k:435 * j + 49 * k + 49] for j in range(n)) for k in range(3)]
    T = [c.g1_decompress(t)[0] for t in T49]
    f = [[int.from_bytes(sig[435 * j + 147 + 48 * i:435 * j + 195 + 48 * i], "big") for j in range(n)] for i in range(6)]
    cc, sa, sb, sx, d1, d2 = f
    mul, fix, add = (lambda p, k, fmt=96: c.g1_mul(p, col(k), fmt)), (lambda b, k, fmt=96: c.g1_mul_fixed(b, col(k), fmt)), c.g1_add
    negc = [-x for x in cc]
    R1 = add(fix(u, sa), mul(T[0], negc), 49)
    R2 = add(fix(v, sb), mul(T[1], negc), 49)
    P1 = add(add(mul(T[2], sx), fix(h, [-p - q for p, q in zip(d1, d2)]), 96), neg96(fix(g1, cc)), 96)
    P2 = add(fix(h, [-(p + q) for p, q in zip(sa, sb)]), mul(T[2], cc), 96)
    R3 = c.pair_product_fixed_g2(P1 + P2, g2w, 2)
    R4 = add(mul(T[0], sx), fix(u, [-d for d in d1]), 49)
    R5 = add(mul(T[1], sx), fix(v, [-d for d in d2]), 49)
    digests = b"".join(hashlib.sha3_512(msgs[MSG_LEN * j:MSG_LEN * j + MSG_LEN] + T49[0][49 * j:49 * j + 49] + T49[1][49 * j:49 * j + 49]
                                        + T49[2][49 * j:49 * j + 49] + R1[49 * j:49 * j + 49] + R2[49 * j:49 * j + 49] + R3[576 * j:576 * j + 576]
                                        + R4[49 * j:49 * j + 49] + R5[49 * j:49 * j + 49]).digest() for j in range(n))
    z = c.zp_from_hash(digests)
    return bytes(1 if z[32 * j:32 * j + 32] == cc[j].to_bytes(32, "big") else 0 for j in range(n))


def cpu_reference(gpk, sigs, msgs):
    """the same composition over the compiled reference's primitives, one thread, one signature at a time"""
    from oracle.bindings import Oracle, have_reference
    if not have_reference():
        return None
    o = Oracle("reference")
    b32 = lambda k: (k % R).to_bytes(32, "big")
    t0 = time.perf_counter()
    out = []
    for sig, msg in zip(sigs, msgs):
        pub = [o.g1_decompress(gpk[a:a + 49])[0] for a in (0, 146, 195, 244)]
        g1, h, u, v = pub
        g2 = o.g2_decompress(gpk[49:146])[0]
        w = o.g2_decompress(gpk[293:390])[0]
        T = [o.g1_decompress(sig[49 * k:49 * k + 49])[0] for k in range(3)]
        cc, sa, sb, sx, d1, d2 = (int.from_bytes(sig[147 + 48 * i:195 + 48 * i], "big") for i in range(6))
        m = lambda p, k: o.g1_mul(p, b32(k), 96)
        R1 = o.g1_add(m(u, sa), m(T[0], -cc), 49)
        R2 = o.g1_add(m(v, sb), m(T[1], -cc), 49)
        P1 = o.g1_add(o.g1_add(m(T[2], sx), m(h, -d1 - d2)), neg96(m(g1, cc)))
        P2 = o.g1_add(m(h, -(sa + sb)), m(T[2], cc))
        R3 = o.gt_op("mul", o.pair(P1, g2), o.pair(P2, w))
        R4 = o.g1_add(m(T[0], sx), m(u, -d1), 49)
        R5 = o.g1_add(m(T[1], sx), m(v, -d2), 49)
        tr = msg + sig[:147] + R1 + R2 + R3 + R4 + R5
        out.append(1 if int.from_bytes(hashlib.sha3_512(tr).digest(), "big") % R == cc else 0)
    return time.perf_counter() - t0, bytes(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--tiled", action="store_true", help="1024 distinct signatures tiled to 2^log2n, as before the signing entry existed")
    ap.add_argument("--compose-log2n", type=int, default=18, help="signatures the composed signing route makes for the A/B (at most the distinct ones)")
    args = ap.parse_args()
    c = Context(0)
    dev = torch.device("cuda", 0)
    n = 1 << args.log2n
    nd = 1024 if args.tiled else n
    d = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    t0 = time.perf_counter()
    gpk, gsk, msgs, rnd224, sig = make(c, nd)
    print("made %d distinct member keys and signatures on the device (c12381_bbs04_issue_batch, c12381_bbs04_sign_batch; inputs drawn in Python) in %.1f s"
          % (nd, time.perf_counter() - t0))
    gsk, msgs, rnd224, sig = (b * (n // nd) for b in (gsk, msgs, rnd224, sig))
    d_gpk, d_gsk, d_msg, d_rnd = d(gpk), d(gsk), d(msgs), d(rnd224)
    d_sig = torch.zeros(435 * n, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    d_ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def timed(run):
        for _ in range(args.warmup):
            run()
            assert c.sync() == 0
        times = []
        for _ in range(args.steps):
            t = time.perf_counter()
            run()
            assert c.sync() == 0
            times.append(time.perf_counter() - t)
        return statistics.median(times), times
    # ---- the signing leg
    smed, stimes = timed(lambda: c.bbs04_sign_dev(n, MSG_LEN, d_gpk.data_ptr(), d_gsk.data_ptr(), d_msg.data_ptr(), d_rnd.data_ptr(), d_sig.data_ptr(),
                                                  d_st.data_ptr()))
    assert bytes(d_st.cpu().numpy().tobytes()) == bytes(n), "a lane was rejected"
    assert bytes(d_sig.cpu().numpy().tobytes()) == sig, "the _dev form disagrees with the host form"
    print("c12381_bbs04_sign_batch_dev    2^%d signatures (%d distinct), msg_len %d: warmup %d, steps %d, median %.2f ms (min %.2f, max %.2f)  %.3e /s"
          % (args.log2n, nd, MSG_LEN, args.warmup, args.steps, smed * 1e3, min(stimes) * 1e3, max(stimes) * 1e3, n / smed))
    t = time.perf_counter()
    sig_host, _ = c.bbs04_sign(gpk, gsk, msgs, rnd224, MSG_LEN)
    dt_host = time.perf_counter() - t
    print("c12381_bbs04_sign_batch (host form, staging included): %.2f ms" % (dt_host * 1e3))
    assert sig_host == sig
    nc = min(nd, 1 << args.compose_log2n)
    gpk_c, sig_c, dt_sc = make_composed(c, nc)
    assert gpk_c == gpk and sig_c == sig[:435 * nc], "composed signatures disagree"
    digest = lambda b: hashlib.sha256(b).hexdigest()[:12]
    print("composed signing as make() did it before (host forms, hashlib and Zp arithmetic on the host; keys and inputs drawn outside the timing), "
          "2^%d signatures, same inputs: %.1f ms  %.3e /s   signature bytes equal: True (digest %s %s)   per signature %.2fx the fused host form "
          "(like for like: both stage from host memory), %.2fx the _dev form on resident inputs"
          % (nc.bit_length() - 1, dt_sc * 1e3, nc / dt_sc, digest(sig_c), digest(sig[:435 * nc]), (dt_sc / nc) / (dt_host / n), (dt_sc / nc) / (smed / n)))
    # ---- the verify leg, on the signatures just made
    run = lambda: c.bbs04_verify_dev(n, MSG_LEN, d_gpk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), d_ok.data_ptr())
    med, times = timed(run)
    ok = bytes(d_ok.cpu().numpy().tobytes())
    assert ok == b"\x01" * n, "a valid signature was rejected"
    print("c12381_bbs04_verify_batch_dev  2^%d signatures (%d distinct), msg_len %d: warmup %d, steps %d, median %.2f ms (min %.2f, max %.2f)  %.3e /s"
          % (args.log2n, nd, MSG_LEN, args.warmup, args.steps, med * 1e3, min(times) * 1e3, max(times) * 1e3, n / med))
    print("sign / verify in this run: %.2f / %.2f ms = %.3f" % (smed * 1e3, med * 1e3, smed / med))
    try:                                                   # the shader clock the driver reports right after the timed legs
        print("device %s, shader clock reported after the verify leg: %d MHz" % (torch.cuda.get_device_name(0), torch.cuda.clock_rate(0)))
    except Exception as e:
        print("device %s, shader clock not available (%s)" % (torch.cuda.get_device_name(0), type(e).__name__))
    t = time.perf_counter()
    ok_host = c.bbs04_verify(gpk, sig, msgs, MSG_LEN)
    print("c12381_bbs04_verify_batch (host form, staging included): %.2f ms" % ((time.perf_counter() - t) * 1e3))
    assert ok_host == ok
    t = time.perf_counter()
    ok_comp = composed(c, gpk, sig, msgs, n)
    dt_comp = time.perf_counter() - t
    assert ok_comp == ok, "composed path disagrees"
    print("composed from earlier public entries (host forms, hashlib on the host): %.1f ms  %.3e /s   ok bytes equal: True   speed-up %.1fx"
          % (dt_comp * 1e3, n / dt_comp, dt_comp / med))
    # SHA3 throughput
    ln = 1024
    d_m = torch.randint(0, 256, (n * ln,), dtype=torch.uint8, device=dev)
    d_o = torch.empty(64 * n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for _ in range(args.warmup):
        c.sha3_512_dev(n, ln, d_m.data_ptr(), d_o.data_ptr()); c.sync()
    st = []
    for _ in range(args.steps):
        t = time.perf_counter()
        c.sha3_512_dev(n, ln, d_m.data_ptr(), d_o.data_ptr()); c.sync()
        st.append(time.perf_counter() - t)
    sm = statistics.median(st)
    j = n // 3
    assert bytes(d_o[64 * j:64 * j + 64].cpu().numpy().tobytes()) == hashlib.sha3_512(bytes(d_m[ln * j:ln * j + ln].cpu().numpy().tobytes())).digest()
    print("c12381_sha3_512_batch_dev  2^%d x %d B: median %.3f ms  %.3e msgs/s  %.1f GB/s of input" % (args.log2n, ln, sm * 1e3, n / sm, n * ln / sm / 1e9))
    cpu = cpu_reference(gpk, [sig[435 * j:435 * j + 435] for j in range(256)], [msgs[MSG_LEN * j:MSG_LEN * j + MSG_LEN] for j in range(256)])
    if cpu is None:
        print("CPU reference: oracle/_ref not built here, skipped")
    else:
        dt, ok_cpu = cpu
        assert ok_cpu == b"\x01" * 256
        print("CPU, compiled reference primitives composed per signature, ONE thread, 256 signatures: %.1f ms  %.3e /s (%.3f ms per signature)"
              % (dt * 1e3, 256 / dt, dt / 256 * 1e3))
    c.close()


if __name__ == "__main__":
    main()
