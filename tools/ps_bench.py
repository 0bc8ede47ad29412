#!/usr/bin/env python3
"""PS signatures from the wire formats on one MI355X: 2^18 signatures, 32-byte messages, both message modes — C12381_PS_MSG_HASH with nY = 1
and C12381_PS_MSG_ENCODE with nY = 3 (a 32-byte message is two units, so nY = 1 cannot take it in that mode).  One INTERLEAVED run: every
step times the fused entry and then the route composed from the public entries that existed before it, on the same inputs, so both see the
same clocks and the spread of each is the spread of this run.
  - wire verify: c12381_ps_verify_wire_batch  vs  a host split of the signatures, c12381_g1_decompress_batch x 2, c12381_g2_decompress_batch,
    c12381_sha3_512_batch + c12381_zp_from_hash_batch (HASH) or the unit encoding on the host (ENCODE), c12381_ps_verify_batch;
  - sign: c12381_ps_sign_batch  vs  the same message scalars, c12381_zp_op_batch for e = x + sum y_i m_i and t e, c12381_g1_mul_fixed_batch
    x 2 on the generator and a host interleave of the two 49-byte columns;
  - aggregate: c12381_ps_verify_aggregate  vs  c12381_ps_verify_batch on the same decoded inputs.
All six are host forms (staging included) — like for like; the _dev forms on resident inputs are timed beside them.  The outputs of the two
routes must be equal; their digests are printed.

    python tools/ps_bench.py [--steps 5] [--warmup 1] [--log2n 18]"""
import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tools.libsel  # noqa: E402,F401  (C12381_LIB -> capi.use_library)
from crypto12381_amd import Context  # noqa: E402
from crypto12381_amd.capi import PS_MSG_ENCODE, PS_MSG_HASH  # noqa: E402
from tools.prof_driver import G1, G2  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
MSG_LEN = 32


def rnd(tag, i):
    return int.from_bytes(hashlib.sha512(b"ps bench|%s|%d" % (tag.encode(), i)).digest(), "big") % R


def col(vals):
    return b"".join((v % R).to_bytes(32, "big") for v in vals)


def digest(b):
    return hashlib.sha256(b).hexdigest()[:12]


def message_scalars(c, mode, msgs, n):
    """message-major 32-byte scalars from the public entries: SHA3-512 + Zp from_hash, or the units of encode_to<Zp> laid out on the host"""
    if mode == PS_MSG_HASH:
        return c.zp_from_hash(c.sha3_512(msgs, n, MSG_LEN)), 1
    units = (MSG_LEN + 30) // 31
    a = np.frombuffer(msgs, dtype=np.uint8).reshape(n, MSG_LEN)
    m = np.zeros((units, n, 32), dtype=np.uint8)
    m[:, :, 0] = 1
    for i in range(units):
        part = a[:, 31 * i:31 * i + 31]
        m[i, :, 1:1 + part.shape[1]] = part
    return m.tobytes(), units


def composed_verify(c, mode, pk97, sig, msgs, n):
    g2_97, X2_97, Y2_97 = pk97
    s = np.frombuffer(sig, dtype=np.uint8).reshape(n, 98)
    s1, _ = c.g1_decompress(s[:, :49].tobytes())
    s2, _ = c.g1_decompress(s[:, 49:].tobytes())
    m, units = message_scalars(c, mode, msgs, n)
    pub, _ = c.g2_decompress(g2_97 + X2_97 + Y2_97[:97 * units])
    return c.ps_verify(pub[:192], pub[192:384], pub[384:], s1, s2, m)


def composed_sign(c, mode, x, y, msgs, t32, n):
    m, units = message_scalars(c, mode, msgs, n)
    e = col([x]) * n
    for i in range(units):
        e = c.zp_op("add", e, c.zp_op("mul", col([y[i]]) * n, m[32 * n * i:32 * n * (i + 1)]))
    s1 = np.frombuffer(c.g1_mul_fixed(G1, t32, 49), dtype=np.uint8).reshape(n, 49)
    s2 = np.frombuffer(c.g1_mul_fixed(G1, c.zp_op("mul", t32, e), 49), dtype=np.uint8).reshape(n, 49)
    return np.concatenate([s1, s2], axis=1).tobytes()


def interleaved(steps, warmup, fused, composed):
    """each step: fused, then composed; returns (fused times, composed times, last outputs)"""
    tf, tc, a, b = [], [], None, None
    for s in range(warmup + steps):
        t = time.perf_counter(); a = fused(); d1 = time.perf_counter() - t
        t = time.perf_counter(); b = composed(); d2 = time.perf_counter() - t
        if s >= warmup:
            tf.append(d1); tc.append(d2)
    return tf, tc, a, b


def report(name, n, tf, tc, equal, da, db):
    f, cmed = statistics.median(tf), statistics.median(tc)
    print("%-34s fused %8.2f ms (min %.2f, max %.2f)   composed %8.2f ms (min %.2f, max %.2f)   composed / fused %.2fx   outputs equal: %s (digest %s %s)   %.3e /s fused"
          % (name, f * 1e3, min(tf) * 1e3, max(tf) * 1e3, cmed * 1e3, min(tc) * 1e3, max(tc) * 1e3, cmed / f, equal, da, db, n / f))
    assert equal, name


def dev_time(c, steps, warmup, run):
    ts = []
    for s in range(warmup + steps):
        t = time.perf_counter()
        run()
        assert c.sync() == 0
        if s >= warmup:
            ts.append(time.perf_counter() - t)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log2n", type=int, default=18)
    args = ap.parse_args()
    c = Context(0)
    dev = torch.device("cuda", 0)
    n = 1 << args.log2n
    d = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    msgs = b"".join(hashlib.sha256(b"ps msg|%d" % i).digest()[:MSG_LEN] for i in range(n))
    t32 = b"".join(hashlib.sha256(b"ps t|%d" % i).digest() for i in range(n))
    rho = b"".join(bytes(16) + hashlib.sha256(b"ps rho|%d" % i).digest()[:16] for i in range(n))
    print("# tools/ps_bench.py --steps %d --warmup %d --log2n %d: %d signatures, msg_len %d, host forms unless a line says _dev; %s"
          % (args.steps, args.warmup, args.log2n, n, MSG_LEN, torch.cuda.get_device_name(0)))
    for mode, nY, label in ((PS_MSG_HASH, 1, "HASH nY=1"), (PS_MSG_ENCODE, 3, "ENCODE nY=3")):
        x, y = rnd("x", nY), [rnd("y%d" % i, nY) for i in range(nY)]
        g2 = c.g2_mul(G2, col([rnd("g2", nY)]), 192)
        X2 = c.g2_mul(g2, col([x]), 192)
        Y2 = b"".join(c.g2_mul(g2, col([v]), 192) for v in y)
        one = col([1])
        pk97 = (c.g2_mul(g2, one, 97), c.g2_mul(X2, one, 97), b"".join(c.g2_mul(Y2[192 * i:192 * i + 192], one, 97) for i in range(nY)))
        x48, y48 = x.to_bytes(48, "big"), b"".join(v.to_bytes(48, "big") for v in y)
        # ---- sign
        tf, tc, sig, sig_c = interleaved(args.steps, args.warmup, lambda: c.ps_sign(x48, y48, msgs, t32, MSG_LEN, mode),
                                         lambda: composed_sign(c, mode, x, y, msgs, t32, n))
        report("sign %s" % label, n, tf, tc, sig == sig_c, digest(sig), digest(sig_c))
        # ---- wire verify, on the signatures just made
        tf, tc, ok, ok_c = interleaved(args.steps, args.warmup, lambda: c.ps_verify_wire(pk97[0], pk97[1], pk97[2], sig, msgs, MSG_LEN, mode),
                                       lambda: composed_verify(c, mode, pk97, sig, msgs, n))
        assert ok == b"\x01" * n, "a valid signature was rejected"
        report("wire verify %s" % label, n, tf, tc, ok == ok_c, digest(ok), digest(ok_c))
        # ---- aggregate against the per-signature entry, decoded inputs
        s = np.frombuffer(sig, dtype=np.uint8).reshape(n, 98)
        s1, _ = c.g1_decompress(s[:, :49].tobytes())
        s2, _ = c.g1_decompress(s[:, 49:].tobytes())
        m, units = message_scalars(c, mode, msgs, n)
        Yu = Y2[:192 * units]
        tf, tc, agg, okb = interleaved(args.steps, args.warmup, lambda: c.ps_verify_aggregate(g2, X2, Yu, s1, s2, m, rho),
                                       lambda: c.ps_verify(g2, X2, Yu, s1, s2, m))
        report("aggregate %s (%d units)" % (label, units), n, tf, tc, agg == (okb == b"\x01" * n), str(agg), digest(okb))
        # ---- the _dev forms on resident inputs
        dt = [d(b) for b in (x48, y48, msgs, t32, pk97[0], pk97[1], pk97[2], sig, g2, X2, Yu, s1, s2, m, rho)]
        p = [v.data_ptr() for v in dt]
        o_sig = torch.zeros(98 * n, dtype=torch.uint8, device=dev)
        o_ok = torch.zeros(n, dtype=torch.uint8, device=dev)
        o_all = torch.zeros(1, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        for name, run in (("c12381_ps_sign_batch_dev", lambda: c.ps_sign_dev(n, nY, MSG_LEN, mode, p[0], p[1], p[2], p[3], o_sig.data_ptr())),
                          ("c12381_ps_verify_wire_batch_dev", lambda: c.ps_verify_wire_dev(n, nY, MSG_LEN, mode, p[4], p[5], p[6], p[7], p[2], o_ok.data_ptr())),
                          ("c12381_ps_verify_batch_dev", lambda: c.ps_verify_dev(n, units, p[8], p[9], p[10], p[11], p[12], p[13], o_ok.data_ptr())),
                          ("c12381_ps_verify_aggregate_dev", lambda: c.ps_verify_aggregate_dev(n, units, p[8], p[9], p[10], p[11], p[12], p[13], p[14],
                                                                                                o_all.data_ptr()))):
            med, ts = dev_time(c, args.steps, args.warmup, run)
            print("  %-34s %s: median %.2f ms (min %.2f, max %.2f)  %.3e /s" % (name, label, med * 1e3, min(ts) * 1e3, max(ts) * 1e3, n / med))
        assert bytes(o_sig.cpu().numpy().tobytes()) == sig and bytes(o_ok.cpu().numpy().tobytes()) == ok and bytes(o_all.cpu().numpy().tobytes()) == b"\x01"
    # ---- randomise (no composed counterpart is asked for: two c12381_g1_mul_batch calls around a host split)
    tf, tc, out, out_c = interleaved(args.steps, args.warmup, lambda: c.ps_randomize(sig, t32)[0], lambda: composed_randomize(c, sig, t32, n))
    report("randomise", n, tf, tc, out == out_c, digest(out), digest(out_c))
    c.close()


def composed_randomize(c, sig, r32, n):
    s = np.frombuffer(sig, dtype=np.uint8).reshape(n, 98)
    o1 = np.frombuffer(c.g1_mul(c.g1_decompress(s[:, :49].tobytes())[0], r32, 49), dtype=np.uint8).reshape(n, 49)
    o2 = np.frombuffer(c.g1_mul(c.g1_decompress(s[:, 49:].tobytes())[0], r32, 49), dtype=np.uint8).reshape(n, 49)
    return np.concatenate([o1, o2], axis=1).tobytes()


if __name__ == "__main__":
    main()
