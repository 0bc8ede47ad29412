#!/usr/bin/env python3
"""AC-rps redact, pres and verify of 2^18 credentials (nattr = 10, I = (0, 3); verify also at nattr = 16) on one MI355X:
  - c12381_ac_rps_redact_batch / _pres_batch / _verify_batch in the _dev form (resident inputs) and the host form (staging included): the
    first call of a context (tables built, workspaces allocated) and the median of the timed steps, separately;
  - A/B in the same process, interleaved step by step: the same caches, presentations and verdicts composed from the public entries that
    existed before (g1 / g2_decompress, g1 / g2_mul_fixed_sum, g2_mul_fixed, g1_mul_sum, g1_mul, g2_add, miller, pair_product_fixed_g2 with
    MILLER_ONLY, gt_op, fexp, gt_is_unity, zp_op / zp_from_hash, SHA3-512 by hashlib on the host), in host forms, on a context of its own so
    that neither route evicts the other's tables.  Outputs must be equal.
Credentials are issued on the device as issue.cpp makes them; --distinct-log2n of them are tiled to 2^log2n lanes.

    python tools/ac_rps_bench.py [--steps 5] [--warmup 1] [--log2n 18] [--distinct-log2n 12] [--out FILE]     (the report also goes to profiles/ac_rps_bench.txt, or FILE)"""
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
from tools.ac_bbs_bench import P, R, arr, base_major, col, enc49, f48, scalars, stream  # noqa: E402
from tools.prof_driver import G1, G2  # noqa: E402

I = (0, 3)
NI = len(I)
u8 = np.uint8
MILLER_ONLY = 2


def kept(nattr):
    """the k of [0, 2 nattr] the filter of pres.cpp keeps, each with its (ii, j) pairs"""
    Ip, J = list(I) + [nattr], [j for j in range(nattr) if j not in I]
    out = []
    for k in range(2 * nattr + 1):
        pairs = [(ii, k + ip - nattr - 1) for ii, ip in enumerate(Ip) if (k + ip - nattr - 1) in J]
        if pairs:
            out.append((k, pairs))
    return out


class Key:
    """keygen.cpp: Y[k] = g^(y^(k+1)) for k <= 2 n, tilde_Y[k] = tilde_g^(y^(k+1)) for k <= n"""

    def __init__(self, c, nattr):
        k = lambda t: int.from_bytes(hashlib.sha512(b"ac-rps key|" + t).digest(), "big") % R
        self.nattr = nattr
        self.g = c.g1_mul_fixed(G1, col([k(b"g")]), 96)
        self.tg = c.g2_mul(G2, col([k(b"tg")]), 192)
        self.x, self.y = k(b"x"), k(b"y")
        self.tX = c.g2_mul(self.tg, col([self.x]), 192)
        self.Y = c.g1_mul(self.g * (2 * nattr + 1), col([pow(self.y, i + 1, R) for i in range(2 * nattr + 1)]), 96)
        self.tY = c.g2_mul(self.tg * (nattr + 1), col([pow(self.y, i + 1, R) for i in range(nattr + 1)]), 192)
        one = col([1])
        self.pk = c.g1_mul(self.g, one, 49) + c.g2_mul(self.tg, one, 97) + c.g2_mul(self.tX, one, 97)
        self.Y49 = c.g1_mul(self.Y, one * (2 * nattr + 1), 49)
        self.tY97 = c.g2_mul(self.tY, one * (nattr + 1), 97)
        pick = lambda b, w, ks: b"".join(b[w * i:w * i + w] for i in ks)
        self.Y_fixed = pick(self.Y, 96, [nattr - i for i in I] + [0])
        self.Y_cross = pick(self.Y, 96, [k for k, _ in kept(nattr)])
        self.tY_I = pick(self.tY, 192, I)
        self.tY_n = pick(self.tY, 192, [nattr])


def column(a, j):
    return np.ascontiguousarray(a[:, j]).tobytes()


def make(c, key, nd):
    """nd credentials as user_keygen.cpp and issue.cpp make them: (attr (nd, nattr, 32), sig195 (nd, 195), z (nd, 32), rnd (nd, 3, 32))"""
    n = key.nattr
    a, z, alpha = scalars(b"pattr%d" % n, (nd, n)), scalars(b"pz", (nd,)), scalars(b"palpha", (nd,))
    h = c.g1_mul_fixed(key.g, alpha.tobytes(), 96)
    upk = c.g1_mul_fixed(key.g, z.tobytes(), 96)
    ym = col([key.x]) * nd
    for i in range(n):
        ym = c.zp_op("add", ym, c.zp_op("mul", column(a, i), col([pow(key.y, i + 1, R)]) * nd))
    ay = c.zp_op("mul", alpha.tobytes(), col([pow(key.y, n + 1, R)]) * nd)
    sigma = c.g1_mul_sum(h + upk, ym + ay, 2, 49)
    tM = c.g2_mul_fixed_sum(key.tY[:192 * n], base_major(a), None, 97)
    sig = np.concatenate([enc49(arr(h, 96)), arr(sigma, 49), arr(tM, 97)], axis=1)
    return a, sig, z, scalars(b"prnd", (nd, 3))


def g2_neg(q192):
    q = arr(q192, 192)
    out = q.copy()
    for j in range(q.shape[0]):
        for lo in (96, 144):
            v = int.from_bytes(q[j, lo:lo + 48].tobytes(), "big")
            out[j, lo:lo + 48] = np.frombuffer(((P - v) % P).to_bytes(48, "big"), dtype=u8)
    return out.tobytes()


def composed_redact(c, key, a, sig):
    t0 = time.perf_counter()
    tM, _ = c.g2_decompress(np.ascontiguousarray(sig[:, 98:]).tobytes())
    c.g1_decompress(np.ascontiguousarray(sig[:, :98]).reshape(-1, 49).tobytes())            # h, sigma: decoded though unused
    prod = c.g2_mul_fixed_sum(key.tY_I, base_major(a[:, list(I)]), None, 192)
    t1 = time.perf_counter()
    neg = g2_neg(prod)
    th = time.perf_counter() - t1
    return c.g2_add(tM, neg, 97), th


def q_columns(c, head, dis48, nattr):
    """q_k for k <= nI from the per-lane head (n, 195) and the disclosed fields (n, 48 nI): SHA3-512 on the host, reduction on the device"""
    t0 = time.perf_counter()
    idx = b"".join(i.to_bytes(8, "little") for i in I)
    rows = [head[j].tobytes() + idx + dis48[j].tobytes() for j in range(head.shape[0])]
    digests = [b"".join(hashlib.sha3_512(r + ip.to_bytes(8, "little")).digest() for r in rows) for ip in list(I) + [nattr]]
    th = time.perf_counter() - t0
    return [c.zp_from_hash(d) for d in digests], th


def composed_pres(c, key, a, sig, cache, z, rnd):
    n, nattr = sig.shape[0], key.nattr
    pts, _ = c.g1_decompress(np.ascontiguousarray(sig[:, :98]).reshape(n, 2, 49).transpose(1, 0, 2).tobytes())
    h, sigma = pts[:96 * n], pts[96 * n:]
    c.g2_decompress(np.ascontiguousarray(sig[:, 98:]).tobytes())                             # tilde_M: decoded though unused
    tH, _ = c.g2_decompress(cache.tobytes())
    r, t, rho = (column(rnd, k) for k in range(3))
    s1 = c.g1_mul(h, r, 96)
    s2 = c.g1_mul_sum(sigma + s1, r + t, 2, 49)
    CC = c.g1_mul(s1 + s1, z.tobytes() + rho, 49)
    ts = c.g2_add(c.g2_mul_fixed(key.tg, t, 192), tH, 97)
    e_s1 = enc49(arr(s1, 96))
    head = np.concatenate([e_s1, arr(s2, 49), arr(ts, 97)], axis=1)
    q, th = q_columns(c, head, f48(a[:, list(I)]).reshape(n, 48 * NI), nattr)
    sc = [c.zp_op("mul", t, qk) for qk in q]
    for k, pairs in kept(nattr):
        acc = None
        for ii, j in pairs:
            term = c.zp_op("mul", q[ii], column(a, j))
            acc = term if acc is None else c.zp_op("add", acc, term)
        sc.append(acc)
    s3 = c.g1_mul_fixed_sum(key.Y_fixed + key.Y_cross, b"".join(sc), None, 49)
    C49, C0_49 = arr(CC[:49 * n], 49), arr(CC[49 * n:], 49)
    t0 = time.perf_counter()
    digests = b"".join(hashlib.sha3_512(row.tobytes()).digest() for row in np.concatenate([e_s1, C49, C0_49], axis=1))
    th += time.perf_counter() - t0
    c0 = c.zp_from_hash(digests)
    s0 = c.zp_op("add", rho, c.zp_op("mul", c.zp_op("neg", c0), z.tobytes()))
    return np.concatenate([e_s1, arr(s2, 49), arr(s3, 49), C49, arr(ts, 97), f48(arr(c0, 32)), f48(arr(s0, 32))], axis=1).tobytes(), th


def composed_verify(c, key, pres, dis):
    """the points of these honest presentations are canonical, so their wire bytes are hashed"""
    n, nattr = pres.shape[0], key.nattr
    g2, _ = c.g2_decompress(key.pk[49:])
    Yf, _ = c.g1_decompress(b"".join(key.Y49[49 * k:49 * k + 49] for k in [nattr - i for i in I] + [0]))
    tYu, _ = c.g2_decompress(b"".join(key.tY97[97 * k:97 * k + 97] for k in list(I) + [nattr]))
    s1, s2, s3, C = (c.g1_decompress(np.ascontiguousarray(pres[:, 49 * k:49 * k + 49]).tobytes())[0] for k in range(4))
    ts, _ = c.g2_decompress(np.ascontiguousarray(pres[:, 196:293]).tobytes())
    c0, s0 = (np.ascontiguousarray(pres[:, 309 + 48 * k:341 + 48 * k]).tobytes() for k in range(2))
    C0 = arr(c.g1_mul_sum(s1 + C, s0 + c0, 2, 49), 49)
    t0 = time.perf_counter()
    digests = b"".join(hashlib.sha3_512(row.tobytes()).digest() for row in np.concatenate([pres[:, :49], pres[:, 147:196], C0], axis=1))
    th = time.perf_counter() - t0
    c0_ok = arr(c.zp_from_hash(digests), 32) == arr(c0, 32)
    q, th2 = q_columns(c, np.concatenate([pres[:, :98], pres[:, 196:293]], axis=1), dis, nattr)
    S = c.g1_mul_fixed_sum(Yf, b"".join(q), None, 96)
    aI = dis.reshape(n, NI, 48)[:, :, 16:]
    W = c.g2_add(c.g2_mul_fixed_sum(tYu[:192 * NI], base_major(aI), g2[192:], 192), ts, 192)
    left = c.gt_op("mul", c.miller(s1, W), c.pair_product_fixed_g2(C, tYu[192 * NI:], 1, MILLER_ONLY))
    fixed = c.pair_product_fixed_g2(s2 + s3, g2[:192], 1, MILLER_ONLY)
    eq1 = c.gt_is_unity(c.fexp(c.gt_op("mul", left, c.gt_op("conj", fixed[:576 * n]))))
    eq2 = c.gt_is_unity(c.fexp(c.gt_op("mul", fixed[576 * n:], c.gt_op("conj", c.miller(S, ts)))))
    ok = c0_ok.all(axis=1) & (np.frombuffer(eq1, dtype=u8) == 1) & (np.frombuffer(eq2, dtype=u8) == 1)
    return ok.astype(u8).tobytes(), th + th2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--distinct-log2n", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ac_rps_bench.txt"),
                    help="the report is also written to this file")
    args = ap.parse_args()
    assert args.steps >= 5, "medians of at least 5 steps"
    report = []

    def say(line):
        print(line, flush=True)
        report.append(line)
    n, nd = 1 << args.log2n, 1 << min(args.log2n, args.distinct_log2n)
    c, c2 = Context(0), Context(0)
    d = lambda x: torch.frombuffer(bytearray(x if isinstance(x, bytes) else x.tobytes()), dtype=torch.uint8).to("cuda")
    back = lambda t: bytes(t.cpu().numpy().tobytes())
    ptr = lambda *ts: [t.data_ptr() for t in ts]

    def clock(fn):
        t = time.perf_counter()
        out = fn()
        return time.perf_counter() - t, out
    legs, want, first, sizes = {}, {}, {}, {}
    for nattr, which in ((10, ("redact", "pres", "verify")), (16, ("verify",))):
        key = Key(c2, nattr)
        t0 = time.perf_counter()
        a, sig, z, rnd = (np.tile(x, (n // nd,) + (1,) * (x.ndim - 1)) for x in make(c2, key, nd))
        attr48, usk = f48(a), f48(z)
        say("issued %d distinct credentials on the device, tiled to 2^%d lanes: nattr %d, I = %s, %d + %d list positions (%.1f s)"
            % (nd, args.log2n, nattr, I, NI + 1, len(kept(nattr)), time.perf_counter() - t0))
        dis_b = np.ascontiguousarray(attr48[:, list(I)]).tobytes()
        d_pk, d_Y, d_tY, d_attr, d_sig, d_usk, d_rnd, d_dis = (d(x) for x in (key.pk, key.Y49, key.tY97, attr48, sig, usk, rnd, dis_b))
        d_cache, d_pres = torch.zeros(97 * n, dtype=torch.uint8, device="cuda"), torch.zeros(389 * n, dtype=torch.uint8, device="cuda")
        d_st, d_ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda"), torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        arr_idx = c._idx(I)[0]

        def redact_dev(p=ptr(d_tY, d_attr, d_sig, d_cache, d_st), nattr=nattr):
            c._ck(c.lib.c12381_ac_rps_redact_batch_dev(c.h, n, nattr, NI, arr_idx, *p))
            assert c.sync() == 0

        def pres_dev(p=ptr(d_pk, d_Y, d_attr, d_sig, d_cache, d_usk, d_rnd, d_pres, d_st), nattr=nattr):
            c._ck(c.lib.c12381_ac_rps_pres_batch_dev(c.h, n, nattr, NI, arr_idx, *p))
            assert c.sync() == 0

        def verify_dev(p=ptr(d_pk, d_Y, d_tY, d_pres, d_dis, d_ok), nattr=nattr):
            c._ck(c.lib.c12381_ac_rps_verify_batch_dev(c.h, n, nattr, NI, arr_idx, *p))
            assert c.sync() == 0
        tag = lambda w: "%s%d" % (w, nattr)
        t_redact = clock(redact_dev)[0]
        cache_b = back(d_cache)
        assert back(d_st) == bytes(n), "redact refused a lane"
        t_pres = clock(pres_dev)[0]
        pres_b = back(d_pres)
        assert back(d_st) == bytes(n), "pres refused a lane"
        t_verify = clock(verify_dev)[0]
        assert back(d_ok) == b"\x01" * n, "a lane was rejected"
        cache_np, pres_np, dis_np = arr(cache_b, 97), arr(pres_b, 389), arr(dis_b, 48 * NI)
        attr_b, sig_b, usk_b, rnd_b = (x.tobytes() for x in (attr48, sig, usk, rnd))
        all_legs = {
            "redact": (t_redact, redact_dev, lambda key=key, a=a, sig=sig: composed_redact(c2, key, a, sig),
                       lambda key=key, attr_b=attr_b, sig_b=sig_b: c.ac_rps_redact(key.tY97, I, attr_b, sig_b), cache_b, (cache_b, bytes(n))),
            "pres": (t_pres, pres_dev, lambda key=key, a=a, sig=sig, cache_np=cache_np, z=z, rnd=rnd: composed_pres(c2, key, a, sig, cache_np, z, rnd),
                     lambda key=key, attr_b=attr_b, sig_b=sig_b, cache_b=cache_b, usk_b=usk_b, rnd_b=rnd_b:
                     c.ac_rps_pres(key.pk, key.Y49, I, attr_b, sig_b, cache_b, usk_b, rnd_b), pres_b, (pres_b, bytes(n))),
            "verify": (t_verify, verify_dev, lambda key=key, pres_np=pres_np, dis_np=dis_np: composed_verify(c2, key, pres_np, dis_np),
                       lambda key=key, pres_b=pres_b, dis_b=dis_b: c.ac_rps_verify(key.pk, key.Y49, key.tY97, I, pres_b, dis_b), b"\x01" * n, b"\x01" * n)}
        for w in which:
            t1, f_dev, f_comp, f_host, w_comp, w_host = all_legs[w]
            first[tag(w) + "_dev"] = t1
            legs[tag(w) + "_dev"], legs[tag(w) + "_composed"], legs[tag(w) + "_host"] = f_dev, f_comp, f_host
            want[tag(w) + "_composed"], want[tag(w) + "_host"] = w_comp, w_host
            sizes[tag(w)] = hashlib.sha256(w_comp).hexdigest()[:12]
    for k, w in want.items():
        first[k], out = clock(legs[k])
        assert (out[0] if k.endswith("composed") else out) == w, "%s disagrees with the _dev form" % k
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    times = {k: [] for k in legs}
    hashing = {k: [] for k in legs if k.endswith("composed")}
    for _ in range(args.steps):                              # interleaved: every route sees the same clocks and the same neighbours
        for k, fn in legs.items():
            dt, out = clock(fn)
            times[k].append(dt)
            if k in hashing:
                hashing[k].append(out[-1])
    med = {k: statistics.median(v) for k, v in times.items()}
    say("outputs equal on every route: " + ", ".join("%s %s" % kv for kv in sizes.items()))
    say("2^%d credentials, warmup %d, steps %d, interleaved; first call / median (min, max) in ms" % (args.log2n, args.warmup, args.steps))
    for k in legs:
        extra = "   of which SHA3-512 (and negation) on the host %.1f" % (statistics.median(hashing[k]) * 1e3) if k in hashing else ""
        say("  %-18s first %9.2f   median %9.2f (%9.2f, %9.2f)   %.3e /s%s"
            % (k, first[k] * 1e3, med[k] * 1e3, min(times[k]) * 1e3, max(times[k]) * 1e3, n / med[k], extra))
    for w in sizes:
        say("%s: composed / one-call host form %.2fx (like for like: both stage from host memory), composed / _dev form %.2fx"
            % (w, med[w + "_composed"] / med[w + "_host"], med[w + "_composed"] / med[w + "_dev"]))
    try:
        say("device %s, shader clock reported after the timed legs: %d MHz" % (torch.cuda.get_device_name(0), torch.cuda.clock_rate(0)))
    except Exception as e:
        say("device %s, shader clock not available (%s)" % (torch.cuda.get_device_name(0), type(e).__name__))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(report) + "\n")
    c.close(); c2.close()


if __name__ == "__main__":
    main()
