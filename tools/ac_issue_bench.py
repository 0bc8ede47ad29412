#!/usr/bin/env python3
"""AC-bbs, AC-rbbs and AC-rps credential issuance and AC-rps user_keygen of 2^18 credentials on one MI355X (nattr = 16 for bbs / rbbs, 4 for rps):
  - c12381_ac_{bbs,rbbs}_issue_batch, c12381_ac_rps_user_keygen_batch and c12381_ac_rps_issue_batch in the _dev form (resident inputs) and the host
    form (staging included): the first call of a context and the median of the timed steps, separately;
  - A/B in the same process, interleaved step by step: the same outputs composed from the public entries that existed before (zp_op for x + w, its
    inverse, the Horner sum and the power of y; g1_mul_fixed_sum, g1_mul, g1_mul_fixed, g1_decompress, g1_mul_sum, g2_mul_fixed_sum) with the
    interleaving of the records on the host, in host forms, on a context of its own so that neither route evicts the other's tables.  Output digests
    must be equal.
--distinct-log2n credentials' inputs are tiled to 2^log2n.  The report goes to --out (default profiles/ac_issue_bench.txt).

    python tools/ac_issue_bench.py [--steps 5] [--warmup 1] [--log2n 18] [--distinct-log2n 12] [--out FILE]"""
import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tools.libsel  # noqa: E402,F401  (C12381_LIB -> capi.use_library)
from crypto12381_amd import Context  # noqa: E402
from crypto12381_amd.capi import _p  # noqa: E402
from tools.ac_bbs_bench import R, arr, base_major, col, enc49, f48, scalars  # noqa: E402
from tools.prof_driver import G1, G2  # noqa: E402

NATTR_BBS, NATTR_RPS = 16, 4
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def b32(a):
    return np.ascontiguousarray(a).tobytes()


class Key:
    """g, tilde_g, tilde_X, x, y and the records issue reads: Y[0 .. nattr) (bbs: independent points; rbbs: g^(y^(k+1))), tilde_Y[0 .. nattr)"""

    def __init__(self, c, scheme, nattr):
        k = lambda t: int.from_bytes(hashlib.sha512(b"ac-issue key|" + scheme.encode() + t).digest(), "big") % R
        self.nattr, self.x, self.y = nattr, k(b"x"), k(b"y")
        self.g = c.g1_mul_fixed(G1, col([k(b"g")]), 96)
        tg = c.g2_mul(G2, col([k(b"tg")]), 192)
        ys = [k(b"Y%d" % i) for i in range(nattr)] if scheme == "bbs" else [pow(self.y, i + 1, R) for i in range(nattr)]
        self.Y = c.g1_mul_fixed(G1 if scheme == "bbs" else self.g, col(ys), 96)
        self.tY = c.g2_mul(tg * nattr, col([pow(self.y, i + 1, R) for i in range(nattr)]), 192)
        self.pk = c.g1_mul_fixed(self.g, col([1]), 49) + c.g2_mul(tg, col([1]), 97) + c.g2_mul(tg, col([self.x]), 97)
        self.Y49 = c.g1_mul(self.Y, col([1]) * nattr, 49) + (c.g1_mul(self.Y, col([1]) * nattr, 49) if scheme == "rbbs" else b"")
        self.tY97 = c.g2_mul(self.tY, col([1]) * nattr, 97) + c.g2_mul(tg, col([1]), 97)
        self.sk = self.x.to_bytes(48, "big") + (b"" if scheme == "bbs" else self.y.to_bytes(48, "big"))


def composed_bbs(c, key, a, w):
    n = a.shape[0]
    C = c.g1_mul_fixed_sum(key.Y, base_major(a), key.g, 96)
    inv = c.zp_op("inv", c.zp_op("add", b32(w), col([key.x]) * n))
    A = arr(c.g1_mul(C, inv, 49), 49)
    return np.concatenate([A, f48(w)], axis=1).tobytes()


def composed_keygen(c, key, usk):
    return f48(usk).tobytes(), c.g1_mul_fixed(key.g, b32(usk), 49)


def composed_rps(c, key, upk49, a, alpha):
    n, na = a.shape[0], key.nattr
    Y = col([key.y]) * n
    acc = None
    for i in reversed(range(na)):                                        # Horner: ((a_(n-1) y + a_(n-2)) y + .. + a_0) y
        acc = b32(a[:, i]) if acc is None else c.zp_op("add", acc, b32(a[:, i]))
        acc = c.zp_op("mul", acc, Y)
    e1 = c.zp_op("add", acc, col([key.x]) * n)
    e2 = c.zp_op("mul", b32(alpha), col([pow(key.y, na + 1, R)]) * n)
    h = c.g1_mul_fixed(key.g, b32(alpha), 96)
    Z = c.g1_decompress(upk49)[0]
    sigma = arr(c.g1_mul_sum(h + Z, e1 + e2, 2, 49), 49)
    tM = arr(c.g2_mul_fixed_sum(key.tY, base_major(a), None, 97), 97)
    return np.concatenate([enc49(arr(h, 96)), sigma, tM], axis=1).tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--distinct-log2n", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ac_issue_bench.txt"))
    args = ap.parse_args()
    assert args.steps >= 5, "medians of at least 5 steps"
    say("python tools/ac_issue_bench.py --steps %d --warmup %d --log2n %d --distinct-log2n %d" % (args.steps, args.warmup, args.log2n, args.distinct_log2n))
    c, c2 = Context(0), Context(0)
    n, nd = 1 << args.log2n, 1 << min(args.log2n, args.distinct_log2n)
    dev = torch.device("cuda", 0)
    tile = lambda x: np.tile(x, (n // nd,) + (1,) * (x.ndim - 1))
    d = lambda b: torch.frombuffer(bytearray(b) or bytearray(1), dtype=torch.uint8).to(dev)
    z = lambda k: torch.full((max(k, 1),), 7, dtype=torch.uint8, device=dev)
    ptr = lambda x: _p(x.data_ptr())
    tb = lambda x, k: bytes(x.cpu().numpy().tobytes())[:k]
    lib = c.lib

    def done(rc):
        assert rc == 0 and c.sync() == 0

    def clock(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    kb, kr, kp = Key(c2, "bbs", NATTR_BBS), Key(c2, "rbbs", NATTR_BBS), Key(c2, "rps", NATTR_RPS)
    a16, a4 = tile(scalars(b"attr16", (nd, NATTR_BBS))), tile(scalars(b"attr4", (nd, NATTR_RPS)))
    w, usk, alpha = (tile(scalars(t, (nd,))) for t in (b"w", b"usk", b"alpha"))
    attr16, attr4 = f48(a16).tobytes(), f48(a4).tobytes()
    say("2^%d credentials (%d distinct draws tiled); AC-bbs / AC-rbbs nattr = %d, AC-rps nattr = %d" % (args.log2n, nd, NATTR_BBS, NATTR_RPS))
    d_a16, d_a4, d_w, d_usk, d_alpha = d(attr16), d(attr4), d(b32(w)), d(b32(usk)), d(b32(alpha))
    dk = {k: (d(key.sk), d(key.pk), d(key.Y49), d(key.tY97)) for k, key in (("bbs", kb), ("rbbs", kr), ("rps", kp))}
    o_sb, o_sr, o_st, o_usk, o_upk, o_sp, o_stp = z(97 * n), z(97 * n), z(n), z(48 * n), z(49 * n), z(195 * n), z(n)
    torch.cuda.synchronize()

    def bbs_dev(scheme, out):
        sk, pk, Y, _ = dk[scheme]
        fn = getattr(lib, "c12381_ac_%s_issue_batch_dev" % scheme)
        return lambda: done(fn(c.h, n, NATTR_BBS, ptr(sk), ptr(pk), ptr(Y), ptr(d_a16), ptr(d_w), ptr(out), ptr(o_st)))

    sk, pk, _, tY = dk["rps"]
    dev_legs = {"bbs_issue": bbs_dev("bbs", o_sb), "rbbs_issue": bbs_dev("rbbs", o_sr),
                "rps_user_keygen": lambda: done(lib.c12381_ac_rps_user_keygen_batch_dev(c.h, n, ptr(pk), ptr(d_usk), ptr(o_usk), ptr(o_upk))),
                "rps_issue": lambda: done(lib.c12381_ac_rps_issue_batch_dev(c.h, n, NATTR_RPS, ptr(sk), ptr(pk), ptr(tY), ptr(o_upk), ptr(d_a4), ptr(d_alpha), ptr(o_sp),
                                                                            ptr(o_stp)))}
    first = {k + "_dev": clock(fn)[0] for k, fn in dev_legs.items()}
    assert tb(o_st, n) == bytes(n) and tb(o_stp, n) == bytes(n), "a lane was refused"
    out = {"bbs_issue": (tb(o_sb, 97 * n),), "rbbs_issue": (tb(o_sr, 97 * n),), "rps_user_keygen": (tb(o_usk, 48 * n), tb(o_upk, 49 * n)),
           "rps_issue": (tb(o_sp, 195 * n),)}
    upk49 = out["rps_user_keygen"][1]
    host_legs = {"bbs_issue": lambda: c.ac_bbs_issue(kb.sk, kb.pk, kb.Y49, attr16, b32(w))[:1],
                 "rbbs_issue": lambda: c.ac_rbbs_issue(kr.sk, kr.pk, kr.Y49, attr16, b32(w))[:1],
                 "rps_user_keygen": lambda: c.ac_rps_user_keygen(kp.pk, b32(usk)),
                 "rps_issue": lambda: c.ac_rps_issue(kp.sk, kp.pk, kp.tY97, upk49, attr4, b32(alpha))[:1]}
    comp_legs = {"bbs_issue": lambda: (composed_bbs(c2, kb, a16, w),), "rbbs_issue": lambda: (composed_bbs(c2, kr, a16, w),),
                 "rps_user_keygen": lambda: composed_keygen(c2, kp, usk), "rps_issue": lambda: (composed_rps(c2, kp, upk49, a4, alpha),)}
    digest = lambda parts: hashlib.sha256(b"".join(parts)).hexdigest()[:12]
    legs = {}
    for k in dev_legs:
        first[k + "_composed"], got = clock(comp_legs[k])
        first[k + "_host"], hgot = clock(host_legs[k])
        say("digests %-16s _dev %s   host %s   composed %s" % (k, digest(out[k]), digest(hgot), digest(got)))
        assert digest(got) == digest(out[k]) == digest(hgot), "%s: the routes disagree" % k
        legs[k + "_dev"], legs[k + "_host"], legs[k + "_composed"] = dev_legs[k], host_legs[k], comp_legs[k]
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    times = {k: [] for k in legs}
    for _ in range(args.steps):                              # interleaved: every route sees the same clocks and the same neighbours
        for k, fn in legs.items():
            times[k].append(clock(fn)[0])
    med = {k: statistics.median(v) for k, v in times.items()}
    say("warmup %d, steps %d, interleaved; first call / median (min, max) in ms" % (args.warmup, args.steps))
    for k in legs:
        say("  %-26s first %9.2f   median %9.2f (%9.2f, %9.2f)   %.3e /s" % (k, first[k] * 1e3, med[k] * 1e3, min(times[k]) * 1e3, max(times[k]) * 1e3, n / med[k]))
    for k in dev_legs:
        ratio_h, ratio_d = med[k + "_composed"] / med[k + "_host"], med[k + "_composed"] / med[k + "_dev"]
        say("%s: composed / one-call host form %.2fx (like for like: both stage from host memory), composed / _dev form %.2fx%s"
            % (k, ratio_h, ratio_d, "" if ratio_h > 1 else "   — the entry is NOT faster than its composition"))
    try:
        say("device %s, shader clock reported after the timed legs: %d MHz" % (torch.cuda.get_device_name(0), torch.cuda.clock_rate(0)))
    except Exception as e:
        say("device %s, shader clock not available (%s)" % (torch.cuda.get_device_name(0), type(e).__name__))
    c.close(); c2.close()
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
