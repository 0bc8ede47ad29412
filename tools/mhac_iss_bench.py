#!/usr/bin/env python3
"""MHAC-bbs attribute generation, issuance, group and type of 2^18 credentials on one MI355X, for two shapes: the reference's examples/MHAC-bbs/test.cpp
(m = 4, Prv = (0, 2), Rev = (1), t = 3, 6 parties, S = (0, 2, 5)) and the same attributes with t = 8 of 8 parties:
  - c12381_mhac_bbs_{attr,iss,group,type}_batch in the _dev form (resident inputs) and the host form (staging included): the first call of a context
    and the median of the timed steps, separately;
  - A/B in the same process, interleaved step by step: the same outputs composed from the public entries that existed before (zp_op for the
    polynomials and the inverse, g1_mul_fixed_sum, g1_decompress, g1_mul_sum, g1_mul, g1_add) with the Lagrange coefficients and the gathers on the
    host, in host forms, on a context of its own so that neither route evicts the other's tables.  Output digests must be equal.
Each entry takes the outputs of the one before it; --distinct-log2n credentials' randomness is tiled to 2^log2n.  The report goes to --out (default
profiles/mhac_iss_bench.txt).

    python tools/mhac_iss_bench.py [--steps 5] [--warmup 1] [--log2n 18] [--distinct-log2n 12] [--out FILE]"""
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
from tools.mhac_bbs_bench import World  # noqa: E402

# m, Prv, Rev, t, nparties, S
SHAPES = [(4, (0, 2), (1,), 3, 6, (0, 2, 5)), (4, (0, 2), (1,), 8, 8, (7, 0, 1, 2, 3, 4, 5, 6))]
u8 = np.uint8
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def lagrange(xs):
    lam = [1] * len(xs)
    for k in range(len(xs)):
        for y in range(len(xs)):
            if y != k:
                lam[k] = lam[k] * (-xs[y] % R) * pow((xs[k] - xs[y]) % R, -1, R) % R
    return lam


def b32(a):
    return np.ascontiguousarray(a).tobytes()


def shares(c, a0, coeffs, nparties):
    """polynomial(k + 1, a0, coeffs) for k < nparties over n credentials, credential-major: (n nparties, 32) bytes, by Horner's rule on zp_op"""
    n = a0.shape[0]
    rep = lambda a: b32(np.repeat(a, nparties, axis=0))
    X = col(list(range(1, nparties + 1))) * n
    acc = None
    for a in reversed(coeffs):
        acc = rep(a) if acc is None else c.zp_op("add", acc, rep(a))
        acc = c.zp_op("mul", acc, X)
    return rep(a0) if acc is None else c.zp_op("add", acc, rep(a0))


def powers(c, cols96, lam, fmt):
    """prod_i cols96[i]^lam[i] per lane: multiplies of their own in products of at most 4 terms joined by additions"""
    n = len(cols96[0]) // 96
    acc = None
    for first in range(0, len(lam), 4):
        kk = min(4, len(lam) - first)
        last = first + kk == len(lam)
        part = c.g1_mul_sum(b"".join(cols96[first:first + kk]), b"".join(col([l]) * n for l in lam[first:first + kk]), kk, fmt if last and acc is None else 96)
        acc = part if acc is None else c.g1_add(acc, part, fmt if last else 96)
    return acc


def composed_attr(c, wd, sh, rnd):
    m, Prv, t, np_ = sh["m"], sh["Prv"], sh["t"], sh["np"]
    n, nP = rnd.shape[0], len(Prv)
    sc = [shares(c, rnd[:, Prv[ii]], [rnd[:, m + ii * (t - 1) + i] for i in range(t - 1)], np_) for ii in range(nP)]
    C = c.g1_mul_fixed_sum(wd.hs(Prv), b"".join(sc), None, 49)
    ashare = f48(np.stack([arr(s, 32) for s in sc], axis=1))                         # (n np, nPrv, 48)
    return f48(rnd[:, sh["Pub"]]).tobytes(), ashare.tobytes(), C


def composed_iss(c, wd, sh, C49, pub48, rnd):
    t, np_, Pub = sh["t"], sh["np"], sh["Pub"]
    n = rnd.shape[0]
    C96 = arr(c.g1_decompress(C49)[0], 96).reshape(n, np_, 96)
    T = powers(c, [b32(C96[:, i]) for i in range(t)], lagrange(list(range(1, t + 1))), 96)
    P = c.g1_mul_fixed_sum(wd.hs(Pub), base_major(arr(pub48, 48).reshape(n, len(Pub), 48)[:, :, 16:]), wd.g1, 96)
    C_a = c.g1_add(T, P, 96)
    e = b32(rnd[:, 0])
    A = c.g1_mul(C_a, c.zp_op("inv", c.zp_op("add", e, col([wd.gamma]) * n)), 96)
    es = shares(c, rnd[:, 0], [rnd[:, 1 + i] for i in range(t - 1)], np_)
    W = c.g1_mul(b32(np.repeat(arr(A, 96), np_, axis=0)), c.zp_op("neg", es), 96)
    D = c.g1_add(b32(C96), W, 49)
    return enc49(arr(A, 96)).tobytes(), f48(arr(es, 32)).tobytes(), D


def composed_group(c, sh, D49, es48, as48):
    t, np_, S, nP = sh["t"], sh["np"], list(sh["S"]), len(sh["Prv"])
    n = len(D49) // (49 * np_)
    lam = lagrange([i + 1 for i in S])
    sel = arr(D49, 49).reshape(n, np_, 49)[:, S]                                      # the gather of the rows of S, on the host
    D96 = arr(c.g1_decompress(b32(sel.transpose(1, 0, 2)))[0], 96).reshape(t, n, 96)
    Dg = powers(c, [b32(D96[k]) for k in range(t)], lam, 49)
    lam48 = np.tile(f48(arr(col(lam), 32)), (n, 1, 1))
    return lam48.tobytes(), Dg, b32(arr(es48, 48).reshape(n, np_, 48)[:, S]), b32(arr(as48, 48 * nP).reshape(n, np_, 48 * nP)[:, S])


def composed_type(c, wd, sh, pub48):
    Pub, Rev = sh["Pub"], sh["Rev"]
    n = len(pub48) // (48 * len(Pub))
    pa = arr(pub48, 48).reshape(n, len(Pub), 48)[:, :, 16:]
    rp, ph = [k for k, i in enumerate(Pub) if i in Rev], [k for k, i in enumerate(Pub) if i not in Rev]
    C_rev = c.g1_mul_fixed_sum(wd.hs([Pub[k] for k in rp]), base_major(pa[:, rp]), wd.g1, 96) if rp else wd.g1 * n
    C_pub = c.g1_add(C_rev, c.g1_mul_fixed_sum(wd.hs([Pub[k] for k in ph]), base_major(pa[:, ph]), None, 96), 96) if ph else C_rev
    return enc49(arr(C_rev, 96)).tobytes(), enc49(arr(C_pub, 96)).tobytes()


def run_shape(c, c2, args, m, Prv, Rev, t, np_, S):
    sh = dict(m=m, Prv=list(Prv), Rev=list(Rev), t=t, np=np_, S=S, Pub=[i for i in range(m) if i not in Prv])
    n, nd = 1 << args.log2n, 1 << min(args.log2n, args.distinct_log2n)
    nP, nPub = len(Prv), m - len(Prv)
    dev = torch.device("cuda", 0)
    wd = World(c2, m)
    tile = lambda a: np.tile(a, (n // nd,) + (1,) * (a.ndim - 1))
    rnd_a, rnd_i = tile(scalars(b"attr%d" % t, (nd, m + nP * (t - 1)))), tile(scalars(b"iss%d" % t, (nd, t)))
    sk = wd.gamma.to_bytes(48, "big")
    say("shape m = %d, Prv = %s, Rev = %s, t = %d, %d parties, S = %s: 2^%d credentials (%d distinct draws tiled)" % (m, tuple(Prv), tuple(Rev), t, np_, S, args.log2n, nd))
    d = lambda b: torch.frombuffer(bytearray(b) or bytearray(1), dtype=torch.uint8).to(dev)
    z = lambda k: torch.full((max(k, 1),), 7, dtype=torch.uint8, device=dev)
    ptr = lambda x: _p(x.data_ptr())
    tb = lambda x, k: bytes(x.cpu().numpy().tobytes())[:k]
    d_pp, d_h, d_sk, d_ra, d_ri = d(wd.pp), d(wd.h49), d(sk), d(rnd_a.tobytes()), d(rnd_i.tobytes())
    d_pub, d_ash, d_C = z(48 * nPub * n), z(48 * nP * np_ * n), z(49 * np_ * n)
    d_A, d_es, d_D, d_sti = z(49 * n), z(48 * np_ * n), z(49 * np_ * n), z(n)
    d_lam, d_Dg, d_eS, d_aS, d_stg = z(48 * t * n), z(49 * n), z(48 * t * n), z(48 * t * nP * n), z(n)
    d_crev, d_cpub, d_stt = z(49 * n), z(49 * n), z(n)
    torch.cuda.synchronize()
    (pa, _), (ra, nR), (ia, _), (sa, _) = Context._idx(Prv), Context._idx(Rev), Context._idx(sh["Pub"]), Context._idx(S)
    lib = c.lib

    def done(rc):
        assert rc == 0 and c.sync() == 0

    dev_legs = {
        "attr": lambda: done(lib.c12381_mhac_bbs_attr_batch_dev(c.h, n, m, t, np_, nP, pa, ptr(d_pp), ptr(d_h), ptr(d_ra), ptr(d_pub), ptr(d_ash), ptr(d_C))),
        "iss": lambda: done(lib.c12381_mhac_bbs_iss_batch_dev(c.h, n, m, t, np_, nPub, ia, ptr(d_pp), ptr(d_h), ptr(d_sk), ptr(d_C), ptr(d_pub), ptr(d_ri), ptr(d_A),
                                                             ptr(d_es), ptr(d_D), ptr(d_sti))),
        "group": lambda: done(lib.c12381_mhac_bbs_group_batch_dev(c.h, n, np_, t, sa, nP, ptr(d_D), ptr(d_es), ptr(d_ash), ptr(d_lam), ptr(d_Dg), ptr(d_eS), ptr(d_aS),
                                                                 ptr(d_stg))),
        "type": lambda: done(lib.c12381_mhac_bbs_type_batch_dev(c.h, n, m, nP, pa, nR, ra, ptr(d_pp), ptr(d_h), ptr(d_pub), ptr(d_crev), ptr(d_cpub), ptr(d_stt)))}

    def clock(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    first = {k + "_dev": clock(fn)[0] for k, fn in dev_legs.items()}
    assert tb(d_sti, n) == bytes(n) and tb(d_stg, n) == bytes(n) and tb(d_stt, n) == bytes(n), "a lane was refused"
    out = {"attr": (tb(d_pub, 48 * nPub * n), tb(d_ash, 48 * nP * np_ * n), tb(d_C, 49 * np_ * n)),
           "iss": (tb(d_A, 49 * n), tb(d_es, 48 * np_ * n), tb(d_D, 49 * np_ * n)),
           "group": (tb(d_lam, 48 * t * n), tb(d_Dg, 49 * n), tb(d_eS, 48 * t * n), tb(d_aS, 48 * t * nP * n)),
           "type": (tb(d_crev, 49 * n), tb(d_cpub, 49 * n))}
    pub48, ash48, C49 = out["attr"]
    _, es48, D49 = out["iss"]
    host_legs = {"attr": lambda: c.mhac_bbs_attr(wd.pp, wd.h49, Prv, t, np_, rnd_a.tobytes()),
                 "iss": lambda: c.mhac_bbs_iss(wd.pp, wd.h49, sk, sh["Pub"], t, np_, C49, pub48, rnd_i.tobytes())[:3],
                 "group": lambda: c.mhac_bbs_group(S, np_, nP, D49, es48, ash48)[:4],
                 "type": lambda: c.mhac_bbs_type(wd.pp, wd.h49, Prv, Rev, pub48)[:2]}
    comp_legs = {"attr": lambda: composed_attr(c2, wd, sh, rnd_a), "iss": lambda: composed_iss(c2, wd, sh, C49, pub48, rnd_i),
                 "group": lambda: composed_group(c2, sh, D49, es48, ash48), "type": lambda: composed_type(c2, wd, sh, pub48)}
    digest = lambda parts: hashlib.sha256(b"".join(parts)).hexdigest()[:12]
    legs = {}
    for k in dev_legs:
        first[k + "_composed"], got = clock(comp_legs[k])
        first[k + "_host"], hgot = clock(host_legs[k])
        say("digests %-5s _dev %s   host %s   composed %s" % (k, digest(out[k]), digest(hgot), digest(got)))
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
    say("2^%d credentials, warmup %d, steps %d, interleaved; first call / median (min, max) in ms" % (args.log2n, args.warmup, args.steps))
    for k in legs:
        say("  %-16s first %9.2f   median %9.2f (%9.2f, %9.2f)   %.3e /s" % (k, first[k] * 1e3, med[k] * 1e3, min(times[k]) * 1e3, max(times[k]) * 1e3, n / med[k]))
    for w in dev_legs:
        ratio_h, ratio_d = med[w + "_composed"] / med[w + "_host"], med[w + "_composed"] / med[w + "_dev"]
        say("%s: composed / one-call host form %.2fx (like for like: both stage from host memory), composed / _dev form %.2fx%s"
            % (w, ratio_h, ratio_d, "" if ratio_h > 1 else "   — the entry is NOT faster than its composition"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--distinct-log2n", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mhac_iss_bench.txt"))
    args = ap.parse_args()
    assert args.steps >= 5, "medians of at least 5 steps"
    say("python tools/mhac_iss_bench.py --steps %d --warmup %d --log2n %d --distinct-log2n %d" % (args.steps, args.warmup, args.log2n, args.distinct_log2n))
    c, c2 = Context(0), Context(0)
    for shape in SHAPES:
        run_shape(c, c2, args, *shape)
    try:
        say("device %s, shader clock reported after the timed legs: %d MHz" % (torch.cuda.get_device_name(0), torch.cuda.clock_rate(0)))
    except Exception as e:
        say("device %s, shader clock not available (%s)" % (torch.cuda.get_device_name(0), type(e).__name__))
    c.close(); c2.close()
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
