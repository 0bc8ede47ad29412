#!/usr/bin/env python3
"""AC-rbbs redact, pres and verify of 2^18 credentials (nattr = 16, I = (0, 3), 32-byte messages) on one MI355X:
  - c12381_ac_rbbs_redact_batch / _pres_batch / _verify_batch in the _dev form (resident inputs) and the host form (staging included): the
    first call of a context (tables built, workspaces allocated) and the median of the timed steps, separately;
  - A/B in the same process, interleaved step by step: the same caches, presentations and verdicts composed from the public entries that
    existed before (g1_decompress, g1_mul_fixed_sum, g2_mul_fixed_sum, g1_mul_sum, g1_mul, g1_add, ps_verify with no messages, pair_eq, zp_op /
    zp_from_hash, SHA3-512 by hashlib on the host), in host forms, on a context of its own so that neither route evicts the other's tables.
    Outputs must be equal.
Credentials are issued on the device as issue.cpp makes them; --distinct-log2n of them are tiled to 2^log2n lanes.

    python tools/ac_rbbs_bench.py [--steps 5] [--warmup 1] [--log2n 18] [--distinct-log2n 12] [--out FILE]     (the report also goes to profiles/ac_rbbs_bench.txt, or FILE)"""
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

NATTR, I, MSG_LEN = 16, (0, 3), 32
J = [i for i in range(NATTR) if i not in I]
NI, NJ = len(I), len(J)
KD = sorted({NATTR - i + j for i in I for j in J})
u8 = np.uint8


class Key:
    """keygen.cpp: Y[k] = g^(y^(k+1)) except Y[n] = g, tilde_Y[k] = tilde_g^(y^(k+1))"""

    def __init__(self, c):
        k = lambda t: int.from_bytes(hashlib.sha512(b"ac-rbbs key|" + t).digest(), "big") % R
        self.g = c.g1_mul_fixed(G1, col([k(b"g")]), 96)
        self.tg = c.g2_mul(G2, col([k(b"tg")]), 192)
        self.x, y = k(b"x"), k(b"y")
        self.tX = c.g2_mul(self.tg, col([self.x]), 192)
        Y = c.g1_mul(self.g * (2 * NATTR), col([pow(y, i + 1, R) for i in range(2 * NATTR)]), 96)
        self.Y = Y[:96 * NATTR] + self.g + Y[96 * (NATTR + 1):]
        self.tY = c.g2_mul(self.tg * NATTR, col([pow(y, i + 1, R) for i in range(NATTR)]), 192)
        one = col([1])
        self.pk = c.g1_mul(self.g, one, 49) + c.g2_mul(self.tg, one, 97) + c.g2_mul(self.tX, one, 97)
        self.Y49 = c.g1_mul(self.Y, one * (2 * NATTR), 49)
        self.tY97 = c.g2_mul(self.tY, one * NATTR, 97)
        pick = lambda b, w, ks: b"".join(b[w * i:w * i + w] for i in ks)
        self.Y_I, self.Y_J, self.Y_K = pick(self.Y, 96, I), pick(self.Y, 96, J), pick(self.Y, 96, KD)
        self.tY_I = pick(self.tY, 192, [NATTR - 1 - i for i in I])


def make(c, key, nd):
    """nd credentials as issue.cpp makes them: (attr (nd, 16, 32), sig97 (nd, 97), msgs, rnd (nd, 3, 32))"""
    a = scalars(b"rattr", (nd, NATTR))
    w = scalars(b"rw", (nd,))
    C = c.g1_mul_fixed_sum(key.Y[:96 * NATTR], base_major(a), key.g, 96)
    inv = c.zp_op("inv", c.zp_op("add", w.tobytes(), col([key.x]) * nd))
    A = arr(c.g1_mul(C, inv, 49), 49)
    return a, np.concatenate([A, f48(w)], axis=1), stream(b"rmsg", (nd, MSG_LEN)), scalars(b"rrnd", (nd, 3))


def q_columns(c, aI48):
    """q_i for i in I from the disclosed fields (n, 48 nI): SHA3-512 on the host, reduction on the device -> ([nI] x bytes of n scalars, seconds)"""
    t0 = time.perf_counter()
    tails = [i.to_bytes(8, "little") for i in I]
    digests = [b"".join(hashlib.sha3_512(row.tobytes() + t).digest() for row in aI48) for t in tails]
    th = time.perf_counter() - t0
    return [c.zp_from_hash(d) for d in digests], th


def column(a, j):
    return np.ascontiguousarray(a[:, j]).tobytes()


def composed_redact(c, key, a, sig):
    q, th = q_columns(c, f48(a[:, list(I)]).reshape(a.shape[0], 48 * NI))
    C_I = c.g1_mul_fixed_sum(key.Y_I, base_major(a[:, list(I)]), key.g, 96)
    C_J = c.g1_mul_fixed_sum(key.Y_J, base_major(a[:, J]), None, 96)
    A, _ = c.g1_decompress(np.ascontiguousarray(sig[:, :49]).tobytes())
    B = c.g1_add(C_I, c.g1_mul(A, c.zp_op("neg", column(sig, slice(65, 97))), 96), 96)
    e = []
    for k in KD:
        acc = None
        for t, i in enumerate(I):
            j = k - NATTR + i
            if 0 <= j < NATTR and j not in I:
                term = c.zp_op("mul", q[t], column(a, j))
                acc = term if acc is None else c.zp_op("add", acc, term)
        e.append(acc)
    D = c.g1_mul_fixed_sum(key.Y_K, b"".join(e), None, 96)
    return np.concatenate([enc49(arr(p, 96)) for p in (C_I, C_J, B, D)], axis=1).tobytes(), th


def composed_pres(c, sig, cache, msgs, rnd):
    n = sig.shape[0]
    dec = lambda x: c.g1_decompress(np.ascontiguousarray(x).tobytes())[0]
    A, C_I, C_J, B, D = dec(sig[:, :49]), dec(cache[:, :49]), dec(cache[:, 49:98]), dec(cache[:, 98:147]), dec(cache[:, 147:])
    r, alpha, beta = (column(rnd, k) for k in range(3))
    four = c.g1_mul(A + B + C_J + D, r * 4, 96)
    A_ = four[:96 * n]
    U = c.g1_mul_sum(C_I + A_, alpha + beta, 2, 96)
    e = np.concatenate([enc49(arr(four, 96)).reshape(4, n, 49).transpose(1, 0, 2).reshape(n, 196), enc49(arr(U, 96))], axis=1)
    t0 = time.perf_counter()
    digests = b"".join(hashlib.sha3_512(row.tobytes()).digest() for row in np.concatenate([msgs, e], axis=1))
    th = time.perf_counter() - t0
    cc = c.zp_from_hash(digests)
    s = c.zp_op("add", alpha, c.zp_op("mul", r, cc))
    t = c.zp_op("add", beta, c.zp_op("mul", c.zp_op("neg", column(sig, slice(65, 97))), cc))
    return np.concatenate([e, f48(arr(s, 32)), f48(arr(t, 32))], axis=1).tobytes(), th


def composed_verify(c, key, pres, dis, msgs):
    """the points of these honest presentations are canonical, so their wire bytes are hashed"""
    n = pres.shape[0]
    g, _ = c.g1_decompress(key.pk[:49])
    Y_I, _ = c.g1_decompress(b"".join(key.Y49[49 * i:49 * i + 49] for i in I))
    g2, _ = c.g2_decompress(key.pk[49:])
    tY_I, _ = c.g2_decompress(b"".join(key.tY97[97 * (NATTR - 1 - i):97 * (NATTR - i)] for i in I))
    A_, B_, CJ_, D_ = (c.g1_decompress(np.ascontiguousarray(pres[:, 49 * k:49 * k + 49]).tobytes())[0] for k in range(4))
    aI = dis.reshape(n, NI, 48)[:, :, 16:]
    K = c.g1_mul_fixed_sum(Y_I, base_major(aI), g, 96)
    t0 = time.perf_counter()
    digests = b"".join(hashlib.sha3_512(row.tobytes()).digest() for row in np.concatenate([msgs, pres[:, :245]], axis=1))
    negB = b"".join(B_[96 * j:96 * j + 48] + (P - int.from_bytes(B_[96 * j + 48:96 * j + 96], "big")).to_bytes(48, "big") for j in range(n))
    th = time.perf_counter() - t0
    cc = c.zp_from_hash(digests)
    s, t = (np.ascontiguousarray(pres[:, 261 + 48 * k:293 + 48 * k]).tobytes() for k in range(2))
    got = arr(c.g1_mul_sum(K + A_ + negB, s + t + cc, 3, 49), 49)
    ok1 = np.frombuffer(c.ps_verify(g2[:192], g2[192:], b"", A_, c.g1_add(CJ_, B_, 96), b""), dtype=u8)
    q, th2 = q_columns(c, dis)
    W = c.g2_mul_fixed_sum(tY_I, b"".join(q), None, 192)
    ok3 = np.frombuffer(c.pair_eq(CJ_, W, D_, g2[:192] * n), dtype=u8)
    return ((ok1 == 1) & (ok3 == 1) & (got == pres[:, 196:245]).all(axis=1)).astype(u8).tobytes(), th + th2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--distinct-log2n", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ac_rbbs_bench.txt"),
                    help="the report is also written to this file")
    args = ap.parse_args()
    assert args.steps >= 5, "medians of at least 5 steps"
    report = []

    def say(line):
        print(line, flush=True)
        report.append(line)
    n, nd = 1 << args.log2n, 1 << min(args.log2n, args.distinct_log2n)
    c, c2 = Context(0), Context(0)
    dev = torch.device("cuda", 0)
    key = Key(c2)
    t0 = time.perf_counter()
    a, sig, msgs, rnd = (np.tile(x, (n // nd,) + (1,) * (x.ndim - 1)) for x in make(c2, key, nd))
    attr48 = f48(a)
    say("issued %d distinct credentials on the device, tiled to 2^%d lanes: nattr %d, I = %s, |K_D| = %d, msg_len %d (%.1f s)"
        % (nd, args.log2n, NATTR, I, len(KD), MSG_LEN, time.perf_counter() - t0))
    d = lambda x: torch.frombuffer(bytearray(x if isinstance(x, bytes) else x.tobytes()), dtype=torch.uint8).to(dev)
    dis_b = np.ascontiguousarray(attr48[:, list(I)]).tobytes()
    d_pk, d_Y, d_tY, d_attr, d_sig, d_msg, d_rnd, d_dis = d(key.pk), d(key.Y49), d(key.tY97), d(attr48), d(sig), d(msgs), d(rnd), d(dis_b)
    d_cache = torch.zeros(196 * n, dtype=torch.uint8, device=dev)
    d_pres = torch.zeros(341 * n, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    d_ok = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    attr_b, sig_b, msg_b, rnd_b = (x.tobytes() for x in (attr48, sig, msgs, rnd))
    back = lambda t: bytes(t.cpu().numpy().tobytes())

    def clock(fn):
        t = time.perf_counter()
        out = fn()
        return time.perf_counter() - t, out

    def redact_dev():
        c.ac_rbbs_redact_dev(n, NATTR, I, d_pk.data_ptr(), d_Y.data_ptr(), d_attr.data_ptr(), d_sig.data_ptr(), d_cache.data_ptr(), d_st.data_ptr())
        assert c.sync() == 0

    def pres_dev():
        c.ac_rbbs_pres_dev(n, MSG_LEN, d_sig.data_ptr(), d_cache.data_ptr(), d_msg.data_ptr(), d_rnd.data_ptr(), d_pres.data_ptr(), d_st.data_ptr())
        assert c.sync() == 0

    def verify_dev():
        c.ac_rbbs_verify_dev(n, NATTR, I, MSG_LEN, d_pk.data_ptr(), d_Y.data_ptr(), d_tY.data_ptr(), d_pres.data_ptr(), d_dis.data_ptr(), d_msg.data_ptr(),
                             d_ok.data_ptr())
        assert c.sync() == 0
    first = {"redact_dev": clock(redact_dev)[0]}
    cache_b = back(d_cache)
    assert back(d_st) == bytes(n), "redact refused a lane"
    first["pres_dev"] = clock(pres_dev)[0]
    pres_b = back(d_pres)
    assert back(d_st) == bytes(n), "pres refused a lane"
    first["verify_dev"] = clock(verify_dev)[0]
    assert back(d_ok) == b"\x01" * n, "a lane was rejected"
    cache_np, pres_np, dis_np = arr(cache_b, 196), arr(pres_b, 341), arr(dis_b, 48 * NI)
    legs = {"redact_dev": redact_dev, "redact_composed": lambda: composed_redact(c2, key, a, sig),
            "redact_host": lambda: c.ac_rbbs_redact(key.pk, key.Y49, I, attr_b, sig_b),
            "pres_dev": pres_dev, "pres_composed": lambda: composed_pres(c2, sig, cache_np, msgs, rnd),
            "pres_host": lambda: c.ac_rbbs_pres(sig_b, cache_b, msg_b, rnd_b, MSG_LEN),
            "verify_dev": verify_dev, "verify_composed": lambda: composed_verify(c2, key, pres_np, dis_np, msgs),
            "verify_host": lambda: c.ac_rbbs_verify(key.pk, key.Y49, key.tY97, I, pres_b, dis_b, msg_b, MSG_LEN)}
    want = {"redact_composed": cache_b, "pres_composed": pres_b, "verify_composed": b"\x01" * n, "redact_host": (cache_b, bytes(n)),
            "pres_host": (pres_b, bytes(n)), "verify_host": b"\x01" * n}
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
    digest = lambda b: hashlib.sha256(b).hexdigest()[:12]
    say("outputs equal on every route: cache %s, pres %s, ok %s" % (digest(cache_b), digest(pres_b), digest(b"\x01" * n)))
    say("2^%d credentials, warmup %d, steps %d, interleaved; first call / median (min, max) in ms" % (args.log2n, args.warmup, args.steps))
    for k in legs:
        extra = "   of which SHA3-512 (and negation) on the host %.1f" % (statistics.median(hashing[k]) * 1e3) if k in hashing else ""
        say("  %-16s first %9.2f   median %9.2f (%9.2f, %9.2f)   %.3e /s%s"
            % (k, first[k] * 1e3, med[k] * 1e3, min(times[k]) * 1e3, max(times[k]) * 1e3, n / med[k], extra))
    for w in ("redact", "pres", "verify"):
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
