#!/usr/bin/env python3
"""AC-bbs presentation and verification of 2^18 presentations (nattr = 32, I = (0, 3), 32-byte messages: the shape of the reference's
examples/AC-bbs/test.cpp) on one MI355X:
  - c12381_ac_bbs_pres_batch / c12381_ac_bbs_verify_batch in the _dev form (resident inputs) and the host form (staging included): the first
    call of a context (tables built, workspaces allocated) and the median of the timed steps, separately;
  - A/B in the same process, interleaved step by step: the same presentations and verdicts composed from the public entries that existed
    before (g1_decompress, g1_mul_fixed_sum, g1_mul_sum, g1_mul, g1_add, ps_verify with no messages, zp_op / zp_from_hash, SHA3-512 by hashlib on
    the host), in host forms, on a context of its own so that neither route evicts the other's tables.  Output digests must be equal.
Credentials are issued on the device as issue.cpp makes them; --distinct-log2n of them are tiled to 2^log2n lanes (every lane runs the same
kernels whatever its values; the default keeps the set-up short).

    python tools/ac_bbs_bench.py [--steps 5] [--warmup 1] [--log2n 18] [--distinct-log2n 12]"""
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
from tools.prof_driver import G1, G2  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
NATTR, I, MSG_LEN = 32, (0, 3), 32
J = [i for i in range(NATTR) if i not in I]
NI, NJ = len(I), len(J)
ORDER = list(I) + J
u8 = np.uint8


def stream(tag, shape):
    """deterministic bytes; callers clear the top byte of a 32-byte scalar so that it is a residue"""
    return np.frombuffer(hashlib.shake_256(b"ac-bbs bench|" + tag).digest(int(np.prod(shape))), dtype=u8).reshape(shape).copy()


def scalars(tag, shape):
    s = stream(tag, tuple(shape) + (32,))
    s[..., 0] = 0
    return s


def col(vals):
    return b"".join((v % R).to_bytes(32, "big") for v in vals)


def base_major(a):
    """(n, k, 32) lane-major scalars -> bytes of the k columns"""
    return np.ascontiguousarray(a.transpose(1, 0, 2)).tobytes()


def f48(a32):
    """(..., 32) scalars -> (..., 48) serialize(Zp) fields"""
    out = np.zeros(a32.shape[:-1] + (48,), dtype=u8)
    out[..., 16:] = a32
    return out


def enc49(p96):
    """(n, 96) affine points other than infinity -> (n, 49) compressed"""
    out = np.empty((p96.shape[0], 49), dtype=u8)
    out[:, 0] = 2 | (p96[:, 95] & 1)
    out[:, 1:] = p96[:, :48]
    return out


def arr(b, width):
    return np.frombuffer(b, dtype=u8).reshape(-1, width)


class Key:
    def __init__(self, c):
        k = lambda t: int.from_bytes(hashlib.sha512(b"ac-bbs key|" + t).digest(), "big") % R
        self.g = c.g1_mul_fixed(G1, col([k(b"g")]), 96)
        self.tg = c.g2_mul(G2, col([k(b"tg")]), 192)
        self.x = k(b"x")
        self.tX = c.g2_mul(self.tg, col([self.x]), 192)
        self.Y = c.g1_mul_fixed(G1, col([k(b"Y%d" % i) for i in range(NATTR)]), 96)
        one = col([1])
        self.pk = c.g1_mul(self.g, one, 49) + c.g2_mul(self.tg, one, 97) + c.g2_mul(self.tX, one, 97)
        self.Y49 = c.g1_mul(self.Y, one * NATTR, 49)
        self.Y_I = b"".join(self.Y[96 * i:96 * i + 96] for i in I)
        self.Y_J = b"".join(self.Y[96 * j:96 * j + 96] for j in J)


def make(c, key, nd):
    """nd credentials as issue.cpp makes them, their messages and the randomness of pres: (attr (nd, 32, 32), sig97 (nd, 97), msgs, rnd (nd, 33, 32))"""
    a = scalars(b"attr", (nd, NATTR))
    w = scalars(b"w", (nd,))
    C = c.g1_mul_fixed_sum(key.Y, base_major(a), key.g, 96)
    inv = c.zp_op("inv", c.zp_op("add", w.tobytes(), col([key.x]) * nd))
    A = arr(c.g1_mul(C, inv, 49), 49)
    return a, np.concatenate([A, f48(w)], axis=1), stream(b"msg", (nd, MSG_LEN)), scalars(b"rnd", (nd, 3 + NJ))


def hash_rows(msgs, e147):
    rows = np.concatenate([msgs, e147], axis=1)
    return b"".join(hashlib.sha3_512(r.tobytes()).digest() for r in rows)


def composed_pres(c, key, a, sig, msgs, rnd):
    """pres from the entries that existed before: returns (pres_243, u_48) bytes and the seconds spent hashing on the host"""
    n = a.shape[0]
    cols = a[:, ORDER, :]
    C_I = c.g1_mul_fixed_sum(key.Y_I, base_major(cols[:, :NI]), key.g, 96)
    C_J = c.g1_mul_fixed_sum(key.Y_J, base_major(cols[:, NI:]), None, 96)
    C = c.g1_add(C_I, C_J, 96)
    A, _ = c.g1_decompress(np.ascontiguousarray(sig[:, :49]).tobytes())
    r, alpha, beta = (np.ascontiguousarray(rnd[:, k]).tobytes() for k in range(3))
    delta = rnd[:, 3:]
    negw = c.zp_op("neg", np.ascontiguousarray(sig[:, 65:]).tobytes())
    A_ = c.g1_mul(A, r, 96)
    B_ = c.g1_mul_sum(C + A_, r + negw, 2, 96)
    U = c.g1_add(c.g1_mul_sum(C_I + A_, alpha + beta, 2, 96), c.g1_mul_fixed_sum(key.Y_J, base_major(delta), None, 96), 96)
    e = np.concatenate([enc49(arr(p, 96)) for p in (A_, B_, U)], axis=1)
    t0 = time.perf_counter()
    digests = hash_rows(msgs, e)
    th = time.perf_counter() - t0
    cc = c.zp_from_hash(digests)
    rc = c.zp_op("mul", r, cc)
    s = c.zp_op("add", alpha, rc)
    t = c.zp_op("add", beta, c.zp_op("mul", negw, cc))
    u = c.zp_op("add", base_major(delta), c.zp_op("mul", rc * NJ, base_major(cols[:, NI:])))
    u = np.frombuffer(u, dtype=u8).reshape(NJ, n, 32).transpose(1, 0, 2)
    pres = np.concatenate([e, f48(arr(s, 32)), f48(arr(t, 32))], axis=1)
    return pres.tobytes(), f48(u).tobytes(), th


def composed_verify(c, key, pres, u, attr, msgs):
    """verify from the entries that existed before; the points of these honest presentations are canonical, so their wire bytes are hashed"""
    n = pres.shape[0]
    pub, _ = c.g1_decompress(key.pk[:49] + key.Y49)
    g, Y = pub[:96], pub[96:]
    g2, _ = c.g2_decompress(key.pk[49:])
    A_, B_, U = (c.g1_decompress(np.ascontiguousarray(pres[:, 49 * k:49 * k + 49]).tobytes())[0] for k in range(3))
    Y_I = b"".join(Y[96 * i:96 * i + 96] for i in I)
    Y_J = b"".join(Y[96 * j:96 * j + 96] for j in J)
    K = c.g1_mul_fixed_sum(Y_I, base_major(attr.reshape(n, NI, 48)[:, :, 16:]), g, 96)
    t0 = time.perf_counter()
    digests = hash_rows(msgs, pres[:, :147])
    negB = b"".join(B_[96 * j:96 * j + 48] + (P - int.from_bytes(B_[96 * j + 48:96 * j + 96], "big")).to_bytes(48, "big") for j in range(n))
    th = time.perf_counter() - t0
    cc = c.zp_from_hash(digests)
    s, t = (np.ascontiguousarray(pres[:, 163 + 48 * k:195 + 48 * k]).tobytes() for k in range(2))
    Rp = c.g1_mul_sum(K + A_ + negB, s + t + cc, 3, 96)
    S = c.g1_mul_fixed_sum(Y_J, base_major(u.reshape(n, NJ, 48)[:, :, 16:]), None, 96)
    got = arr(c.g1_add(Rp, S, 49), 49)
    okp = np.frombuffer(c.ps_verify(g2[:192], g2[192:], b"", A_, B_, b""), dtype=u8)
    return ((okp == 1) & (got == pres[:, 98:147]).all(axis=1)).astype(u8).tobytes(), th


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--distinct-log2n", type=int, default=12)
    args = ap.parse_args()
    assert args.steps >= 5, "medians of at least 5 steps"
    n, nd = 1 << args.log2n, 1 << min(args.log2n, args.distinct_log2n)
    c, c2 = Context(0), Context(0)
    dev = torch.device("cuda", 0)
    key = Key(c2)
    t0 = time.perf_counter()
    a, sig, msgs, rnd = (np.tile(x, (n // nd,) + (1,) * (x.ndim - 1)) for x in make(c2, key, nd))
    attr48 = f48(a)
    print("issued %d distinct credentials on the device, tiled to 2^%d lanes: nattr %d, I = %s, msg_len %d (%.1f s)"
          % (nd, args.log2n, NATTR, I, MSG_LEN, time.perf_counter() - t0))
    d = lambda x: torch.frombuffer(bytearray(x if isinstance(x, bytes) else x.tobytes()), dtype=torch.uint8).to(dev)
    d_pk, d_Y, d_attr, d_sig, d_msg, d_rnd = d(key.pk), d(key.Y49), d(attr48), d(sig), d(msgs), d(rnd)
    d_pres = torch.zeros(243 * n, dtype=torch.uint8, device=dev)
    d_u = torch.zeros(48 * NJ * n, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    d_ok = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    d_dis = d(np.ascontiguousarray(attr48[:, list(I)]))
    torch.cuda.synchronize()
    digest = lambda b: hashlib.sha256(b).hexdigest()[:12]
    host_b = [x.tobytes() for x in (attr48, sig, msgs, rnd)]
    dis_b = np.ascontiguousarray(attr48[:, list(I)]).tobytes()

    def clock(fn):
        t = time.perf_counter()
        out = fn()
        return time.perf_counter() - t, out

    def pres_dev():
        c.ac_bbs_pres_dev(n, NATTR, I, MSG_LEN, d_pk.data_ptr(), d_Y.data_ptr(), d_attr.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), d_rnd.data_ptr(),
                          d_pres.data_ptr(), d_u.data_ptr(), d_st.data_ptr())
        assert c.sync() == 0

    def verify_dev():
        c.ac_bbs_verify_dev(n, NATTR, I, MSG_LEN, d_pk.data_ptr(), d_Y.data_ptr(), d_pres.data_ptr(), d_u.data_ptr(), d_dis.data_ptr(), d_msg.data_ptr(),
                            d_ok.data_ptr())
        assert c.sync() == 0
    pres_host = lambda: c.ac_bbs_pres(key.pk, key.Y49, I, *host_b, MSG_LEN)
    first = {"pres_dev": clock(pres_dev)[0], "verify_dev": clock(verify_dev)[0]}
    pres_b, u_b = bytes(d_pres.cpu().numpy().tobytes()), bytes(d_u.cpu().numpy().tobytes())
    assert bytes(d_st.cpu().numpy().tobytes()) == bytes(n) and bytes(d_ok.cpu().numpy().tobytes()) == b"\x01" * n, "a lane was rejected"
    verify_host = lambda: c.ac_bbs_verify(key.pk, key.Y49, I, pres_b, u_b, dis_b, host_b[2], MSG_LEN)
    pres_np, u_np, dis_np = arr(pres_b, 243), arr(u_b, 48 * NJ), arr(dis_b, 48 * NI)
    comp_pres = lambda: composed_pres(c2, key, a, sig, msgs, rnd)
    comp_verify = lambda: composed_verify(c2, key, pres_np, u_np, dis_np, msgs)
    first["pres_composed"], (cp, cu, _) = clock(comp_pres)
    first["verify_composed"], (cok, _) = clock(comp_verify)
    assert (cp, cu) == (pres_b, u_b), "composed presentations disagree"
    assert cok == b"\x01" * n, "composed verdicts disagree"
    legs = {"pres_dev": pres_dev, "pres_composed": comp_pres, "pres_host": pres_host, "verify_dev": verify_dev, "verify_composed": comp_verify,
            "verify_host": verify_host}
    first["pres_host"], hp = clock(pres_host)
    first["verify_host"], hv = clock(verify_host)
    assert hp == (pres_b, u_b, bytes(n)) and hv == b"\x01" * n, "the host form disagrees with the _dev form"
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    times = {k: [] for k in legs}
    hashing = {"pres_composed": [], "verify_composed": []}
    for _ in range(args.steps):                              # interleaved: every route sees the same clocks and the same neighbours
        for k, fn in legs.items():
            dt, out = clock(fn)
            times[k].append(dt)
            if k in hashing:
                hashing[k].append(out[-1])
    med = {k: statistics.median(v) for k, v in times.items()}
    print("digests: pres %s = composed %s, u %s = composed %s, ok %s = composed %s" % (digest(pres_b), digest(cp), digest(u_b), digest(cu),
                                                                                       digest(b"\x01" * n), digest(cok)))
    print("2^%d presentations, warmup %d, steps %d, interleaved; first call / median (min, max) in ms" % (args.log2n, args.warmup, args.steps))
    for k in legs:
        extra = "   of which SHA3-512 and negation on the host %.1f" % (statistics.median(hashing[k]) * 1e3) if k in hashing else ""
        print("  %-16s first %9.2f   median %9.2f (%9.2f, %9.2f)   %.3e /s%s"
              % (k, first[k] * 1e3, med[k] * 1e3, min(times[k]) * 1e3, max(times[k]) * 1e3, n / med[k], extra))
    for w in ("pres", "verify"):
        print("%s: composed / one-call host form %.2fx (like for like: both stage from host memory), composed / _dev form %.2fx"
              % (w, med[w + "_composed"] / med[w + "_host"], med[w + "_composed"] / med[w + "_dev"]))
    try:
        print("device %s, shader clock reported after the timed legs: %d MHz" % (torch.cuda.get_device_name(0), torch.cuda.clock_rate(0)))
    except Exception as e:
        print("device %s, shader clock not available (%s)" % (torch.cuda.get_device_name(0), type(e).__name__))
    c.close(); c2.close()


if __name__ == "__main__":
    main()
