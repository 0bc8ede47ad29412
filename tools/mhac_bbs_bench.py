#!/usr/bin/env python3
"""MHAC-bbs presentation and verification of 2^18 presentations on one MI355X, for two shapes: the reference's examples/MHAC-bbs/test.cpp (m = 4,
Prv = (0, 2), Rev = (1), t = 3) and m = 16 with four private and two revealed attributes, t = 3:
  - c12381_mhac_bbs_pres_batch / c12381_mhac_bbs_verify_batch in the _dev form (resident inputs) and the host form (staging included): the first
    call of a context (tables built, workspaces allocated) and the median of the timed steps, separately;
  - A/B in the same process, interleaved step by step: the same presentations and verdicts composed from the public entries that existed before
    (g1_decompress, g1_mul_fixed_sum, g1_mul_sum, g1_mul, g1_add, ps_verify with no messages, zp_op / zp_from_hash, SHA3-512 by hashlib on the
    host), in host forms, on a context of its own so that neither route evicts the other's tables.  Output digests must be equal.
Credentials are issued on the device (one group of t parties per credential, the shares chosen so that they interpolate the attributes);
--distinct-log2n of them are tiled to 2^log2n lanes.  The report goes to --out (default profiles/mhac_bbs_bench.txt).

    python tools/mhac_bbs_bench.py [--steps 5] [--warmup 1] [--log2n 18] [--distinct-log2n 12] [--out FILE]"""
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
from tools.ac_bbs_bench import R, arr, base_major, col, enc49, f48, scalars  # noqa: E402
from tools.prof_driver import G1, G2  # noqa: E402

T = 3
SHAPES = [(4, (0, 2), (1,)), (16, (0, 1, 2, 3), (4, 5))]
u8 = np.uint8
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def ints(a32):
    """(..., 32) scalars -> nested lists of integers"""
    flat = a32.reshape(-1, 32)
    return np.array([int.from_bytes(r.tobytes(), "big") for r in flat], dtype=object).reshape(a32.shape[:-1])


def sc32(vals):
    """object array of integers (n, k) or (n,) -> (n, k, 32) / (n, 32) scalars mod r"""
    v = np.asarray(vals, dtype=object)
    out = np.frombuffer(b"".join((int(x) % R).to_bytes(32, "big") for x in v.reshape(-1)), dtype=u8)
    return out.reshape(v.shape + (32,)).copy()


def cols(a):
    """(n, 32) or (n, k, 32) scalars -> base-major bytes"""
    return base_major(a if a.ndim == 3 else a[:, None, :])


class Shape:
    def __init__(self, m, Prv, Rev):
        self.m, self.Prv, self.Rev = m, list(Prv), list(Rev)
        self.Pub = [i for i in range(m) if i not in Prv]
        self.Hid = [i for i in range(m) if i not in Rev]
        self.HidPub = [i for i in self.Hid if i not in Prv]
        self.RevPub = [k for k, i in enumerate(self.Pub) if i in Rev]
        self.PubHid = [k for k, i in enumerate(self.Pub) if i in self.Hid]
        self.nrnd = 2 + (T - 1) * len(Prv) + len(self.Hid) + T
        self.o_bj, self.o_g = 2 + (T - 1) * len(Prv), 2 + (T - 1) * len(Prv) + len(self.Hid)
        assert all(self.Hid[ii] == Prv[ii] for ii in range(len(Prv))), "a shape whose honest presentations the reference's formulas reject"


class World:
    def __init__(self, c, m):
        k = lambda t: int.from_bytes(hashlib.sha512(b"mhac-bbs world|" + t).digest(), "big") % R
        one = col([1])
        self.g1 = c.g1_mul_fixed(G1, col([k(b"g1")]), 96)
        self.g2 = c.g2_mul(G2, col([k(b"g2")]), 192)
        self.gamma = k(b"gamma")
        self.w = c.g2_mul(self.g2, col([self.gamma]), 192)
        self.h = c.g1_mul_fixed(G1, col([k(b"h%d" % i) for i in range(m)]), 96)
        self.pp = c.g1_mul(self.g1, one, 49) + c.g2_mul(self.g2, one, 97)
        self.pk = c.g2_mul(self.w, one, 97)
        self.h49 = c.g1_mul(self.h, one * m, 49)

    def hs(self, idx):
        return b"".join(self.h[96 * i:96 * i + 96] for i in idx)


def make(c, wd, sh, nd):
    """nd credentials with their groups and types: dict of (nd, ...) uint8 arrays in the entry's wire formats"""
    nP, nPub = len(sh.Prv), len(sh.Pub)
    xs = [k + 1 for k in range(T)]
    lam = [1] * T
    for k in range(T):
        for y in range(T):
            if y != k:
                lam[k] = lam[k] * (-xs[y] % R) * pow((xs[k] - xs[y]) % R, -1, R) % R
    a_S = ints(scalars(b"a_S%d" % sh.m, (nd, T, nP)))
    e_S = ints(scalars(b"e_S%d" % sh.m, (nd, T)))
    pub_a = ints(scalars(b"pub%d" % sh.m, (nd, nPub)))
    attr_prv = np.array([[sum(lam[k] * a_S[j, k, ii] for k in range(T)) % R for ii in range(nP)] for j in range(nd)], dtype=object).reshape(nd, nP)
    e = np.array([sum(lam[k] * e_S[j, k] for k in range(T)) % R for j in range(nd)], dtype=object)
    C_prv = c.g1_mul_fixed_sum(wd.hs(sh.Prv), cols(sc32(attr_prv)), None, 96)
    C_a = c.g1_mul_fixed_sum(wd.hs(sh.Pub), cols(sc32(pub_a)), wd.g1, 96)
    C_a = c.g1_add(C_a, C_prv, 96)
    inv = c.zp_op("inv", sc32(np.array([(wd.gamma + x) % R for x in e], dtype=object)).tobytes())
    A = c.g1_mul(C_a, inv, 96)
    D = c.g1_add(C_prv, c.g1_mul(A, sc32(np.array([-x % R for x in e], dtype=object)).tobytes(), 96), 96)
    revp = sc32(pub_a[:, sh.RevPub]) if sh.RevPub else None
    C_rev = c.g1_mul_fixed_sum(wd.hs([sh.Pub[k] for k in sh.RevPub]), cols(revp), wd.g1, 96) if sh.RevPub else wd.g1 * nd
    if sh.PubHid:
        C_pub = c.g1_add(C_rev, c.g1_mul_fixed_sum(wd.hs([sh.Pub[k] for k in sh.PubHid]), cols(sc32(pub_a[:, sh.PubHid])), None, 96), 96)
    else:
        C_pub = C_rev
    one = col([1]) * nd
    w49 = lambda p: arr(c.g1_mul(p, one, 49), 49)
    return dict(A=w49(A), D=w49(D), lam=f48(sc32(np.array([lam] * nd, dtype=object))), es=f48(sc32(e_S)), ash=f48(sc32(a_S)).reshape(nd, T * nP, 48), crev=w49(C_rev),
                cpub=w49(C_pub), pub=f48(sc32(pub_a)), rnd=scalars(b"rnd%d" % sh.m, (nd, sh.nrnd)))


def hash_rows(e147, fields):
    rows = np.concatenate([e147, fields.reshape(e147.shape[0], -1)], axis=1)
    return b"".join(hashlib.sha3_512(r.tobytes()).digest() for r in rows)


def composed_pres(c, wd, sh, x):
    """cred_pres from the entries that existed before: (fixed_242, z_48, zhp_48) bytes and the seconds spent hashing on the host"""
    n, nP, zp = x["A"].shape[0], len(sh.Prv), c.zp_op
    dec = lambda a: c.g1_decompress(np.ascontiguousarray(a).tobytes())[0]
    A, D, C_rev, C_pub = dec(x["A"]), dec(x["D"]), dec(x["crev"]), dec(x["cpub"])
    rnd = x["rnd"]
    rc = lambda k: np.ascontiguousarray(rnd[:, k]).tobytes()
    r, alpha = rc(0), rc(1)
    AB = c.g1_mul(A + c.g1_add(C_pub, D, 96), r + r, 96)
    A_, B_ = AB[:96 * n], AB[96 * n:]
    U = c.g1_mul_sum(C_rev + A_ * T, alpha + b"".join(rc(sh.o_g + k) for k in range(T)), T + 1, 96)
    lst = list(sh.Hid) + sh.Prv * (T - 1)
    ex = np.concatenate([rnd[:, sh.o_bj:sh.o_bj + len(sh.Hid)], rnd[:, 2:2 + (T - 1) * nP]], axis=1)
    U = c.g1_add(U, c.g1_mul_fixed_sum(wd.hs(lst), base_major(ex), None, 96), 96)
    e = np.concatenate([enc49(arr(p, 96)) for p in (U, A_, B_)], axis=1)
    t0 = time.perf_counter()
    digests = hash_rows(e, x["pub"][:, sh.RevPub])
    th = time.perf_counter() - t0
    ch = c.zp_from_hash(digests)
    chr_ = zp("mul", ch, r)
    f = lambda a48, k: np.ascontiguousarray(a48[:, k, 16:]).tobytes()
    zr = zp("add", alpha, chr_)
    ze = None
    for k in range(T):
        term = zp("add", rc(sh.o_g + k), zp("mul", ch, zp("mul", zp("neg", f(x["es"], k)), f(x["lam"], k))))
        ze = term if ze is None else zp("add", ze, term)
    z = []
    for ii in range(nP):
        acc = rc(sh.o_bj + ii)
        for k in range(T):
            acc = zp("add", acc, zp("mul", chr_, zp("mul", f(x["ash"], k * nP + ii), f(x["lam"], k))))
            if k:
                acc = zp("add", acc, rc(2 + (k - 1) * nP + ii))
        z.append(arr(acc, 32))
    zhp = [arr(zp("add", rc(sh.o_bj + sh.Hid.index(i)), zp("mul", chr_, f(x["pub"], sh.Pub.index(i)))), 32) for i in sh.HidPub]
    fixed = np.concatenate([e[:, 49:], f48(arr(ch, 32)), f48(arr(zr, 32)), f48(arr(ze, 32))], axis=1)
    pack = lambda v: f48(np.stack(v, axis=1)).tobytes() if v else b""
    return fixed.tobytes(), pack(z), pack(zhp), th


def composed_verify(c, wd, sh, crev, fixed, z, zhp, rev):
    """verify_pres from the entries that existed before; the points of these honest presentations are canonical, so their wire bytes are hashed"""
    n, nP, nhp = fixed.shape[0], len(sh.Prv), len(sh.HidPub)
    lst = sh.Prv + sh.HidPub
    hl, _ = c.g1_decompress(b"".join(wd.h49[49 * i:49 * i + 49] for i in lst))
    g2, _ = c.g2_decompress(wd.pp[49:])
    w, _ = c.g2_decompress(wd.pk)
    dec = lambda a: c.g1_decompress(np.ascontiguousarray(a).tobytes())[0]
    A_, B_, C_rev = dec(fixed[:, :49]), dec(fixed[:, 49:98]), dec(crev)
    ch, zr, ze = (np.ascontiguousarray(fixed[:, 114 + 48 * k:146 + 48 * k]).tobytes() for k in range(3))
    Rp = c.g1_mul_sum(B_ + C_rev + A_, c.zp_op("neg", ch) + zr + ze, 3, 96)
    ex = np.concatenate([z.reshape(n, nP, 48)[:, :, 16:], zhp.reshape(n, nhp, 48)[:, :, 16:]], axis=1)
    U = arr(c.g1_add(Rp, c.g1_mul_fixed_sum(hl, base_major(ex), None, 96), 49), 49)
    t0 = time.perf_counter()
    digests = hash_rows(np.concatenate([U, fixed[:, :98]], axis=1), rev)
    th = time.perf_counter() - t0
    same = (arr(c.zp_from_hash(digests), 32) == arr(ch, 32)).all(axis=1)
    okp = np.frombuffer(c.ps_verify(g2, w, b"", A_, B_, b""), dtype=u8)
    return ((okp == 1) & same).astype(u8).tobytes(), th


def run_shape(c, c2, args, m, Prv, Rev):
    sh = Shape(m, Prv, Rev)
    n, nd = 1 << args.log2n, 1 << min(args.log2n, args.distinct_log2n)
    nP, nhp, nrp, nPub = len(sh.Prv), len(sh.HidPub), len(sh.RevPub), len(sh.Pub)
    dev = torch.device("cuda", 0)
    wd = World(c2, m)
    t0 = time.perf_counter()
    x = {k: np.tile(v, (n // nd,) + (1,) * (v.ndim - 1)) for k, v in make(c2, wd, sh, nd).items()}
    say("shape m = %d, Prv = %s, Rev = %s, t = %d: issued %d distinct credentials on the device, tiled to 2^%d lanes (%.1f s)"
        % (m, tuple(Prv), tuple(Rev), T, nd, args.log2n, time.perf_counter() - t0))
    order = ("A", "D", "lam", "es", "ash", "crev", "cpub", "pub", "rnd")
    host_in = [x[k].tobytes() for k in order]
    d = lambda b: torch.frombuffer(bytearray(b) or bytearray(1), dtype=torch.uint8).to(dev)
    d_pp, d_h, d_pk = d(wd.pp), d(wd.h49), d(wd.pk)
    d_in = [d(b) for b in host_in]
    d_fixed, d_z, d_zhp = (torch.zeros(max(k * n, 1), dtype=torch.uint8, device=dev) for k in (242, 48 * nP, 48 * nhp))
    d_st = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    d_ok = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    rev_np = np.ascontiguousarray(x["pub"][:, sh.RevPub]).reshape(n, 48 * nrp)
    d_rev = d(rev_np.tobytes())
    torch.cuda.synchronize()
    pa, ra = (Context._idx(Prv), Context._idx(Rev))
    ptr = lambda t: t.data_ptr()
    from crypto12381_amd.capi import _p
    lib = c.lib

    def clock(fn):
        t = time.perf_counter()
        out = fn()
        return time.perf_counter() - t, out

    def pres_dev():
        rc = lib.c12381_mhac_bbs_pres_batch_dev(c.h, n, m, T, pa[1], pa[0], ra[1], ra[0], _p(ptr(d_pp)), _p(ptr(d_h)), *(_p(ptr(t)) for t in d_in),
                                               _p(ptr(d_fixed)), _p(ptr(d_z)), _p(ptr(d_zhp)), _p(ptr(d_st)))
        assert rc == 0 and c.sync() == 0

    def verify_dev():
        rc = lib.c12381_mhac_bbs_verify_batch_dev(c.h, n, m, pa[1], pa[0], ra[1], ra[0], _p(ptr(d_pp)), _p(ptr(d_h)), _p(ptr(d_pk)), _p(ptr(d_in[5])),
                                                 _p(ptr(d_fixed)), _p(ptr(d_z)), _p(ptr(d_zhp)), _p(ptr(d_rev)), _p(ptr(d_ok)))
        assert rc == 0 and c.sync() == 0
    first = {"pres_dev": clock(pres_dev)[0], "verify_dev": clock(verify_dev)[0]}
    tb = lambda t, k: bytes(t.cpu().numpy().tobytes())[:k]
    fixed_b, z_b, zhp_b = tb(d_fixed, 242 * n), tb(d_z, 48 * nP * n), tb(d_zhp, 48 * nhp * n)
    assert tb(d_st, n) == bytes(n) and tb(d_ok, n) == b"\x01" * n, "a lane was rejected"
    pres_host = lambda: c.mhac_bbs_pres(wd.pp, wd.h49, Prv, Rev, T, *host_in)
    verify_host = lambda: c.mhac_bbs_verify(wd.pp, wd.h49, wd.pk, Prv, Rev, host_in[5], fixed_b, z_b, zhp_b, rev_np.tobytes())
    fixed_np, z_np, zhp_np = arr(fixed_b, 242), np.frombuffer(z_b, dtype=u8), np.frombuffer(zhp_b, dtype=u8)
    comp_pres = lambda: composed_pres(c2, wd, sh, x)
    comp_verify = lambda: composed_verify(c2, wd, sh, x["crev"], fixed_np, z_np, zhp_np, rev_np)
    first["pres_composed"], (cf, cz, chp, _) = clock(comp_pres)
    first["verify_composed"], (cok, _) = clock(comp_verify)
    assert (cf, cz, chp) == (fixed_b, z_b, zhp_b), "composed presentations disagree"
    assert cok == b"\x01" * n, "composed verdicts disagree"
    first["pres_host"], hp = clock(pres_host)
    first["verify_host"], hv = clock(verify_host)
    assert hp == (fixed_b, z_b, zhp_b, bytes(n)) and hv == b"\x01" * n, "the host form disagrees with the _dev form"
    legs = {"pres_dev": pres_dev, "pres_composed": comp_pres, "pres_host": pres_host, "verify_dev": verify_dev, "verify_composed": comp_verify,
            "verify_host": verify_host}
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
    digest = lambda b: hashlib.sha256(b).hexdigest()[:12]
    say("digests: fixed %s = composed %s, z %s = composed %s, zhp %s = composed %s, ok %s = composed %s"
        % (digest(fixed_b), digest(cf), digest(z_b), digest(cz), digest(zhp_b), digest(chp), digest(b"\x01" * n), digest(cok)))
    say("2^%d presentations, warmup %d, steps %d, interleaved; first call / median (min, max) in ms" % (args.log2n, args.warmup, args.steps))
    for k in legs:
        extra = "   of which SHA3-512 on the host %.1f" % (statistics.median(hashing[k]) * 1e3) if k in hashing else ""
        say("  %-16s first %9.2f   median %9.2f (%9.2f, %9.2f)   %.3e /s%s"
            % (k, first[k] * 1e3, med[k] * 1e3, min(times[k]) * 1e3, max(times[k]) * 1e3, n / med[k], extra))
    for w in ("pres", "verify"):
        say("%s: composed / one-call host form %.2fx (like for like: both stage from host memory), composed / _dev form %.2fx"
            % (w, med[w + "_composed"] / med[w + "_host"], med[w + "_composed"] / med[w + "_dev"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--distinct-log2n", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mhac_bbs_bench.txt"))
    args = ap.parse_args()
    assert args.steps >= 5, "medians of at least 5 steps"
    say("python tools/mhac_bbs_bench.py --steps %d --warmup %d --log2n %d --distinct-log2n %d" % (args.steps, args.warmup, args.log2n, args.distinct_log2n))
    c, c2 = Context(0), Context(0)
    for m, Prv, Rev in SHAPES:
        run_shape(c, c2, args, m, Prv, Rev)
    try:
        say("device %s, shader clock reported after the timed legs: %d MHz" % (torch.cuda.get_device_name(0), torch.cuda.clock_rate(0)))
    except Exception as e:
        say("device %s, shader clock not available (%s)" % (torch.cuda.get_device_name(0), type(e).__name__))
    c.close(); c2.close()
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
