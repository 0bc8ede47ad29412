"""The complete fallback of the G1 scalar multiplication on the device (g1_mul_kernel: g1_scalar_mul, then g1_scalar_mul_complete for
the lanes whose Jacobian Z became 0), fed with points of small order from g1_torsion.py so that the fallback actually runs: whole
wavefronts of it, single fallback lanes at either end of a wavefront, scattered loop exceptions of eigenpoints, and the entry points that
launch the kernel (compressed input, the _dev form on a side stream, F_IN_SUBGROUP, the broadcast launch of g1_mul_fixed, the product
routes) plus the finish kernel's chains over infinity and invalid results.  Every lane is compared with the CPU oracle; every input is
computed on the CPU, and the lanes that must fall back are counted by the predictor, so the test cannot quietly stop reaching the path."""
import os
import subprocess
import sys

import pytest

from g1_torsion import X2, crt, ec_add, enc, eigenpoint, exceptional, generator, point_of_order
from util import P, R, prng

pytestmark = pytest.mark.gpu

W = 64                                      # lanes per wavefront (BLOCK = 256: four per workgroup)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF_CURVE = (1).to_bytes(48, "big") + (1).to_bytes(48, "big")


def _b32(k):
    return (k % (1 << 256)).to_bytes(32, "big")


@pytest.fixture(scope="module")
def batch(oracle_port):
    """A ragged batch of wavefront layouts: (points, scalars, per-lane kind, per-lane predicted fallback, dict of named points)"""
    g = generator()
    o3a, o3b, o11 = (0, 2), (0, P - 2), point_of_order(11)
    te, lam = eigenpoint(10177)
    g3 = ec_add(g, o3a)
    subs = oracle_port.g1_mul(enc(g) * 96, b"".join(_b32(prng(9501, i) % R) for i in range(96)), 96, 8)
    sub = lambda i: subs[96 * (i % 96):96 * (i % 96) + 96]
    lanes = []                                                              # (point bytes, scalar, kind)
    # wavefront 0: every lane falls back.  Order 3 and 11 alternately; scalars below x^2 (the [r]phi(P) term follows the fallback),
    # multiples of the order (the fallback itself returns infinity), above x^2, and random
    ks = list(range(1, 23)) + [33, 66, 99, 3 * 11 * 7, X2 + 1, 2 * X2 + 2, 11 * X2 + 11, X2 - 1, R - 1, (1 << 256) - 1]
    ks += [prng(9502, i) % (1 << 256) for i in range(W - len(ks))]
    for i, k in enumerate(ks):
        lanes.append((enc((o3a, o11, o3b)[i % 3]), k, "small"))
    # wavefronts 1 and 2: one fallback lane, at lane 0 and at lane 63, among subgroup lanes
    k_exc = next(k for k in (prng(9503, i) % (1 << 256) for i in range(10000)) if exceptional(k, 10177, lam))
    for w, pos, (pt, k, kind) in ((1, 0, (enc(te), k_exc, "eigen")), (2, W - 1, (enc(o11), prng(9504, 0), "small"))):
        for i in range(W):
            lanes.append((pt, k, kind) if i == pos else (sub(64 * w + i), prng(9505, 64 * w + i) % (1 << 256), "sub"))
    # wavefronts 3..10: the eigenpoint with random scalars (its loop exceptions are scattered)
    for i in range(8 * W):
        lanes.append((enc(te), prng(9506, i) % (1 << 256), "eigen"))
    # a ragged last wavefront: subgroup points, infinity, zero scalars, G + (0, 2)
    for i in range(37):
        c = i % 4
        pt = (sub(i), bytes(96), sub(i + 1), enc(g3))[c]
        k = (prng(9507, i) % (1 << 256), prng(9508, i) % (1 << 256), 0 if i % 8 == 2 else R, prng(9509, i) % (1 << 256))[c]
        lanes.append((pt, k, ("sub", "inf", "sub", "mixed3")[c]))

    def falls_back(pt, k, kind):
        if kind == "small":
            return k % R != 0
        if kind == "eigen":
            return exceptional(k, 10177, lam) is not None
        if kind == "sub":
            return exceptional(k, R, X2 % R) is not None
        if kind == "mixed3":
            return exceptional(k, 3 * R, crt(X2, R, -1, 3)) is not None
        return False
    fb = [falls_back(*ln) for ln in lanes]
    pts = b"".join(ln[0] for ln in lanes)
    sc = b"".join(_b32(ln[1]) for ln in lanes)
    named = {"o3a": o3a, "o3b": o3b, "o11": o11, "te": te, "g3": g3, "gte": ec_add(g, te), "g": g}
    return pts, sc, [ln[2] for ln in lanes], fb, named


def _lanes(buf, w, idx):
    return b"".join(buf[w * i:w * i + w] for i in idx)


def test_fallback_wavefront_layouts(batch, oracle_port):
    """the ragged batch at 49 and 96 bytes: every lane equals the oracle; the predicted fallback lanes are where they were built to be;
    strict mode raises nothing; an off-curve lane inside the all-fallback wavefront is 0xff and E_POINT, its neighbours unchanged"""
    from crypto12381_amd import Context
    from crypto12381_amd.capi import C12381Error, E_POINT
    pts, sc, kinds, fb, _ = batch
    n = len(kinds)
    assert n % W != 0
    waves = [fb[w * W:(w + 1) * W] for w in range((n + W - 1) // W)]
    assert all(waves[0]) and waves[1] == [True] + [False] * (W - 1) and waves[2] == [False] * (W - 1) + [True]
    eig = [sum(wv) for wv in waves[3:11]]
    assert sum(eig) >= 4 and sum(1 for c in eig if c) >= 3, eig            # loop exceptions in several eigenpoint wavefronts
    assert not any(waves[11])
    ctx = Context(0)
    for fmt in (49, 96):
        got = ctx.g1_mul(pts, sc, fmt)
        exp = oracle_port.g1_mul(pts, sc, fmt, 8)
        bad = [i for i in range(n) if got[fmt * i:fmt * i + fmt] != exp[fmt * i:fmt * i + fmt]]
        assert bad == [], [(i, kinds[i], fb[i]) for i in bad[:8]]
        # one lane of wavefront 0 off the curve
        bad_pts = pts[:96 * 5] + OFF_CURVE + pts[96 * 6:]
        with pytest.raises(C12381Error) as e:
            ctx.g1_mul(bad_pts, sc, fmt)
        assert e.value.code == E_POINT
        got = ctx.g1_mul(bad_pts, sc, fmt, strict=False)
        assert got[fmt * 5:fmt * 6] == b"\xff" * fmt
        assert got[:fmt * 5] == exp[:fmt * 5] and got[fmt * 6:] == exp[fmt * 6:]
    ctx.close()


def test_finish_chains_over_fallback_results(batch, oracle_port):
    """n = 2^17 + 3 tiles the batch; the simultaneous inversion runs 3 elements per lane (t, t + T, t + 2T).  Planted: a lane whose whole
    chain is infinity (from the fallback, from an infinity point, from a zero scalar), a chain with one finite element, and a chain of
    an invalid input, an infinity and a finite result (X = 1, Z = 0 against X = 0, Z = 0)"""
    from crypto12381_amd import Context
    pts, sc, kinds, _, named = batch
    nb = len(kinds)
    n = (1 << 17) + 3
    per = (n + 65535) // 65536
    T = (n + per - 1) // per
    T = (T + 63) // 64 * 64                                                 # finish_lanes in c12381_hip.hip
    assert per == 3 and n - 2 * T > 40000
    reps = n // nb + 1
    P_ = bytearray((pts * reps)[:96 * n])
    S_ = bytearray((sc * reps)[:32 * n])
    o3 = enc(named["o3a"])
    inf_in = [(o3, X2 + 1), (bytes(96), prng(9510, 0)), (enc(named["g"]), 0), (o3, 2 * X2 + 2)]    # fallback -> infinity, inf point, k = 0
    t0, t1, t2 = 5, n - 2 * T - 1, 1000
    plant = {t0: inf_in[0], t0 + T: inf_in[1], t0 + 2 * T: inf_in[3],
             t1: inf_in[2], t1 + 2 * T: inf_in[0],
             t2: (OFF_CURVE, prng(9511, 0)), t2 + T: inf_in[3]}
    for e, (pb, k) in plant.items():
        P_[96 * e:96 * e + 96] = pb
        S_[32 * e:32 * e + 32] = _b32(k)
    ctx = Context(0)
    for fmt in (49, 96):
        tile = oracle_port.g1_mul(pts, sc, fmt, 8)
        exp = bytearray((tile * reps)[:fmt * n])
        for e, (pb, k) in plant.items():
            v = b"\xff" * fmt if pb == OFF_CURVE else oracle_port.g1_mul(pb, _b32(k), fmt, 1)
            assert pb == OFF_CURVE or v == bytes(fmt), e                      # the planted valid inputs give infinity
            exp[fmt * e:fmt * e + fmt] = v
        got = ctx.g1_mul(bytes(P_), bytes(S_), fmt, strict=False)
        assert got[fmt * (t1 + T):fmt * (t1 + T + 1)] != bytes(fmt)             # the finite element of chain t1
        if got != bytes(exp):
            bad = [i for i in range(n) if got[fmt * i:fmt * i + fmt] != exp[fmt * i:fmt * i + fmt]]
            pytest.fail("fmt %d: %d lanes differ, first %s" % (fmt, len(bad), [(i, i % T, kinds[i % nb]) for i in bad[:8]]))
    ctx.close()


def test_entry_points_over_fallback_lanes(batch, oracle_port):
    """compressed input (with the device's decompression), the _dev form on a side stream, F_IN_SUBGROUP, g1_mul_fixed on torsion bases
    (generic broadcast launch), the bucket product and sum_of_products with torsion terms, and additions on order-3 points"""
    import torch
    from crypto12381_amd import Context
    from crypto12381_amd.capi import F_COMPRESSED_IN, F_IN_SUBGROUP
    pts, sc, kinds, fb, named = batch
    n = len(kinds)
    ctx = Context(0)
    exp96 = oracle_port.g1_mul(pts, sc, 96, 8)
    exp49 = oracle_port.g1_mul(pts, sc, 49, 8)
    # compressed encodings of the same points: (0, +-2) are x = 0 under either sign tag, infinity is all-zero
    c49 = oracle_port.g1_compress(pts)
    xz = b"".join(bytes([t]) + x.to_bytes(48, "big") for t in (2, 3) for x in (0, P))
    assert ctx.g1_decompress(c49 + xz) == oracle_port.g1_decompress(c49 + xz)
    assert ctx.g1_decompress(c49)[0] == pts and set(ctx.g1_decompress(c49)[1]) == {1}
    assert ctx.g1_mul_flags(c49, sc, 96, F_COMPRESSED_IN) == exp96
    assert ctx.g1_mul_flags(c49, sc, 49, F_COMPRESSED_IN) == exp49
    # _dev on torch tensors, the library on a non-default stream
    dev = torch.device("cuda", 0)
    dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).to(dev)
    dc = torch.frombuffer(bytearray(c49), dtype=torch.uint8).to(dev)
    ds = torch.frombuffer(bytearray(sc), dtype=torch.uint8).to(dev)
    o96 = torch.empty(96 * n, dtype=torch.uint8, device=dev)
    o49 = torch.empty(49 * n, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    ctx.set_stream(s.cuda_stream)
    ctx.g1_mul_flags_dev(n, dp.data_ptr(), ds.data_ptr(), o96.data_ptr(), 96, 0)
    ctx.g1_mul_flags_dev(n, dc.data_ptr(), ds.data_ptr(), o49.data_ptr(), 49, F_COMPRESSED_IN)
    assert ctx.sync() == 0
    assert o96.cpu().numpy().tobytes() == exp96 and o49.cpu().numpy().tobytes() == exp49
    ctx.set_stream(None)
    # F_IN_SUBGROUP: the subgroup lanes of the wavefronts that hold fallback lanes
    got = ctx.g1_mul_flags(pts, sc, 96, F_IN_SUBGROUP)
    shared = [i for i in range(n) if kinds[i] == "sub" and any(fb[(i // W) * W:(i // W + 1) * W])]
    assert len(shared) >= 2 * (W - 1)
    assert _lanes(got, 96, shared) == _lanes(exp96, 96, shared)
    # one torsion base for the whole batch: not in G1, so the fixed-base table is refused and every lane runs the generic kernel
    m = 3 * W + 5
    fsc = sc[:32 * m]
    for name in ("o3a", "o3b", "o11", "te", "g3", "gte"):
        base = enc(named[name])
        for fmt in (49, 96):
            assert ctx.g1_mul_fixed(base, fsc, fmt) == oracle_port.g1_mul(base * m, fsc, fmt, 8), (name, fmt)
    # products: a single torsion term (the scalar-multiplication route), and torsion terms among random subgroup terms (buckets)
    tor = [named[k] for k in ("o3a", "o3b", "o11", "te", "g3", "gte")]
    tsc = [5, 22, X2 + 1, prng(9512, 0), R - 1, 3 * X2 - 40]
    for p, k in zip(tor, tsc):
        assert ctx.g1_msm(enc(p), _b32(k), 96) == oracle_port.g1_msm(enc(p), _b32(k), 96, 1)
    subs = [i for i in range(n) if kinds[i] == "sub"]
    for m in (300, (1 << 12) + 37):
        idx = [subs[i % len(subs)] for i in range(m - len(tor))]
        tp = _lanes(pts, 96, idx)
        ts = _lanes(sc, 32, idx)
        for j, (p, k) in enumerate(zip(tor, tsc)):                            # torsion terms spread through the product
            at = 96 * (j * (m // len(tor)))
            tp = tp[:at] + enc(p) + tp[at:]
            ts = ts[:at // 3] + _b32(k) + ts[at // 3:]
        assert ctx.g1_msm(tp, ts, 49) == oracle_port.g1_msm(tp, ts, 49, 8), m
        if m == 300:
            assert ctx.g1_sum_of_products(tp, ts, 96) == oracle_port.g1_sum_of_products(tp, ts, 96), m
    # additions on the order-3 points: P + P, P + (-P), with infinity and with G + (0, 2)
    o3a, o3b, g3 = named["o3a"], named["o3b"], named["g3"]
    a = [o3a, o3a, o3b, o3b, o3a, None, g3, g3, g3]
    b = [o3a, o3b, o3a, o3b, None, o3b, o3a, o3b, g3]
    ab, bb = b"".join(enc(p) for p in a), b"".join(enc(q) for q in b)
    for fmt in (49, 96):
        assert ctx.g1_add(ab, bb, fmt) == oracle_port.g1_add(ab, bb, fmt), fmt
    assert ctx.g1_add(ab, bb, 96) == b"".join(enc(ec_add(p, q)) for p, q in zip(a, b))
    ctx.close()


NAIVE_CODE = r"""
import sys
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')
import tools.libsel  # C12381_LIB -> capi.use_library
from crypto12381_amd import Context
c = Context(0)
data = sys.stdin.buffer.read()
for m in (300, 4133):
    tp, data = data[:96 * m], data[96 * m:]
    ts, data = data[:32 * m], data[32 * m:]
    sys.stdout.buffer.write(c.g1_msm(tp, ts, 96))
c.close()
"""


def test_product_by_scalar_multiplications_with_torsion_terms(batch, oracle_port):
    """the n-scalar-multiplication route of the product (g1_mul_kernel + tree sum, selected by C12381_MSM=naive in the experiments
    build) on either side of the 4096-term step of its reduction, with torsion terms that take the fallback"""
    pts, sc, kinds, fb, _ = batch
    n = len(kinds)
    data, exp = b"", b""
    for m in (300, 4133):
        idx = [(7 * i) % n for i in range(m)]                               # every lane of the batch, fallback lanes included
        tp, ts = _lanes(pts, 96, idx), _lanes(sc, 32, idx)
        data += tp + ts
        exp += oracle_port.g1_msm(tp, ts, 96, 8)
    assert sum(fb[(7 * i) % n] for i in range(300)) >= 10
    env = {k: v for k, v in os.environ.items() if not k.startswith("C12381_")}
    env.update(C12381_LIB=os.path.join(ROOT, "crypto12381_amd", "lib", "libc12381_hip_exp.so"), C12381_MSM="naive")
    r = subprocess.run([sys.executable, "-c", NAIVE_CODE], input=data, env=env, cwd=ROOT, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == exp
