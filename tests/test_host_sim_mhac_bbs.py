"""CPU tests of the per-lane scalar and byte work of the MHAC-bbs entries (crypto12381_amd/csrc/mhac_bbs.hpp) compiled for the host with the bounds
checker (tests/host_sim/mhac_bbs.cpp, C12381_CHECK_BOUNDS), against Python: the derived sets and both base lists for every shape of the GPU tests
and the argument errors; the transcript and c at 0, 1, 2 and 3 revealed values (147 + 48 k bytes is 3, 51, 27 mod 72: the padding never meets a
block edge; the four lengths absorb three, three, four and five blocks); the Zp formulas of pres against Python integers with r = 0, ch r
wrapping, lambda = 0 and e = 0 (-0 = 0).  And tests/host_sim/mhac_layouts.cpp, a stand-alone program built with -fsanitize=address,undefined
that carves the two new slab layouts on mallocs of exactly their size."""
import ctypes
import hashlib
import os
import subprocess

import pytest

import mhac_bbs_cases as mh
from util import P, R, prng

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t


def _stale(target, srcs):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in srcs)


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIM_DIR, "libsim_mhac_bbs.so")
    src = os.path.join(SIM_DIR, "mhac_bbs.cpp")
    if _stale(so, [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def test_the_new_layouts_are_aligned_disjoint_and_inside_their_slabs():
    exe = os.path.join(SIM_DIR, "mhac_layouts")
    srcs = [os.path.join(SIM_DIR, "mhac_layouts.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if _stale(exe, srcs):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, srcs[0]], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mhac layouts ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


def u32(v):
    return (ctypes.c_uint32 * max(len(v), 1))(*v)


def derive(sim, m, Prv, Rev, t=1):
    counts, lists, vl, pl = (ctypes.create_string_buffer(k) for k in (7, 192, 32, 32))
    lens = (sz * 2)()
    if not sim.sim_mhac_bbs_sets(sz(m), u32(Prv), sz(len(Prv)), u32(Rev), sz(len(Rev)), sz(t), counts, lists, vl, pl, lens):
        return None
    c = list(counts.raw)
    take = lambda i, k: list(lists.raw[32 * i:32 * i + k])
    return dict(counts=c, prv=take(0, c[1]), hid=take(1, c[4]), hidpub=take(2, c[5]), revpub=take(3, c[6]), hp_hid=take(4, c[5]), hp_pub=take(5, c[5]),
                vlist=list(vl.raw[:lens[0]]), plen=lens[1], plist=list(pl.raw[:min(lens[1], 32)]))


SHAPES = [(4, (0, 2), (1,)), (4, (), (1,)), (4, (0, 1, 2, 3), ()), (4, (0, 2), ()), (4, (0, 2), (1, 3)), (4, (2, 0), (1,)), (1, (), ()), (1, (0,), ()),
          (1, (), (0,)), (32, (0, 2), (1,)), (32, tuple(range(31, 15, -1)), tuple(range(16))), (5, (0, 1, 2, 3), ()), (4, (), (3, 0, 2, 1))]


@pytest.mark.parametrize("m,Prv,Rev", SHAPES)
def test_sets_and_base_lists(sim, m, Prv, Rev):
    Pub, Hid, HidPub, RevPub, _ = mh.sets(m, Prv, Rev)
    for t in (1, 3, 8):
        d = derive(sim, m, Prv, Rev, t)
        assert d["counts"] == [m, len(Prv), len(Rev), len(Pub), len(Hid), len(HidPub), len(RevPub)]
        assert (d["prv"], d["hid"], d["hidpub"], d["revpub"]) == (list(Prv), Hid, HidPub, RevPub)
        assert d["hp_hid"] == [Hid.index(i) for i in HidPub] and d["hp_pub"] == [Pub.index(i) for i in HidPub]
        assert d["vlist"] == list(Prv) + HidPub
        want = Hid + list(Prv) * (t - 1)
        assert d["plen"] == len(want) and d["plist"] == want[:32]


def test_the_list_bound_of_pres(sim):
    assert derive(sim, 4, (0, 1, 2, 3), (), 8)["plen"] == 32 and derive(sim, 5, (0, 1, 2, 3), (), 8)["plen"] == 33


@pytest.mark.parametrize("m,Prv,Rev", [(0, (), ()), (33, (), ()), (4, (4,), ()), (4, (), (4,)), (4, (0, 0), ()), (4, (), (1, 2, 1)), (4, (0, 2), (2,)),
                                       (4, (1 << 31,), ()), (4, (), (36,)), (4, (0, 1, 2, 3, 0), ()), (1, (0,), (0,))])
def test_sets_refused(sim, m, Prv, Rev):
    """m = 0, m above the fixed-base bound, an index >= m (one that would shift out of the mask included), a repeated index, Rev and Prv meeting"""
    assert derive(sim, m, Prv, Rev) is None


def enc49(pt):
    return bytes(49) if pt is None else bytes([2 | (pt[1] & 1)]) + pt[0].to_bytes(48, "big")


def raw96(pt):
    return bytes(96) if pt is None else pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")


@pytest.mark.parametrize("count", [0, 1, 2, 3])
@pytest.mark.parametrize("perm", [None, (3, 0, 2)])
def test_transcript_and_challenge(sim, count, perm):
    """U | A_ | B_ | values, the points as serialize writes them (tag from the parity of y, 49 zeros for infinity), c = SHA3-512 mod r"""
    pts = [(prng(8700 + count, 0, 48) % P, prng(8700 + count, 1, 48) % P), (5, 2 * count + 2), None if count == 1 else (7, 2 * count + 1)]
    vals = [prng(8701, k) % R for k in range(4)]
    pick = list(perm[:count]) if perm else list(range(count))
    L = 147 + 48 * count
    tr, c = ctypes.create_string_buffer(L + 3), ctypes.create_string_buffer(32)
    pub = b"".join(mh.b48(v) for v in vals)
    assert sim.sim_mhac_bbs_challenge(raw96(pts[0]), raw96(pts[1]), raw96(pts[2]), pub, sz(count), bytes(perm) if perm else None, tr, c) == 0
    want = b"".join(enc49(p) for p in pts) + b"".join(mh.b48(vals[k]) for k in pick)
    assert tr.raw[:L] == want
    assert int.from_bytes(c.raw, "big") == int.from_bytes(hashlib.sha3_512(want).digest(), "big") % R


def responses(sim, m, Prv, Rev, t, ch, rnd, lam, es, a_S, pub_a):
    Pub, Hid, HidPub, _, _ = mh.sets(m, Prv, Rev)
    nP = len(Prv)
    b = lambda vals, w: b"".join(v.to_bytes(w, "big") for v in vals) or None
    zrze, z, zhp = (ctypes.create_string_buffer(max(k, 1)) for k in (96, 48 * nP, 48 * len(HidPub)))
    got = sim.sim_mhac_bbs_responses(sz(m), u32(Prv), sz(nP), u32(Rev), sz(len(Rev)), sz(t), ch.to_bytes(32, "big"), b(rnd, 32), b(lam, 48), b(es, 48),
                                     b([v for row in a_S for v in row], 48), b(pub_a, 48), zrze, z, zhp)
    assert got == len(rnd) == mh.rnd_count(m, Prv, Rev, t)
    v = [x % R for x in rnd]
    r, alpha, o_bj, o_g = v[0], v[1], 2 + (t - 1) * nP, 2 + (t - 1) * nP + len(Hid)
    ints = lambda buf, k: [int.from_bytes(buf.raw[48 * i:48 * i + 48], "big") for i in range(k)]
    ctx = (m, Prv, Rev, t, ch, rnd[:2])
    assert ints(zrze, 2) == [(alpha + ch * r) % R, sum(v[o_g + k] + ch * ((-es[k] % R) * lam[k]) for k in range(t)) % R], ctx
    assert ints(z, nP) == [(v[o_bj + ii] + ch * r * a_S[0][ii] * lam[0] + sum(v[2 + (k - 1) * nP + ii] + ch * r * a_S[k][ii] * lam[k] for k in range(1, t))) % R
                           for ii in range(nP)], ctx
    assert ints(zhp, len(HidPub)) == [(v[o_bj + Hid.index(i)] + ch * pub_a[Pub.index(i)] * r) % R for i in HidPub], ctx


def _lane(seed, m, Prv, Rev, t):
    Pub = mh.sets(m, Prv, Rev)[0]
    return dict(ch=prng(seed, 0) % R, rnd=[prng(seed, 10 + k, 32) for k in range(mh.rnd_count(m, Prv, Rev, t))], lam=[prng(seed, 100 + k) % R for k in range(t)],
                es=[prng(seed, 200 + k) % R for k in range(t)], a_S=[[prng(seed, 300 + 40 * k + ii) % R for ii in range(len(Prv))] for k in range(t)],
                pub_a=[prng(seed, 400 + k) % R for k in range(len(Pub))])


# every shape and party count whose base list the entry accepts
RESPONSE_SHAPES = [(m, Prv, Rev, t) for m, Prv, Rev in SHAPES[:9] + [(32, (0, 2), (1,))] for t in (1, 3, 4, 8)
                   if len(mh.sets(m, Prv, Rev)[1]) + (t - 1) * len(Prv) <= 32]


@pytest.mark.parametrize("m,Prv,Rev,t", RESPONSE_SHAPES)
def test_responses_prng(sim, m, Prv, Rev, t):
    for j in range(4):
        responses(sim, m, Prv, Rev, t, **_lane(8800 + j, m, Prv, Rev, t))


def test_responses_corner_values(sim):
    """r = 0 (every ch r term vanishes), r and ch at r - 1 (ch r wraps), lambda = 0, e = 0 (-0 = 0), a = 0, randomness at r and 2^256 - 1 (reduced first)"""
    m, Prv, Rev, t = 4, (0, 2), (1,), 3
    corners = (0, 1, R - 1, R, (1 << 256) - 1)
    base = lambda: _lane(8900, m, Prv, Rev, t)
    for pos in range(mh.rnd_count(m, Prv, Rev, t)):
        for v in corners:
            ln = base()
            ln["rnd"][pos] = v
            responses(sim, m, Prv, Rev, t, **ln)
    for v in (0, 1, R - 1):
        for name in ("lam", "es", "pub_a"):
            for k in range(len(base()[name])):
                ln = base()
                ln[name][k] = v
                responses(sim, m, Prv, Rev, t, **ln)
        for k in range(t):
            for ii in range(2):
                ln = base()
                ln["a_S"][k][ii] = v
                responses(sim, m, Prv, Rev, t, **ln)
        ln = base()
        ln["ch"] = v
        responses(sim, m, Prv, Rev, t, **ln)
        ln["rnd"][0] = v                                                   # ch = r = R - 1: the product wraps
        responses(sim, m, Prv, Rev, t, **ln)
    for v in (0, R - 1):                                                   # the same corner everywhere
        ln = base()
        ln = dict(ch=v, rnd=[v] * len(ln["rnd"]), lam=[v] * t, es=[v] * t, a_S=[[v, v] for _ in range(t)], pub_a=[v, v])
        responses(sim, m, Prv, Rev, t, **ln)
