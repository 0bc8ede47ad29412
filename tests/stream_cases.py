"""Two valid batches per _dev entry of include/c12381_hip.h and include/c12381_ac.h, for the stream-contract tests (tests/test_gpu_stream_contract.py;
premises that need no GPU: tests/test_stream_cases.py).  A row names the entry and builds its argument list — in the typed form of
tests/test_gpu_api_contract.py::_entries (In, OptIn, Out, Fmt, Op, K, Count, ...), plus Idx for the HOST index array of the credential entries — for
a lane count n and a variant v: v = 0 is batch A, v = 1 batch B, another valid batch of the same shapes under other keys, points, scalars and
messages.  The rows with a verdict output hold really signed / really equal lanes, some of them tampered, so that the expected bytes of A are mixed
and a call that read B's tables, keys or lanes would not reproduce them.

Expected bytes, by `source`:
    "integers"   Python integers / hashlib
    "oracle"     the CPU oracle's primitives (oracle/c12381_oracle.c), composed here
    "builders"   the case builders of the feature suites (bbs_cases, ps_cases, test_gpu_bbs04[_sign], ac_*_cases), which compose the oracle
No row takes its expected bytes from the library under test.  Nothing here touches the library."""
import hashlib

import ac_bbs_cases as ab
import ac_rbbs_cases as arb
import ac_rps_cases as arp
import bbs_cases as bc
import ps_cases as pc
from test_gpu_api_contract import Count, Flags, Fmt, In, K, NH, Op, OptIn, Out   # noqa: F401  (the typed form is theirs)
from util import P as P_MOD, R, golden, prng, scalars

G1GEN = bytes.fromhex(golden("g1")["generator"])[:96]
G2GEN = bytes.fromhex(golden("g2")["generator"])[:192]
N = 5                                   # lanes of A and B
NMSG = 2                                # nmsg / nY / k / nb
NATTR, I_SET = 4, (0, 3)
MSG_LEN = 40                            # two 31-byte units
BIG = 1 << 15                           # the first size whose window segments are sorted on two streams


class Idx(tuple):
    """the disclosure set of a credential entry: a HOST array of uint32_t in both forms, read before anything is launched"""


class Row:
    """id; host and _dev name; build(orc, n, v) -> (args, want, status): the arguments after the context, the expected bytes of every Out in order,
    the status c12381_sync returns; source of `want`; verdict: an Out holds per-lane verdicts, both kinds in A; unread: {argument index: reason}
    for the inputs the entry's documentation says the output does not depend on; pipelined: part of the back-to-back test (side-stream forks,
    shared key workspaces)"""

    def __init__(self, id, host, build, source, verdict=False, unread=None, pipelined=False, n=N):
        self.id, self.host, self.dev, self.build, self.source = id, host, host + "_dev", build, source
        self.verdict, self.unread, self.pipelined, self.n = verdict, unread or {}, pipelined, n


_CACHE = {}


def case(orc, row, n=None, v=0):
    """(args, want, status) of row for n lanes (default: the row's) and variant v, built once"""
    n = row.n if n is None else n
    key = (row.id, n, v)
    if key not in _CACHE:
        _CACHE[key] = row.build(orc, n, v)
    return _CACHE[key]


def ins(args):
    return [(i, a) for i, a in enumerate(args) if isinstance(a, In)]


# ---------------------------------------------------------------- inputs
def _seed(v, k=0):
    return 7100 + 1000 * v + 10 * k


def g1pts(orc, seed, n):
    return orc.g1_mul(G1GEN * n, scalars(seed, n), 96, 8)


def g2pts(orc, seed, n):
    return orc.g2_mul(G2GEN * n, scalars(seed, n), 192, 8)


def _rec(b, w, j):
    return b[w * j:w * j + w]


def _g1sum(orc, cols, fmt):
    """lane-wise sum of equally long columns of 96-byte points"""
    acc = cols[0]
    for c in cols[1:]:
        acc = orc.g1_add(acc, c, 96)
    return orc.g1_add(acc, bytes(len(acc)), fmt)


def _g2sum(orc, cols, fmt):
    acc = cols[0]
    for c in cols[1:]:
        acc = orc.g2_add(acc, c, 192)
    return orc.g2_add(acc, bytes(len(acc)), fmt)


def _gts(orc, seed, n):
    return orc.pair(g1pts(orc, seed, n), g2pts(orc, seed + 1, n), 8)


def _gt_one(orc):
    return orc.pair(bytes(96), G2GEN)


def _tampered(n, v):
    """the lanes of a verdict row that are made to fail: 1 and 3 (of every 5) in A, 0 and 2 in B"""
    return [j for j in range(n) if j % 5 in ((1, 3) if v == 0 else (0, 2))]


# ---------------------------------------------------------------- field and scalar rows
def _fp_mul(orc, n, v):
    a = [prng(_seed(v), j) % P_MOD for j in range(n)]
    b = [prng(_seed(v, 1), j) % P_MOD for j in range(n)]
    enc = lambda xs: b"".join(x.to_bytes(48, "big") for x in xs)
    return [Op(0), n, In(enc(a)), In(enc(b)), Out(48 * n)], [enc([x * y % P_MOD for x, y in zip(a, b)])], 0


def _zp(op):
    def build(orc, n, v):
        a, b = scalars(_seed(v), n), scalars(_seed(v, 1), n)
        ai = [int.from_bytes(_rec(a, 32, j), "big") for j in range(n)]
        bi = [int.from_bytes(_rec(b, 32, j), "big") for j in range(n)]
        out = [x * y % R for x, y in zip(ai, bi)] if op == 0 else [pow(x, R - 2, R) for x in ai]
        return [Op(op), n, In(a), In(b) if op == 0 else OptIn(b), Out(32 * n)], [b"".join(x.to_bytes(32, "big") for x in out)], 0
    return build


def _zp_inner(orc, n, v):
    a, b = scalars(_seed(v), n), scalars(_seed(v, 1), n)
    s = sum(int.from_bytes(_rec(a, 32, j), "big") * int.from_bytes(_rec(b, 32, j), "big") for j in range(n)) % R
    return [n, In(a), OptIn(b), Out(32)], [s.to_bytes(32, "big")], 0


def _sha3(orc, n, v):
    msgs = pc.messages(_seed(v), n, MSG_LEN)
    return [n, MSG_LEN, In(b"".join(msgs)), Out(64 * n)], [b"".join(hashlib.sha3_512(m).digest() for m in msgs)], 0


def _from_hash(orc, n, v):
    d = b"".join(hashlib.sha3_512(m).digest() for m in pc.messages(_seed(v), n, MSG_LEN))
    return [n, In(d), Out(96 * n), Fmt(96)], [orc.g1_from_hash(d, 96)], 0


# ---------------------------------------------------------------- G1
def _g1_mul(orc, n, v):
    p, sc = g1pts(orc, _seed(v), n), scalars(_seed(v, 1), n)
    return [n, In(p), In(sc), Out(49 * n), Fmt(49)], [orc.g1_mul(p, sc, 49, 8)], 0


def _g1_mul_flags(orc, n, v):
    p, sc = g1pts(orc, _seed(v), n), scalars(_seed(v, 1), n)
    return [n, In(orc.g1_compress(p)), In(sc), Out(96 * n), Fmt(96), Flags(4)], [orc.g1_mul(p, sc, 96, 8)], 0


def _msm_terms(orc, n, v):
    """random points of G1 and full-size scalars; in A, term 2 is G + T3 (T3 of order 3, outside G1) under the scalar 77: the one entry of the
    small-scalar bucket, whose [r]phi(S) the bucket product forms on the side stream — B's bucket is empty, so a term formed from B's ranges is
    missing from the product (tests/msm_cases.py "f:one-small-among-large/G+T3"; the oracle's g1_msm evaluates multiply() term by term)"""
    p, sc = g1pts(orc, _seed(v), n), scalars(_seed(v, 1), n)
    if v == 0:
        from g1_torsion import enc, point_of_order
        p = p[:192] + orc.g1_add(G1GEN, enc(point_of_order(3)), 96) + p[288:]
        sc = sc[:64] + (77).to_bytes(32, "big") + sc[96:]
    return p, sc


def _g1_msm(orc, n, v):
    p, sc = _msm_terms(orc, n, v)
    return [n, In(p), In(sc), Out(49), Fmt(49)], [orc.g1_msm(p, sc, 49, 8)], 0


def generator_multiples(orc, seed, n):
    """n = 2^k points g^(s_i) with their logs: 64 from the oracle's multiply, then the set doubled k - 6 times by adding one more multiple of g to
    every point it holds (2^k - 64 oracle additions instead of 2^k multiplications; the logs are kept as integers)"""
    assert n >= 64 and n & (n - 1) == 0
    logs = [prng(seed, j) % R for j in range(64)]
    pts = orc.g1_mul(G1GEN * 64, b"".join(s.to_bytes(32, "big") for s in logs), 96, 8)
    k = 0
    while len(logs) < n:
        d = prng(seed + 1, k) % R
        k += 1
        pts += orc.g1_add(pts, orc.g1_mul(G1GEN, d.to_bytes(32, "big"), 96) * len(logs), 96)
        logs += [(s + d) % R for s in logs]
    return pts, logs


def _g1_msm_big(orc, n, v):
    """the generator-multiple identity of tests/test_gpu_full_size.py: sum k_i g^(s_i) = g^(sum s_i k_i)"""
    p, logs = generator_multiples(orc, _seed(v), n)
    sc = scalars(_seed(v, 1), n)
    e = sum(s * int.from_bytes(_rec(sc, 32, j), "big") for j, s in enumerate(logs)) % R
    return [n, In(p), In(sc), Out(49), Fmt(49)], [orc.g1_mul(G1GEN, e.to_bytes(32, "big"), 49)], 0


def _g1_msm_flags(orc, n, v):
    p, sc = _msm_terms(orc, n, v)
    return [n, In(orc.g1_compress(p)), In(sc), Out(96), Fmt(96), Flags(4)], [orc.g1_msm(p, sc, 96, 8)], 0


def _g1_sum(orc, n, v):
    p = g1pts(orc, _seed(v), n)
    return [n, In(p), Out(49), Fmt(49)], [_g1sum(orc, [_rec(p, 96, j) for j in range(n)], 49)], 0


def _g1_sop(orc, n, v):
    p, sc = g1pts(orc, _seed(v), n), scalars(_seed(v, 1), n)
    return [n, In(p), In(sc), Out(96), Fmt(96)], [orc.g1_sum_of_products(p, sc, 96)], 0


def _g1_mul_sum(orc, n, v):
    p, sc = g1pts(orc, _seed(v), NMSG * n), scalars(_seed(v, 1), NMSG * n)
    prod = orc.g1_mul(p, sc, 96, 8)
    return ([n, Count(NMSG, (0, 5)), In(p), In(sc), Out(49 * n), Fmt(49), Flags(0)],
            [_g1sum(orc, [prod[96 * n * i:96 * n * (i + 1)] for i in range(NMSG)], 49)], 0)


def _g1_mul_fixed(orc, n, v):
    base, sc = g1pts(orc, _seed(v), 1), scalars(_seed(v, 1), n)
    return [n, In(base), In(sc), Out(49 * n), Fmt(49)], [orc.g1_mul(base * n, sc, 49, 8)], 0


def _g1_fixed_sum(orc, n, v):
    pts, sc = g1pts(orc, _seed(v), NMSG + 1), scalars(_seed(v, 1), NMSG * n)
    bases, addend = pts[:96 * NMSG], pts[96 * NMSG:]
    cols = [orc.g1_mul(_rec(bases, 96, i) * n, sc[32 * n * i:32 * n * (i + 1)], 96, 8) for i in range(NMSG)]
    return [n, Count(NMSG, (0, 33)), In(bases), OptIn(addend), In(sc), Out(49 * n), Fmt(49)], [_g1sum(orc, cols + [addend * n], 49)], 0


# ---------------------------------------------------------------- G2
def _g2_mul(orc, n, v):
    q, sc = g2pts(orc, _seed(v), n), scalars(_seed(v, 1), n)
    return [n, In(q), In(sc), Out(97 * n), Fmt(97)], [orc.g2_mul(q, sc, 97, 8)], 0


def _g2_mul_flags(orc, n, v):
    q, sc = g2pts(orc, _seed(v), n), scalars(_seed(v, 1), n)
    return [n, In(orc.g2_compress(q)), In(sc), Out(192 * n), Fmt(192), Flags(4)], [orc.g2_mul(q, sc, 192, 8)], 0


def _g2_msm(orc, n, v):
    q, sc = g2pts(orc, _seed(v), n), scalars(_seed(v, 1), n)
    prod = orc.g2_mul(q, sc, 192, 8)
    return [n, In(q), OptIn(sc), Out(97), Fmt(97)], [_g2sum(orc, [_rec(prod, 192, j) for j in range(n)], 97)], 0


def _g2_mul_fixed(orc, n, v):
    base, sc = g2pts(orc, _seed(v), 1), scalars(_seed(v, 1), n)
    return [n, In(base), In(sc), Out(97 * n), Fmt(97)], [orc.g2_mul(base * n, sc, 97, 8)], 0


def _g2_fixed_sum(orc, n, v):
    pts, sc = g2pts(orc, _seed(v), NMSG + 1), scalars(_seed(v, 1), NMSG * n)
    bases, addend = pts[:192 * NMSG], pts[192 * NMSG:]
    cols = [orc.g2_mul(_rec(bases, 192, i) * n, sc[32 * n * i:32 * n * (i + 1)], 192, 8) for i in range(NMSG)]
    return [n, Count(NMSG, (0, 33)), In(bases), OptIn(addend), In(sc), Out(97 * n), Fmt(97)], [_g2sum(orc, cols + [addend * n], 97)], 0


def _decompress(g):
    def build(orc, n, v):
        if g == 1:
            p = g1pts(orc, _seed(v), n)
            c, (out, st) = orc.g1_compress(p), orc.g1_decompress(orc.g1_compress(p))
        else:
            p = g2pts(orc, _seed(v), n)
            c, (out, st) = orc.g2_compress(p), orc.g2_decompress(orc.g2_compress(p))
        assert out == p
        return [n, In(c), Out(len(p)), Out(n)], [out, st], 0
    return build


# ---------------------------------------------------------------- pairings and GT
def _pair(orc, n, v):
    p, q = g1pts(orc, _seed(v), n), g2pts(orc, _seed(v, 1), n)
    return [n, In(p), In(q), Out(576 * n)], [orc.pair(p, q, 8)], 0


def _pair_flags(orc, n, v):
    p, q = g1pts(orc, _seed(v), n), g2pts(orc, _seed(v, 1), n)
    return [n, In(orc.g1_compress(p)), In(orc.g2_compress(q)), Out(576 * n), Flags(4)], [orc.pair(p, q, 8)], 0


def _pair_product(orc, n, v):
    p, q = g1pts(orc, _seed(v), NMSG * n), g2pts(orc, _seed(v, 1), NMSG * n)
    e = orc.pair(p, q, 8)
    return [n, K(NMSG), In(p), In(q), Out(576 * n), Flags(0)], [orc.gt_op("mul", e[:576 * n], e[576 * n:])], 0


def _pair_eq(orc, n, v):
    """e(s P, Q) against e(P, s Q) on scalar multiples of the golden points; the tampered lanes take (s + 1) Q"""
    P = [bytes.fromhex(h) for h in golden("g1")["points"]]
    Q = [bytes.fromhex(h) for h in golden("g2")["points"]]
    b1 = b"".join(P[(j + 3 * v) % len(P)] for j in range(n))
    a2 = b"".join(Q[(j + 2 * v) % len(Q)] for j in range(n))
    s = [prng(_seed(v), j) % R for j in range(n)]
    bad = _tampered(n, v)
    a1 = orc.g1_mul(b1, b"".join(x.to_bytes(32, "big") for x in s), 96, 8)
    b2 = orc.g2_mul(a2, b"".join(((x + (j in bad)) % R).to_bytes(32, "big") for j, x in enumerate(s)), 192, 8)
    return [n, In(a1), In(a2), In(b1), In(b2), Out(n)], [orc.pair_eq(a1, a2, b1, b2, 8)], 0


def _miller(orc, n, v):
    p, q = g1pts(orc, _seed(v), n), g2pts(orc, _seed(v, 1), n)
    return [n, In(p), In(q), Out(576 * n)], [orc.miller(p, q)], 0


def _fexp(orc, n, v):
    f = orc.miller(g1pts(orc, _seed(v), n), g2pts(orc, _seed(v, 1), n))
    return [n, In(f), Out(576 * n)], [orc.fexp(f)], 0


def _gt_op(op):
    def build(orc, n, v):
        if op == 3:
            a = orc.miller(g1pts(orc, _seed(v), n), g2pts(orc, _seed(v, 1), n))
        else:
            a = _gts(orc, _seed(v), n)
        b = scalars(_seed(v, 2), n) if op == 2 else _gts(orc, _seed(v, 3), n)
        want = orc.fexp(a) if op == 3 else orc.gt_op({0: "mul", 1: "conj", 2: "pow"}[op], a, b)
        return [Op(op), n, In(a), In(b) if op in (0, 2) else OptIn(b), Out(576 * n)], [want], 0
    return build


def _gt_is_unity(orc, n, v):
    e, one = _gts(orc, _seed(v), n), _gt_one(orc)
    ones = _tampered(n, 1 - v)
    a = b"".join(one if j in ones else _rec(e, 576, j) for j in range(n))
    return [n, In(a), Out(n)], [bytes(1 if j in ones else 0 for j in range(n))], 0


def _pair_fixed(orc, n, v):
    p, q = g1pts(orc, _seed(v), n), g2pts(orc, _seed(v, 1), 1)
    return [n, In(p), In(q), Out(576 * n)], [orc.pair(p, q * n, 8)], 0


def _pair_product_fixed(orc, n, v):
    p, q = g1pts(orc, _seed(v), NMSG * n), g2pts(orc, _seed(v, 1), NMSG)
    e = [orc.pair(p[96 * n * i:96 * n * (i + 1)], _rec(q, 192, i) * n, 8) for i in range(NMSG)]
    return [n, Count(NMSG, (0, 9)), In(p), In(q), Out(576 * n), Flags(0)], [orc.gt_op("mul", e[0], e[1])], 0


# ---------------------------------------------------------------- PS
def _ps_batch(orc, n, v, bad):
    """keys, message scalars (lists per lane), s1, s2 of n signatures; the lanes in `bad` carry the s2 of their neighbour"""
    keys = pc.Keys(orc, NMSG, _seed(v))
    ms = [[prng(_seed(v, 1) + i, j) % R for i in range(NMSG)] for j in range(n)]
    s1, s2 = pc.sign_points(orc, keys, ms, [prng(_seed(v, 3), j) % (R - 1) + 1 for j in range(n)])
    s2 = b"".join(_rec(s2, 96, (j + 1) % n if j in bad else j) for j in range(n))
    m = b"".join(pc.b32(ms[j][i]) for i in range(NMSG) for j in range(n))
    W = keys.X2 * n
    for i in range(NMSG):
        W = orc.g2_add(W, orc.g2_mul(_rec(keys.Y2, 192, i) * n, m[32 * n * i:32 * n * (i + 1)], 192, 8), 192)
    return keys, s1, s2, m, orc.pair_eq(s1, W, s2, keys.g2 * n, 8)


def _ps_verify(orc, n, v):
    keys, s1, s2, m, ok = _ps_batch(orc, n, v, _tampered(n, v))
    return [n, NMSG, In(keys.g2), In(keys.X2), In(keys.Y2), In(s1), In(s2), In(m), Out(n)], [ok], 0


def _ps_aggregate(orc, n, v):
    """A: every lane valid, verdict 1; B: one forged lane, verdict 0"""
    keys, s1, s2, m, ok = _ps_batch(orc, n, v, [2] if v else [])
    assert ok == bytes(0 if v and j == 2 else 1 for j in range(n))
    rho = scalars(_seed(v, 4), n, 1 << 64)
    return [n, NMSG, In(keys.g2), In(keys.X2), In(keys.Y2), In(s1), In(s2), In(m), In(rho), Out(4)], [bytes([0 if v else 1, 0, 0, 0])], 0


def _ps_wire_batch(orc, mode, n, v):
    nY = NMSG if mode == pc.ENCODE else 1
    keys = pc.Keys(orc, nY, _seed(v))
    msgs = pc.messages(_seed(v, 1), n, MSG_LEN)
    ts = [prng(_seed(v, 2), j) % (R - 1) + 1 for j in range(n)]
    return nY, keys, msgs, ts


def _ps_verify_wire(mode):
    def build(orc, n, v):
        nY, keys, msgs, ts = _ps_wire_batch(orc, mode, n, v)
        sigs = pc.to_wire(orc, *pc.sign_points(orc, keys, [pc.msg_scalars(orc, mode, m) for m in msgs], ts))
        for j in _tampered(n, v):                                             # signed, then the message changed
            msgs[j] = bytes([msgs[j][0] ^ 1]) + msgs[j][1:]
        want = pc.expected_wire(orc, mode, keys.g2_97, keys.X2_97, keys.Y2_97, sigs, msgs)
        return ([n, Count(nY, (1,) if mode else (2,)), MSG_LEN, Count(mode, (2,)), In(keys.g2_97), In(keys.X2_97), In(keys.Y2_97), In(sigs),
                 In(b"".join(msgs)), Out(n)], [want], 0)
    return build


def _ps_sign(mode):
    def build(orc, n, v):
        from test_gpu_ps_wire import sign_want
        nY, keys, msgs, ts = _ps_wire_batch(orc, mode, n, v)
        want, _ = sign_want(orc, mode, keys.x, keys.y, msgs, ts)
        return ([n, Count(nY, (1,) if mode else (2,)), MSG_LEN, Count(mode, (2,)), In(keys.x48()), In(keys.y48()), In(b"".join(msgs)),
                 In(b"".join(pc.b32(t) for t in ts)), Out(98 * n)], [want], 0)
    return build


def _ps_randomize(orc, n, v):
    nY, keys, msgs, ts = _ps_wire_batch(orc, pc.ENCODE, n, v)
    s1, s2 = pc.sign_points(orc, keys, [pc.msg_scalars(orc, pc.ENCODE, m) for m in msgs], ts)
    sigs, r = pc.to_wire(orc, s1, s2), scalars(_seed(v, 3), n)
    o1, o2 = orc.g1_mul(s1, r, 49, 8), orc.g1_mul(s2, r, 49, 8)
    return [n, In(sigs), In(r), Out(98 * n), Out(n)], [b"".join(_rec(o1, 49, j) + _rec(o2, 49, j) for j in range(n)), bytes(n)], 0


# ---------------------------------------------------------------- BBS+
def _bbs_lanes(orc, n, v, bad):
    p = bc.Params(orc, _seed(v), NMSG)
    lanes = bc.valid_lanes(p, n, _seed(v, 1))
    for j in bad:
        lanes[j].x = (lanes[j].x + 5) % R                                     # "wrong x" of bbs_cases.lanes
    return p, lanes


def _bbs_verify(orc, n, v):
    p, lanes = _bbs_lanes(orc, n, v, _tampered(n, v))
    g1, g2, h0, h, w = p.public()
    A, x, r, m = bc.pack(lanes)
    return [n, NMSG, In(g1), In(g2), In(h0), In(h), In(w), In(A), In(x), In(r), In(m), Out(n)], [bc.expect(p, lanes)], 0


def _bbs_aggregate(orc, n, v):
    """A: every lane valid, verdict 1; B: one lane with a wrong x, verdict 0"""
    p, lanes = _bbs_lanes(orc, n, v, [2] if v else [])
    assert bc.expect(p, lanes) == bytes(0 if v and j == 2 else 1 for j in range(n))
    g1, g2, h0, h, w = p.public()
    A, x, r, m = bc.pack(lanes)
    return ([n, NMSG, In(g1), In(g2), In(h0), In(h), In(w), In(A), In(x), In(r), In(m), In(scalars(_seed(v, 4), n, 1 << 64)), Out(4)],
            [bytes([0 if v else 1, 0, 0, 0])], 0)


def _bbs_wire(orc, n, v):
    p = bc.Params(orc, _seed(v), NMSG)
    wl = bc.wire_lanes(p, MSG_LEN)
    good = [ln for ln in wl if ln.kind == "valid"]
    bad = [ln for ln in wl if ln.kind in ("wrong message", "wrong x", "wrong r", "-A")]
    t = _tampered(n, v)
    sel = [bad[j % len(bad)] if j in t else good[j % len(good)] for j in range(n)]
    sig, msgs = bc.wire_pack(sel)
    pub, h49, pk = bc.wire_public(p)
    return [n, NH(NMSG), MSG_LEN, In(pub), In(h49), In(pk), In(sig), In(msgs), Out(n)], [bc.wire_expect(p, sel, MSG_LEN)], 0


def _bbs_sign(orc, n, v):
    p, lanes = _bbs_lanes(orc, n, v, [])
    _, x, r, m = bc.pack(lanes)
    return [n, NMSG, In(p.g1), In(p.h0), In(p.h), In(bc.b32(p.gamma)), In(x), In(r), In(m), Out(96 * n)], [bc.sign_expect(p, lanes)], 0


# ---------------------------------------------------------------- bbs04
def _bbs04(orc, n, v):
    import test_gpu_bbs04 as b4
    op = b4.Ops(orc)
    k = b4.Keys(op, _seed(v))
    msgs = pc.messages(_seed(v, 1), n, MSG_LEN)
    return b4, op, k, msgs


def _bbs04_verify(orc, n, v):
    b4, op, k, msgs = _bbs04(orc, n, v)
    sigs = [b4.sign(op, k, j % 3, msgs[j], _seed(v, 2) + j) for j in range(n)]
    for j in _tampered(n, v):
        msgs[j] = bytes([msgs[j][0] ^ 1]) + msgs[j][1:]
    want = bytes(b4.expected_verify(op, k.gpk, sigs[j], msgs[j]) for j in range(n))
    return [n, MSG_LEN, In(k.gpk), In(b"".join(sigs)), In(b"".join(msgs)), Out(n)], [want], 0


def _bbs04_open(orc, n, v):
    """really signed lanes of three members; the expected bytes are the members' A (a lane with a status other than 0 has unspecified bytes)"""
    b4, op, k, msgs = _bbs04(orc, n, v)
    sigs = [b4.sign(op, k, j % 3, msgs[j], _seed(v, 2) + j) for j in range(n)]
    want = [b4.expected_open(op, k.gmsk, s) for s in sigs]
    assert all(st == 0 for _, st in want) and [a for a, _ in want] == [op.enc(k.members[j % 3][0]) for j in range(n)]
    return [n, In(k.gmsk), In(b"".join(sigs)), Out(49 * n), Out(n)], [b"".join(a for a, _ in want), bytes(n)], 0


def _bbs04_sign(orc, n, v):
    import test_gpu_bbs04_sign as s4
    b4, op, k, msgs = _bbs04(orc, n, v)
    lanes = [(s4.gsk_of(op, k, j % 3), msgs[j], s4.seed_rnd(_seed(v, 2) + j)) for j in range(n)]
    gsk, mm, rnd = s4.pack(lanes)
    return ([n, MSG_LEN, In(k.gpk), In(gsk), In(mm), In(rnd), Out(435 * n), Out(n)],
            [b"".join(s4.model_sign(op, k, *ln) for ln in lanes), bytes(n)], 0)


def _bbs04_issue(orc, n, v):
    import test_gpu_bbs04_sign as s4
    b4, op, k, _ = _bbs04(orc, n, v)
    xs = [prng(_seed(v, 3), j) % R for j in range(n)]
    return ([n, In(k.gpk), In(k.gamma.to_bytes(32, "big")), In(b"".join(x.to_bytes(32, "big") for x in xs)), Out(97 * n)],
            [s4.expected_issue(op, k, k.gamma, xs)], 0)


# ---------------------------------------------------------------- credentials
def _tamper_attr(mod, lanes, bad):
    return [mod._with(ln, "a+1", attr48=mod._plus1(ln.attr, 1)) if j in bad else ln for j, ln in enumerate(lanes)]


def _ac_bbs_verify(orc, n, v):
    op = ab.Ops(orc)
    key = ab.Key(op, _seed(v), NATTR)
    lanes = _tamper_attr(ab, ab.valid_lanes(op, key, I_SET, n, _seed(v, 1), MSG_LEN), _tampered(n, v))
    pres, u, attr, msgs = ab.pack(lanes)
    return ([n, NATTR, len(I_SET), Idx(I_SET), MSG_LEN, In(key.pk), In(key.Y49), In(pres), In(u), In(attr), In(msgs), Out(n)],
            [ab.expect(op, key, I_SET, lanes)], 0)


def _ac_bbs_pres(orc, n, v):
    op = ab.Ops(orc)
    key = ab.Key(op, _seed(v), NATTR)
    nJ = NATTR - len(I_SET)
    attr = [b"".join(ab.b48(a) for a in ab.attributes(_seed(v, 1) + j, NATTR)) for j in range(n)]
    sigs = [ab.issue(op, key, ab.attributes(_seed(v, 1) + j, NATTR), _seed(v, 2) + j) for j in range(n)]
    msgs = [ab.message(_seed(v, 3), j, MSG_LEN) for j in range(n)]
    rnd = [scalars(_seed(v, 4) + j, 3 + nJ) for j in range(n)]
    want = [ab.expected_pres(op, key, I_SET, attr[j], sigs[j], msgs[j], rnd[j]) for j in range(n)]
    return ([n, NATTR, len(I_SET), Idx(I_SET), MSG_LEN, In(key.pk), In(key.Y49), In(b"".join(attr)), In(b"".join(sigs)), In(b"".join(msgs)),
             In(b"".join(rnd)), Out(243 * n), Out(48 * nJ * n), Out(n)],
            [b"".join(w[0] for w in want), b"".join(w[1] for w in want), bytes(w[2] for w in want)], 0)


def _ac_rbbs_verify(orc, n, v):
    op = ab.Ops(orc)
    key = arb.Key(op, _seed(v), NATTR)
    lanes = _tamper_attr(arb, arb.valid_lanes(op, key, I_SET, n, _seed(v, 1), MSG_LEN), _tampered(n, v))
    pres, attr, msgs = arb.pack(lanes)
    return ([n, NATTR, len(I_SET), Idx(I_SET), MSG_LEN, In(key.pk), In(key.Y49), In(key.tY97), In(pres), In(attr), In(msgs), Out(n)],
            [arb.expect(op, key, I_SET, lanes)], 0)


def _ac_rbbs_creds(orc, n, v):
    op = ab.Ops(orc)
    key = arb.Key(op, _seed(v), NATTR)
    return op, key, [arb.Cred(op, key, I_SET, _seed(v, 1), j, MSG_LEN) for j in range(n)]


def _ac_rbbs_pres(orc, n, v):
    op, key, cr = _ac_rbbs_creds(orc, n, v)
    rnd = [b"".join(ab.b32(x) for x in c.rnd) for c in cr]
    want = [arb.expected_pres(op, c.sig, c.cache, c.msg, r) for c, r in zip(cr, rnd)]
    return ([n, MSG_LEN, In(b"".join(c.sig for c in cr)), In(b"".join(c.cache for c in cr)), In(b"".join(c.msg for c in cr)), In(b"".join(rnd)),
             Out(341 * n), Out(n)], [b"".join(w[0] for w in want), bytes(w[1] for w in want)], 0)


def _ac_rbbs_redact(orc, n, v):
    op, key, cr = _ac_rbbs_creds(orc, n, v)
    want = [arb.expected_redact(op, key.pk, key.Y49, NATTR, I_SET, c.attr_all, c.sig) for c in cr]
    return ([n, NATTR, len(I_SET), Idx(I_SET), In(key.pk), In(key.Y49), In(b"".join(c.attr_all for c in cr)), In(b"".join(c.sig for c in cr)),
             Out(196 * n), Out(n)], [b"".join(w[0] for w in want), bytes(w[1] for w in want)], 0)


def _ac_rps_verify(orc, n, v):
    op = ab.Ops(orc)
    key = arp.Key(op, _seed(v), NATTR)
    lanes = _tamper_attr(arp, arp.valid_lanes(op, key, I_SET, n, _seed(v, 1)), _tampered(n, v))
    pres, attr = arp.pack(lanes)
    return ([n, NATTR, len(I_SET), Idx(I_SET), In(key.pk), In(key.Y49), In(key.tY97), In(pres), In(attr), Out(n)],
            [arp.expect(op, key, I_SET, lanes)], 0)


def _ac_rps_creds(orc, n, v):
    op = ab.Ops(orc)
    key = arp.Key(op, _seed(v), NATTR)
    return op, key, [arp.Cred(op, key, I_SET, _seed(v, 1), j) for j in range(n)]


def _ac_rps_pres(orc, n, v):
    op, key, cr = _ac_rps_creds(orc, n, v)
    want = [arp.expected_pres(op, key.pk, key.Y49, NATTR, I_SET, c.attr_all, c.sig, c.cache, c.usk, c.rnd96) for c in cr]
    return ([n, NATTR, len(I_SET), Idx(I_SET), In(key.pk), In(key.Y49), In(b"".join(c.attr_all for c in cr)), In(b"".join(c.sig for c in cr)),
             In(b"".join(c.cache for c in cr)), In(b"".join(c.usk for c in cr)), In(b"".join(c.rnd96 for c in cr)), Out(389 * n), Out(n)],
            [b"".join(w[0] for w in want), bytes(w[1] for w in want)], 0)


def _ac_rps_redact(orc, n, v):
    op, key, cr = _ac_rps_creds(orc, n, v)
    want = [arp.expected_redact(op, key.tY97, NATTR, I_SET, c.attr_all, c.sig) for c in cr]
    return ([n, NATTR, len(I_SET), Idx(I_SET), In(key.tY97), In(b"".join(c.attr_all for c in cr)), In(b"".join(c.sig for c in cr)), Out(97 * n),
             Out(n)], [b"".join(w[0] for w in want), bytes(w[1] for w in want)], 0)


# ---------------------------------------------------------------- the table
_UNARY = "a unary op ignores b (include/c12381_hip.h); passed non-NULL all the same"
_RHO = "rho only weights the lanes: the verdict of a batch whose lanes all verify is 1 for every rho"

ROWS = [
    Row("fp_op[mul]", "fp_op_batch", _fp_mul, "integers"),
    Row("g1_mul", "g1_mul_batch", _g1_mul, "oracle"),
    Row("g1_mul_flags", "g1_mul_batch_flags", _g1_mul_flags, "oracle"),
    Row("g1_mul_sum", "g1_mul_sum_batch", _g1_mul_sum, "oracle"),
    Row("g1_msm", "g1_msm", _g1_msm, "oracle", pipelined=True),
    Row("g1_msm[2^15]", "g1_msm", _g1_msm_big, "oracle", pipelined=True, n=BIG),
    Row("g1_msm_flags", "g1_msm_flags", _g1_msm_flags, "oracle"),
    Row("g1_sum", "g1_sum", _g1_sum, "oracle"),
    Row("g1_sum_of_products", "g1_sum_of_products", _g1_sop, "oracle"),
    Row("g2_mul", "g2_mul_batch", _g2_mul, "oracle"),
    Row("g2_mul_flags", "g2_mul_batch_flags", _g2_mul_flags, "oracle"),
    Row("g2_msm", "g2_msm", _g2_msm, "oracle"),
    Row("pair", "pair_batch", _pair, "oracle"),
    Row("pair_flags", "pair_batch_flags", _pair_flags, "oracle"),
    Row("pair_product", "pair_product_batch", _pair_product, "oracle"),
    Row("pair_eq", "pair_eq_batch", _pair_eq, "oracle", verdict=True),
    Row("g1_decompress", "g1_decompress_batch", _decompress(1), "oracle"),
    Row("g2_decompress", "g2_decompress_batch", _decompress(2), "oracle"),
    Row("miller", "miller_batch", _miller, "oracle"),
    Row("fexp", "fexp_batch", _fexp, "oracle"),
    Row("gt_op[mul]", "gt_op_batch", _gt_op(0), "oracle"),
    Row("gt_op[conj]", "gt_op_batch", _gt_op(1), "oracle", unread={3: _UNARY}),
    Row("gt_op[pow]", "gt_op_batch", _gt_op(2), "oracle"),
    Row("gt_op[fexp]", "gt_op_batch", _gt_op(3), "oracle", unread={3: _UNARY}),
    Row("gt_is_unity", "gt_is_unity_batch", _gt_is_unity, "oracle", verdict=True),
    Row("pair_fixed_g2", "pair_fixed_g2_batch", _pair_fixed, "oracle"),
    Row("pair_product_fixed_g2", "pair_product_fixed_g2_batch", _pair_product_fixed, "oracle"),
    Row("ps_verify", "ps_verify_batch", _ps_verify, "oracle", verdict=True),
    Row("g1_mul_fixed", "g1_mul_fixed_batch", _g1_mul_fixed, "oracle"),
    Row("g2_mul_fixed", "g2_mul_fixed_batch", _g2_mul_fixed, "oracle"),
    Row("g1_mul_fixed_sum", "g1_mul_fixed_sum_batch", _g1_fixed_sum, "oracle", pipelined=True),
    Row("g2_mul_fixed_sum", "g2_mul_fixed_sum_batch", _g2_fixed_sum, "oracle", pipelined=True),
    Row("bbs_plus_verify", "bbs_plus_verify_batch", _bbs_verify, "builders", verdict=True, pipelined=True),
    Row("bbs_plus_verify_aggregate", "bbs_plus_verify_aggregate", _bbs_aggregate, "builders", unread={11: _RHO}, pipelined=True),
    Row("bbs_plus_verify_wire", "bbs_plus_verify_wire_batch", _bbs_wire, "builders", verdict=True, pipelined=True),
    Row("bbs_plus_sign", "bbs_plus_sign_batch", _bbs_sign, "builders"),
    Row("g1_from_hash", "g1_from_hash_batch", _from_hash, "oracle"),
    Row("zp_op[mul]", "zp_op_batch", _zp(0), "integers"),
    Row("zp_op[inv]", "zp_op_batch", _zp(4), "integers", unread={3: _UNARY}),
    Row("zp_inner_product", "zp_inner_product", _zp_inner, "integers"),
    Row("sha3_512", "sha3_512_batch", _sha3, "integers"),
    Row("bbs04_verify", "bbs04_verify_batch", _bbs04_verify, "builders", verdict=True, pipelined=True),
    Row("bbs04_open", "bbs04_open_batch", _bbs04_open, "builders"),
    Row("bbs04_sign", "bbs04_sign_batch", _bbs04_sign, "builders", pipelined=True),
    Row("bbs04_issue", "bbs04_issue_batch", _bbs04_issue, "builders", pipelined=True),
    Row("ps_verify_wire[encode]", "ps_verify_wire_batch", _ps_verify_wire(pc.ENCODE), "builders", verdict=True, pipelined=True),
    Row("ps_verify_wire[hash]", "ps_verify_wire_batch", _ps_verify_wire(pc.HASH), "builders", verdict=True, pipelined=True),
    Row("ps_sign[encode]", "ps_sign_batch", _ps_sign(pc.ENCODE), "builders", pipelined=True),
    Row("ps_sign[hash]", "ps_sign_batch", _ps_sign(pc.HASH), "builders", pipelined=True),
    Row("ps_randomize", "ps_randomize_batch", _ps_randomize, "oracle"),
    Row("ps_verify_aggregate", "ps_verify_aggregate", _ps_aggregate, "oracle", unread={8: _RHO}),
    Row("ac_bbs_verify", "ac_bbs_verify_batch", _ac_bbs_verify, "builders", verdict=True, pipelined=True),
    Row("ac_bbs_pres", "ac_bbs_pres_batch", _ac_bbs_pres, "builders", pipelined=True),
    Row("ac_rbbs_verify", "ac_rbbs_verify_batch", _ac_rbbs_verify, "builders", verdict=True, pipelined=True),
    Row("ac_rbbs_pres", "ac_rbbs_pres_batch", _ac_rbbs_pres, "builders", pipelined=True),
    Row("ac_rbbs_redact", "ac_rbbs_redact_batch", _ac_rbbs_redact, "builders", pipelined=True),
    Row("ac_rps_verify", "ac_rps_verify_batch", _ac_rps_verify, "builders", verdict=True, pipelined=True),
    Row("ac_rps_pres", "ac_rps_pres_batch", _ac_rps_pres, "builders", pipelined=True),
    Row("ac_rps_redact", "ac_rps_redact_batch", _ac_rps_redact, "builders", pipelined=True),
]
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)

# _dev names of the two headers that have no row, each with its reason
NO_CASE = {
    "fp_mulchain_dev": "benchmark kernel of the Fp leaf: no host form, no bytes anyone relies on",
}
