"""c12381_bbs04_verify_batch / c12381_bbs04_open_batch: bbs04 group signatures (the reference's examples/bbs04/src/bbs.cpp) from the wire
formats.  Keys and signatures are made here as key_gen and sign make them (scalars from util.prng, points by the CPU oracle, c by hashlib's
SHA3-512 mod r); the expected byte of every lane is verify / open composed independently from the oracle's primitives (g1_mul = PAIR_G1mul,
g1_add, pair, GT multiplication, compression).  Edge lanes: tampered fields, T at infinity, a T with a leading 0x00 and bytes behind it, an
x >= p, T outside G1 (order 3, eigenpoint), zero scalars, empty messages, T off the curve and Zp fields >= r (0xff), gpk with w at infinity
or outside G2 (the generic route of the k = 2 product), an undecodable gpk (every lane 0xff, C12381_E_POINT)."""
import hashlib

import pytest

from g1_torsion import P as FP, eigenpoint, enc, point_of_order
from util import R, cat, golden, prng

pytestmark = pytest.mark.gpu

G1GEN = bytes.fromhex(golden("g1")["generator"])
G2GEN = bytes.fromhex(golden("g2")["generator"])
MSG_LEN = 32


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


def _b32(k):
    return (k % R).to_bytes(32, "big")


def _b48(k):
    return k.to_bytes(48, "big")


class Ops:
    """the group operations of the reference on 96-byte affine G1 points / 192-byte G2 points, by the CPU oracle"""

    def __init__(self, orc):
        self.o = orc

    def mul(self, p, k):                       # multiply (PAIR_G1mul), k reduced mod r
        return self.o.g1_mul(p, _b32(k), 96)

    def add(self, a, b):
        return self.o.g1_add(a, b, 96)

    def neg(self, a):
        if a == bytes(96):
            return a
        return a[:48] + ((FP - int.from_bytes(a[48:], "big")) % FP).to_bytes(48, "big")

    def enc(self, a):
        return self.o.g1_compress(a)

    def dec(self, c49):
        pt, st = self.o.g1_decompress(c49)
        return pt, st[0] != 0

    def g2mul(self, q, k):
        return self.o.g2_mul(q, _b32(k), 192)

    def pair2(self, p1, q1, p2, q2):
        return self.o.gt_op("mul", self.o.pair(p1, q1), self.o.pair(p2, q2))


def _hash(op, msg, T, Rs, R3):
    """hash(message, T1, T2, T3, R1, R2, R3, R4, R5).to(Zp)"""
    tr = msg + b"".join(op.enc(t) for t in T) + op.enc(Rs[0]) + op.enc(Rs[1]) + R3 + op.enc(Rs[2]) + op.enc(Rs[3])
    return int.from_bytes(hashlib.sha3_512(tr).digest(), "big") % R


class Keys:
    def __init__(self, op, seed, gamma=None, w=None):
        s = lambda i: prng(seed, i) % R
        self.g1 = op.mul(G1GEN, s(0))
        self.h = op.mul(G1GEN, s(1))
        self.g2 = op.g2mul(G2GEN, s(2))
        self.xi1, self.xi2 = s(3), s(4)
        self.gamma = s(5) if gamma is None else gamma
        self.u = op.mul(self.h, pow(self.xi1, -1, R))
        self.v = op.mul(self.h, pow(self.xi2, -1, R))
        self.w = op.g2mul(self.g2, self.gamma) if w is None else w
        self.gpk = (op.enc(self.g1) + op.o.g2_compress(self.g2) + op.enc(self.h) + op.enc(self.u) + op.enc(self.v)
                    + op.o.g2_compress(self.w))
        self.gmsk = _b48(self.xi1) + _b48(self.xi2)
        self.members = []
        for i in range(3):
            x = s(10 + i)
            inv = pow((self.gamma + x) % R, -1, R) if (self.gamma + x) % R else 0
            self.members.append((op.mul(self.g1, inv), x))


def sign(op, k, member, msg, seed, alpha=None, beta=None):
    """sign (bbs.cpp:33-59) with the random scalars drawn from prng(seed, .); alpha / beta may be forced (0: T1 / T2 at infinity)"""
    A, x = k.members[member]
    s = lambda i: prng(seed, i) % R
    a = s(0) if alpha is None else alpha
    b = s(1) if beta is None else beta
    ra, rb, rx, rd1, rd2 = (s(2 + i) for i in range(5))
    T1, T2 = op.mul(k.u, a), op.mul(k.v, b)
    T3 = op.add(A, op.mul(k.h, a + b))
    R1, R2 = op.mul(k.u, ra), op.mul(k.v, rb)
    R3 = op.pair2(op.add(op.mul(T3, rx), op.mul(k.h, -(rd1 + rd2))), k.g2, op.mul(k.h, -(ra + rb)), k.w)
    R4 = op.add(op.mul(T1, rx), op.mul(k.u, -rd1))
    R5 = op.add(op.mul(T2, rx), op.mul(k.v, -rd2))
    c = _hash(op, msg, (T1, T2, T3), (R1, R2, R4, R5), R3)
    cx = c * x % R
    fields = [c, (ra + c * a) % R, (rb + c * b) % R, (rx + cx) % R, (rd1 + a * cx) % R, (rd2 + b * cx) % R]
    return op.enc(T1) + op.enc(T2) + op.enc(T3) + b"".join(_b48(f) for f in fields)


def expected_verify(op, gpk, sig, msg):
    """verify (bbs.cpp:61-78) composed from the oracle; 0xff where the reference would terminate, None when gpk does not decode"""
    pub = []
    for off, ln in ((0, 49), (49, 97), (146, 49), (195, 49), (244, 49), (293, 97)):
        if ln == 49:
            pt, ok = op.dec(gpk[off:off + 49])
        else:
            pt, st = op.o.g2_decompress(gpk[off:off + 97])
            ok = st[0] != 0
        if not ok:
            return None
        pub.append(pt)
    g1, g2, h, u, v, w = pub
    T = []
    for k in range(3):
        pt, ok = op.dec(sig[49 * k:49 * k + 49])
        if not ok:
            return 0xff
        T.append(pt)
    f = [int.from_bytes(sig[147 + 48 * i:195 + 48 * i], "big") for i in range(6)]
    if any(x >= R for x in f):
        return 0xff
    c, sa, sb, sx, sd1, sd2 = f
    T1, T2, T3 = T
    R1 = op.add(op.mul(u, sa), op.mul(T1, -c))
    R2 = op.add(op.mul(v, sb), op.mul(T2, -c))
    P1 = op.add(op.add(op.mul(T3, sx), op.mul(h, (-sd1) + (-sd2))), op.neg(op.mul(g1, c)))
    P2 = op.add(op.mul(h, -(sa + sb)), op.mul(T3, c))
    R3 = op.pair2(P1, g2, P2, w)
    R4 = op.add(op.mul(T1, sx), op.mul(u, -sd1))
    R5 = op.add(op.mul(T2, sx), op.mul(v, -sd2))
    return 1 if _hash(op, msg, T, (R1, R2, R4, R5), R3) == c else 0


def expected_open(op, gmsk, sig):
    xi1, xi2 = int.from_bytes(gmsk[:48], "big"), int.from_bytes(gmsk[48:], "big")
    T = []
    for k in range(3):
        pt, ok = op.dec(sig[49 * k:49 * k + 49])
        if not ok:
            return None, 0xff
        T.append(pt)
    if any(int.from_bytes(sig[147 + 48 * i:195 + 48 * i], "big") >= R for i in range(6)):
        return None, 0xff
    a = op.add(T[2], op.neg(op.add(op.mul(T[0], xi1), op.mul(T[1], xi2))))
    return op.enc(a), 0


def _field(sig, i, value):
    return sig[:147 + 48 * i] + value.to_bytes(48, "big") + sig[195 + 48 * i:]


def _off_curve_x():
    x = 5
    while pow((x ** 3 + 4) % FP, (FP - 1) // 2, FP) == 1:
        x += 1
    return b"\x02" + x.to_bytes(48, "big")


@pytest.fixture(scope="module")
def world(oracle_port):
    op = Ops(oracle_port)
    k = Keys(op, 9400)
    msgs, sigs, kinds = [], [], []

    def lane(kind, msg, sig):
        kinds.append(kind); msgs.append(msg); sigs.append(sig)

    m = lambda i: prng(9401, i, MSG_LEN).to_bytes(MSG_LEN, "big")
    for i in range(12):                                              # valid
        lane("valid", m(i), sign(op, k, i % 3, m(i), 9500 + i))
    base_sig, base_msg = sigs[0], msgs[0]
    lane("flipped msg", bytes([base_msg[0] ^ 1]) + base_msg[1:], base_sig)
    for i, name in ((0, "c+1"), (3, "sx+1"), (1, "sa+1"), (5, "sd2+1")):
        lane(name, base_msg, _field(base_sig, i, (int.from_bytes(base_sig[147 + 48 * i:195 + 48 * i], "big") + 1) % R))
    lane("T3 swapped", base_msg, base_sig[:98] + sigs[1][98:147] + base_sig[147:])
    s_inf1 = sign(op, k, 1, m(20), 9600, alpha=0)
    lane("T1 at infinity", m(20), s_inf1)
    lane("T2 at infinity", m(21), sign(op, k, 2, m(21), 9601, beta=0))
    lane("leading 00 + bytes", m(20), b"\x00" + bytes(range(1, 49)) + s_inf1[49:])
    t1 = op.dec(base_sig[:49])[0]
    x_big = int.from_bytes(t1[:48], "big") + FP                          # x >= p, same point
    lane("x >= p", base_msg, base_sig[:1] + x_big.to_bytes(48, "big") + base_sig[49:])
    t3 = enc(point_of_order(3))                                          # outside G1
    te, _ = eigenpoint(10177)
    lane("T1 order 3", base_msg, oracle_port.g1_compress(t3) + base_sig[49:])
    lane("T2 eigenpoint", base_msg, base_sig[:49] + oracle_port.g1_compress(enc(te)) + base_sig[98:])
    lane("T3 + order 3", base_msg, base_sig[:98] + oracle_port.g1_compress(op.add(op.dec(base_sig[98:147])[0], t3)) + base_sig[147:])
    lane("c = 0", base_msg, _field(base_sig, 0, 0))
    lane("sd1 = sd2 = 0", base_msg, _field(_field(base_sig, 4, 0), 5, 0))
    lane("sa = sb = sx = 0", base_msg, _field(_field(_field(base_sig, 1, 0), 2, 0), 3, 0))
    lane("T2 off curve", base_msg, base_sig[:49] + _off_curve_x() + base_sig[98:])
    lane("T3 bad tag", base_msg, base_sig[:98] + b"\x05" + base_sig[99:])
    lane("sb = r", base_msg, _field(base_sig, 2, R))
    lane("sd1 = 2^384 - 1", base_msg, _field(base_sig, 4, (1 << 384) - 1))
    return op, k, msgs, sigs, kinds


def _check(ctx, op, gpk, msgs, sigs, kinds, msg_len=MSG_LEN):
    got = ctx.bbs04_verify(gpk, b"".join(sigs), b"".join(msgs), msg_len)
    want = bytes(expected_verify(op, gpk, s, m) for s, m in zip(sigs, msgs))
    bad = [(kinds[j], got[j], want[j]) for j in range(len(sigs)) if got[j] != want[j]]
    assert not bad, bad
    return want


def test_verify_edge_lanes(ctx, world):
    op, k, msgs, sigs, kinds = world
    want = _check(ctx, op, k.gpk, msgs, sigs, kinds)
    by = dict(zip(kinds, want))
    assert all(w == 1 for kd, w in zip(kinds, want) if kd == "valid")
    for kd in ("T1 at infinity", "T2 at infinity", "leading 00 + bytes", "x >= p"):
        assert by[kd] == 1, kd                                             # re-encoded T's hash like the parsed points
    for kd in ("flipped msg", "c+1", "sx+1", "sa+1", "sd2+1", "T3 swapped", "c = 0"):
        assert by[kd] == 0, kd
    for kd in ("T2 off curve", "T3 bad tag", "sb = r", "sd1 = 2^384 - 1"):
        assert by[kd] == 0xff, kd


def test_verify_other_gpk(ctx, world, oracle_port):
    op, k, msgs, sigs, kinds = world
    k2 = Keys(op, 9410)
    want = _check(ctx, op, k2.gpk, msgs[:12], sigs[:12], kinds[:12])
    assert set(want) == {0}


def test_verify_empty_messages(ctx, world):
    op, k, _, _, _ = world
    sigs = [sign(op, k, i % 3, b"", 9700 + i) for i in range(4)]
    got = ctx.bbs04_verify(k.gpk, b"".join(sigs), b"", 0)
    assert got == b"\x01" * 4
    assert got == bytes(expected_verify(op, k.gpk, s, b"") for s in sigs)


@pytest.mark.parametrize("w_kind", ["infinity", "outside G2"])
def test_verify_generic_route(ctx, oracle_port, w_kind):
    """w at infinity (gamma = 0) or outside G2: the k = 2 product takes its generic route; signatures made under that key"""
    op = Ops(oracle_port)
    if w_kind == "infinity":
        k = Keys(op, 9420, gamma=0)
        assert k.w == bytes(192)
    else:
        k = Keys(op, 9421, w=cat(golden("g2")["offsubgroup_points"])[:192])
    m = [prng(9422, i, MSG_LEN).to_bytes(MSG_LEN, "big") for i in range(4)]
    sigs = [sign(op, k, i % 3, m[i], 9800 + i) for i in range(4)]
    sigs.append(_field(sigs[0], 3, 7))
    want = _check(ctx, op, k.gpk, m + [m[0]], sigs, ["valid"] * 4 + ["sx"])
    assert want[:4] == b"\x01" * 4 if w_kind == "infinity" else True


def test_verify_undecodable_gpk(ctx, world):
    from crypto12381_amd.capi import C12381Error, E_POINT
    op, k, msgs, sigs, kinds = world
    bad = b"\x05" + k.gpk[1:]
    assert expected_verify(op, bad, sigs[0], msgs[0]) is None
    got = ctx.bbs04_verify(bad, b"".join(sigs[:5]), b"".join(msgs[:5]), MSG_LEN, strict=False)
    assert got == b"\xff" * 5
    with pytest.raises(C12381Error) as e:
        ctx.bbs04_verify(bad, b"".join(sigs[:5]), b"".join(msgs[:5]), MSG_LEN)
    assert e.value.code == E_POINT
    assert ctx.bbs04_verify(k.gpk, b"".join(sigs[:2]), b"".join(msgs[:2]), MSG_LEN) == b"\x01\x01"    # the context recovers


def test_verify_arguments(ctx, world):
    from crypto12381_amd.capi import E_ARG
    op, k, msgs, sigs, kinds = world
    lib, ok = ctx.lib, bytearray(1)
    import ctypes
    buf = ctypes.create_string_buffer(1)
    assert lib.c12381_bbs04_verify_batch(ctx.h, 1, MSG_LEN, None, sigs[0], msgs[0], buf) == E_ARG
    assert lib.c12381_bbs04_verify_batch(ctx.h, 1, MSG_LEN, k.gpk, None, msgs[0], buf) == E_ARG
    assert lib.c12381_bbs04_verify_batch(ctx.h, 1, MSG_LEN, k.gpk, sigs[0], None, buf) == E_ARG
    assert lib.c12381_bbs04_verify_batch(ctx.h, 1, MSG_LEN, k.gpk, sigs[0], msgs[0], None) == E_ARG
    assert lib.c12381_bbs04_verify_batch(ctx.h, 0, MSG_LEN, k.gpk, sigs[0], msgs[0], buf) == 0
    assert lib.c12381_bbs04_open_batch(ctx.h, 1, None, sigs[0], buf, buf) == E_ARG


def test_verify_large_tiled_host_and_dev(ctx, world):
    import torch
    op, k, msgs, sigs, kinds = world
    distinct = list(zip(sigs, msgs, kinds))
    extra = [prng(9430, i, MSG_LEN).to_bytes(MSG_LEN, "big") for i in range(64 - len(distinct))]
    for i, mm in enumerate(extra):
        distinct.append((sign(op, k, i % 3, mm, 9900 + i), mm, "valid"))
    want_d = bytes(expected_verify(op, k.gpk, s, m) for s, m, _ in distinct)
    n = 1 << 16
    idx = [(j * 37) % 64 for j in range(n)]
    sig_all = b"".join(distinct[i][0] for i in idx)
    msg_all = b"".join(distinct[i][1] for i in idx)
    want = bytes(want_d[i] for i in idx)
    assert ctx.bbs04_verify(k.gpk, sig_all, msg_all, MSG_LEN) == want
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    d_gpk, d_sig, d_msg = dev(k.gpk), dev(sig_all), dev(msg_all)
    d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.bbs04_verify_dev(n, MSG_LEN, d_gpk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), d_ok.data_ptr())
    assert ctx.sync() == 0
    assert bytes(d_ok.cpu().numpy().tobytes()) == want


def test_open(ctx, world):
    op, k, msgs, sigs, kinds = world
    out, st = ctx.bbs04_open(k.gmsk, b"".join(sigs))
    for j, (s, kd) in enumerate(zip(sigs, kinds)):
        a, status = expected_open(op, k.gmsk, s)
        assert st[j] == status, kd
        if status == 0:
            assert out[49 * j:49 * j + 49] == a, kd
    for j, kd in enumerate(kinds):
        if kd == "valid":
            assert out[49 * j:49 * j + 49] == op.enc(k.members[j % 3][0])          # the signer's A_i


def test_open_dev_and_bad_gmsk(ctx, world):
    import torch
    from crypto12381_amd.capi import C12381Error, E_ARG
    op, k, msgs, sigs, kinds = world
    n = 1 << 12
    sig_all = b"".join(sigs[j % 12] for j in range(n))
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    d_g, d_s = dev(k.gmsk), dev(sig_all)
    d_out = torch.zeros(49 * n, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.bbs04_open_dev(n, d_g.data_ptr(), d_s.data_ptr(), d_out.data_ptr(), d_st.data_ptr())
    assert ctx.sync() == 0
    out = bytes(d_out.cpu().numpy().tobytes())
    assert bytes(d_st.cpu().numpy().tobytes()) == bytes(n)
    assert all(out[49 * j:49 * j + 49] == op.enc(k.members[(j % 12) % 3][0]) for j in range(n))
    bad = k.gmsk[:48] + R.to_bytes(48, "big")
    out, st = ctx.bbs04_open(bad, b"".join(sigs[:3]), strict=False)
    assert st == b"\xff" * 3
    with pytest.raises(C12381Error) as e:
        ctx.bbs04_open(bad, b"".join(sigs[:3]))
    assert e.value.code == E_ARG
