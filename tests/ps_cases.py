"""Shared inputs and expected values of the PS wire / aggregate tests (test_gpu_ps_wire.py, test_gpu_ps_aggregate.py): keys, messages,
signatures made as examples/ps/src/ps.cpp signs them — with Python integers for the scalars and the CPU oracle for every point — and the
verdicts of verify as the oracle's pair_eq gives them.  Nothing here touches the library under test."""
import hashlib

from g1_torsion import dec, ec_add, eigenpoint, enc
from util import P, R, golden, prng

HASH, ENCODE = 0, 1
G1 = bytes.fromhex(golden("g1")["generator"])
G2 = bytes.fromhex(golden("g2")["generator"])
T3 = (0, 2)                                        # a point of order 3
T_CORNERS = (0, 1, R - 1, R, (1 << 256) - 1)


def b32(k):
    return (k % (1 << 256)).to_bytes(32, "big")


def rec(b, w, j):
    return b[w * j:w * j + w]


def messages(seed, n, length):
    return [prng(seed, j, max(length, 1)).to_bytes(max(length, 1), "big")[:length] for j in range(n)]


def msg_scalars(orc, mode, msg):
    """the message scalars of one message as integers: hash(message).to(Zp), or the units of encode_to<Zp>"""
    if mode == HASH:
        d = hashlib.sha3_512(msg).digest()
        return [int.from_bytes(orc.zp_from_hash(d), "big")]
    e = orc.encode_to_zp(msg)
    return [int.from_bytes(e[32 * i:32 * i + 32], "big") for i in range(len(e) // 32)]


class Keys:
    """x, y_1..y_nY below r; g2 = G2^a, X2 = g2^x, Y2_i = g2^y_i as 192-byte and as 97-byte records"""

    def __init__(self, orc, nY, seed):
        self.nY = nY
        self.x = prng(seed, 0) % R
        self.y = [prng(seed, 1 + i) % R for i in range(nY)]
        self.g2 = orc.g2_mul(G2, b32(prng(seed, 1000) % R), 192, 1)
        self.X2 = orc.g2_mul(self.g2, b32(self.x), 192, 1)
        self.Y2 = b"".join(orc.g2_mul(self.g2, b32(v), 192, 1) for v in self.y)
        self.g2_97, self.X2_97, self.Y2_97 = (orc.g2_compress(v) for v in (self.g2, self.X2, self.Y2))

    def x48(self):
        return self.x.to_bytes(48, "big")

    def y48(self):
        return b"".join(v.to_bytes(48, "big") for v in self.y)

    def exponent(self, m):
        return (self.x + sum(yi * mi for yi, mi in zip(self.y, m))) % R


def sign_points(orc, keys, ms, ts):
    """(s1, s2) as 96-byte columns: s1_j = G^t_j, s2_j = s1_j^e_j (ps.cpp:21-23, :79-81), multiply by the oracle"""
    n = len(ts)
    s1 = orc.g1_mul(G1 * n, b"".join(b32(t) for t in ts), 96, 8)
    s2 = orc.g1_mul(s1, b"".join(b32(keys.exponent(m)) for m in ms), 96, 8)
    return s1, s2


def to_wire(orc, s1, s2):
    """serialize(σ1, σ2): n x 98 bytes"""
    n = len(s1) // 96
    c1, c2 = orc.g1_compress(s1), orc.g1_compress(s2)
    return b"".join(rec(c1, 49, j) + rec(c2, 49, j) for j in range(n))


def no_point_x():
    """an x with no point on the curve"""
    x = 5
    while pow((x ** 3 + 4) % P, (P - 1) // 2, P) == 1:
        x += 1
    return x


def mixed_wire_lanes(orc, sigs, msgs, msg_len):
    """tamper the first lanes of a batch of valid signatures; returns (sigs, msgs, kinds)"""
    n = len(msgs)
    sig = [bytearray(rec(sigs, 98, j)) for j in range(n)]
    msgs = list(msgs)
    kinds = ["valid"] * n
    te, _ = eigenpoint(10177)

    def add_to_s1(j, t):
        p96 = orc.g1_decompress(bytes(sig[j][:49]))[0]
        sig[j][:49] = orc.g1_compress(enc(ec_add(dec(p96), t)))
    k = 0
    for kind in ("wrong_msg", "swapped", "s1_inf_junk", "both_inf", "s1_t3", "s1_eigen", "x_ge_p", "x_ge_p_s2", "bad_tag", "bad_tag_s2", "no_point", "no_point_s2"):
        j = 2 * k + 1                                           # odd lanes, valid lanes between them
        k += 1
        kinds[j] = kind
        if kind == "wrong_msg":
            if msg_len:
                msgs[j] = bytes([msgs[j][0] ^ 1]) + msgs[j][1:]
            else:
                sig[j][49:] = sig[j - 1][49:]                   # an empty message cannot be wrong: another lane's σ2
        elif kind == "swapped":
            sig[j][:49], sig[j][49:] = sig[j][49:], sig[j][:49]
        elif kind == "s1_inf_junk":
            sig[j][0] = 0
        elif kind == "both_inf":
            sig[j][0] = 0
            sig[j][49:] = bytes(49)
        elif kind == "s1_t3":
            add_to_s1(j, T3)
        elif kind == "s1_eigen":
            add_to_s1(j, te)
        elif kind in ("x_ge_p", "x_ge_p_s2"):
            o = 0 if kind == "x_ge_p" else 49
            sig[j][o + 1:o + 49] = (int.from_bytes(sig[j][o + 1:o + 49], "big") + P).to_bytes(48, "big")
        elif kind in ("bad_tag", "bad_tag_s2"):
            sig[j][0 if kind == "bad_tag" else 49] = 5
        else:
            o = 0 if kind == "no_point" else 49
            sig[j][o:o + 49] = b"\x02" + no_point_x().to_bytes(48, "big")
    return b"".join(bytes(s) for s in sig), msgs, kinds


def expected_wire(orc, mode, g2_97, X2_97, Y2_97, sigs, msgs):
    """verify(pk, msg_j, sig_j) per lane from the oracle: decode, W = X2 + sum m_i Y2_i, pair_eq(σ1, W, σ2, g2); 0xff where a σ does not decode"""
    n = len(msgs)
    ms = [msg_scalars(orc, mode, m) for m in msgs]
    units = len(ms[0])
    g2, st0 = orc.g2_decompress(g2_97)
    X2, st1 = orc.g2_decompress(X2_97)
    Y2, st2 = orc.g2_decompress(Y2_97[:97 * units])
    assert st0 == b"\x01" and st1 == b"\x01" and st2 == b"\x01" * units
    s1, a = orc.g1_decompress(b"".join(rec(sigs, 98, j)[:49] for j in range(n)))
    s2, b = orc.g1_decompress(b"".join(rec(sigs, 98, j)[49:] for j in range(n)))
    W = X2 * n
    for i in range(units):
        W = orc.g2_add(W, orc.g2_mul(rec(Y2, 192, i) * n, b"".join(b32(m[i]) for m in ms), 192, 8), 192)
    ok = orc.pair_eq(s1, W, s2, g2 * n, 8)
    return bytes(ok[j] if a[j] and b[j] else 0xff for j in range(n))
