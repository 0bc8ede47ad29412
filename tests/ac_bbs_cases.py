"""Builders for the AC-bbs tests (the reference's examples/AC-bbs): keygen, issue and pres as the reference writes them — scalars from
util.prng, points by the CPU oracle (g1_mul = PAIR_G1mul, g1_add, compression, pair), c by hashlib's SHA3-512 mod r — and the expected
results of the library's entries composed independently from the same primitives:
    expected_verify   verify.cpp:6-26 from the wire bytes, with op.mul(B_, c) on the left side of the Schnorr equation
    expected_pres     pres.cpp:6-42 from the wire bytes and the caller's randomness
tests/test_ac_bbs_cases.py checks the builders against themselves on the CPU; the GPU tests compare the library with them."""
import hashlib

from g1_torsion import P as FP, eigenpoint, enc as enc96, point_of_order
from util import R, cat, golden, prng

G1GEN = bytes.fromhex(golden("g1")["generator"])
G2GEN = bytes.fromhex(golden("g2")["generator"])
MSG_LEN = 32


def b32(k):
    return (k % R).to_bytes(32, "big")


def b48(k):
    return k.to_bytes(48, "big")


class Ops:
    """the group operations of the reference on 96-byte affine G1 points / 192-byte G2 points, by the CPU oracle"""

    def __init__(self, orc):
        self.o = orc

    def mul(self, p, k):                       # multiply (PAIR_G1mul), k reduced mod r
        return self.o.g1_mul(p, b32(k), 96)

    def add(self, a, b):
        return self.o.g1_add(a, b, 96)

    def enc(self, a):
        return self.o.g1_compress(a)

    def dec(self, c49):
        pt, st = self.o.g1_decompress(c49)
        return pt, st[0] != 0

    def g2mul(self, q, k):
        return self.o.g2_mul(q, b32(k), 192)

    def g2dec(self, c97):
        pt, st = self.o.g2_decompress(c97)
        return pt, st[0] != 0

    def prod(self, start, bases, scalars):
        """start * prod_i bases[i]^scalars[i]; start = None: the empty product is infinity"""
        acc = bytes(96) if start is None else start
        for b, k in zip(bases, scalars):
            acc = self.add(acc, self.mul(b, k))
        return acc


def hidden(nattr, I):
    return [i for i in range(nattr) if i not in I]


def challenge(op, msg, A_, B_, U):
    """hash(m, A_, B_, U).to(Zp): the message bytes, then the three points as serialize writes them"""
    return int.from_bytes(hashlib.sha3_512(msg + op.enc(A_) + op.enc(B_) + op.enc(U)).digest(), "big") % R


class Key:
    """keygen (keygen.cpp): g, tilde_g, x, tilde_X = tilde_g^x, Y_0 .. Y_(n-1); g, Y entries and tilde_X may be replaced (points outside G1 / G2)"""

    def __init__(self, op, seed, nattr, g=None, Y=None, tilde_X=None):
        s = lambda i: prng(seed, i) % R
        self.nattr = nattr
        self.g = op.mul(G1GEN, s(0)) if g is None else g
        self.tilde_g = op.g2mul(G2GEN, s(1))
        self.x = s(2)
        self.tilde_X = op.g2mul(self.tilde_g, self.x) if tilde_X is None else tilde_X
        self.Y = [op.mul(G1GEN, s(10 + i)) for i in range(nattr)]
        for i, y in (Y or {}).items():
            self.Y[i] = y
        self.pk = op.enc(self.g) + op.o.g2_compress(self.tilde_g) + op.o.g2_compress(self.tilde_X)
        self.Y49 = b"".join(op.enc(y) for y in self.Y)


def attributes(seed, nattr):
    return [prng(seed, i) % R for i in range(nattr)]


def issue(op, key, a, seed, w=None):
    """issue.cpp: A = (g * prod Y_i^a_i)^inverse(x + w); serialize(A, w)"""
    w = (prng(seed, 0) % (R - 1) + 1) if w is None else w
    inv = pow((key.x + w) % R, -1, R) if (key.x + w) % R else 0
    A = op.mul(op.prod(key.g, key.Y, a), inv)
    return op.enc(A) + b48(w)


def draw(seed, nJ):
    """the 3 + nJ scalars pres draws: r, alpha, beta, delta_0 .."""
    return [prng(seed, i) % R for i in range(3 + nJ)]


def pres(op, key, msg, a, A, w, I, rnd, w_used=None):
    """pres.cpp:6-42 on parsed values: A a 96-byte point, a and w integers below r, rnd = [r, alpha, beta, delta_0 ..] reduced mod r.
    w_used: another w in B_ and t — a presentation whose Schnorr half holds while the pairing half fails."""
    J = hidden(key.nattr, I)
    r, alpha, beta, delta = rnd[0] % R, rnd[1] % R, rnd[2] % R, [d % R for d in rnd[3:]]
    w = w if w_used is None else w_used
    C_I = op.prod(key.g, [key.Y[i] for i in I], [a[i] for i in I])
    C_J = op.prod(None, [key.Y[j] for j in J], [a[j] for j in J])
    A_ = op.mul(A, r)
    B_ = op.add(op.mul(op.add(C_I, C_J), r), op.mul(A_, -w))
    U = op.prod(op.add(op.mul(C_I, alpha), op.mul(A_, beta)), [key.Y[j] for j in J], delta)
    c = challenge(op, msg, A_, B_, U)
    s = (alpha + r * c) % R
    t = (beta + (-w % R) * c) % R
    u = [(delta[k] + r * c * a[J[k]]) % R for k in range(len(J))]
    return op.enc(A_) + op.enc(B_) + op.enc(U) + b48(s) + b48(t), b"".join(b48(v) for v in u)


def _parse_pk(op, pk, Y49):
    g, ok = op.dec(pk[:49])
    tg, ok1 = op.g2dec(pk[49:146])
    tX, ok2 = op.g2dec(pk[146:243])
    Y = [op.dec(Y49[49 * i:49 * i + 49]) for i in range(len(Y49) // 49)]
    if not (ok and ok1 and ok2 and all(y[1] for y in Y)):
        return None
    return g, tg, tX, [y[0] for y in Y]


def _fields(b, count):
    return [int.from_bytes(b[48 * i:48 * i + 48], "big") for i in range(count)]


def expected_verify(op, pk, Y49, I, pres243, u48, attr48, msg):
    """verify.cpp:6-26 composed from the oracle on the wire bytes; attr48: the disclosed values in the order of I.  0xff where the
    reference would throw, None when pk does not decode."""
    pub = _parse_pk(op, pk, Y49)
    if pub is None:
        return None
    g, tg, tX, Y = pub
    J = hidden(len(Y), I)
    pts = []
    for k in range(3):
        pt, ok = op.dec(pres243[49 * k:49 * k + 49])
        if not ok:
            return 0xff
        pts.append(pt)
    A_, B_, U = pts
    s, t = _fields(pres243[147:], 2)
    u, a = _fields(u48, len(J)), _fields(attr48, len(I))
    if any(v >= R for v in [s, t] + u + a):
        return 0xff
    c = challenge(op, msg, A_, B_, U)
    if op.o.pair(A_, tX) != op.o.pair(B_, tg):
        return 0
    K = op.prod(g, [Y[i] for i in I], a)
    left = op.add(U, op.mul(B_, c))
    right = op.prod(op.add(op.mul(K, s), op.mul(A_, t)), [Y[j] for j in J], u)
    return 1 if left == right else 0


def expected_pres(op, key, I, attr48, sig97, msg, rnd):
    """pres from the wire bytes: (PresInfo.fixed_part, PresInfo.u, status); rnd: (3 + nJ) x 32 bytes, any values.  Where the reference would
    throw — A does not decode, w or an attribute >= r — status 0xff and records of 0xff."""
    nJ = key.nattr - len(I)
    a, (w,) = _fields(attr48, key.nattr), _fields(sig97[49:], 1)
    A, ok = op.dec(sig97[:49])
    if not ok or w >= R or any(v >= R for v in a):
        return b"\xff" * 243, b"\xff" * (48 * nJ), 0xff
    vals = [int.from_bytes(rnd[32 * i:32 * i + 32], "big") for i in range(3 + nJ)]
    p, u = pres(op, key, msg, a, A, w, I, vals)
    return p, u, 0


# ---------------------------------------------------------------- lanes of the main shape: nattr = 4, I = (0, 3), 32-byte messages
NATTR, I_MAIN = 4, (0, 3)


def off_curve_x():
    x = 5
    while pow((x ** 3 + 4) % FP, (FP - 1) // 2, FP) == 1:
        x += 1
    return b"\x02" + x.to_bytes(48, "big")


class Lane:
    def __init__(self, kind, msg, pres243, u48, attr48):
        self.kind, self.msg, self.pres, self.u, self.attr = kind, msg, pres243, u48, attr48


def message(seed, i, msg_len=MSG_LEN):
    return prng(seed, i, msg_len).to_bytes(msg_len, "big") if msg_len else b""


def valid_lanes(op, key, I, count, seed, msg_len=MSG_LEN):
    """`count` honest presentations under key with the disclosure set I"""
    out = []
    nJ = key.nattr - len(I)
    for i in range(count):
        a = attributes(seed + 1000 + i, key.nattr)
        sig = issue(op, key, a, seed + 2000 + i)
        msg = message(seed, i, msg_len)
        p, u = pres(op, key, msg, a, op.dec(sig[:49])[0], int.from_bytes(sig[49:], "big"), I, draw(seed + 3000 + i, nJ))
        out.append(Lane("valid", msg, p, u, b"".join(b48(a[k]) for k in I)))
    return out


def _with(lane, kind, **kw):
    d = dict(msg=lane.msg, pres243=lane.pres, u48=lane.u, attr48=lane.attr)
    d.update(kw)
    return Lane(kind, d["msg"], d["pres243"], d["u48"], d["attr48"])


def _field(b, i, value, base=0):
    return b[:base + 48 * i] + value.to_bytes(48, "big") + b[base + 48 * i + 48:]


def _plus1(b, i, base=0):
    return _field(b, i, (int.from_bytes(b[base + 48 * i:base + 48 * i + 48], "big") + 1) % R, base)


def main_lanes(op, key):
    """valid, tampered, degenerate, off-subgroup and malformed lanes of the main shape, with their kinds"""
    I, nJ = I_MAIN, NATTR - len(I_MAIN)
    lanes = valid_lanes(op, key, I, 12, 5100)
    b, b1 = lanes[0], lanes[1]
    a = attributes(5100 + 1000, NATTR)                                   # lane 0's attributes, signature and draw again
    sig = issue(op, key, a, 5100 + 2000)
    A, w = op.dec(sig[:49])[0], int.from_bytes(sig[49:], "big")
    rnd = draw(5100 + 3000, nJ)
    mk = lambda kind, p_u, msg=b.msg: Lane(kind, msg, p_u[0], p_u[1], b.attr)
    # tampered
    lanes.append(_with(b, "flipped msg", msg=bytes([b.msg[0] ^ 1]) + b.msg[1:]))
    lanes.append(_with(b, "s+1", pres243=_plus1(b.pres, 0, 147)))
    lanes.append(_with(b, "t+1", pres243=_plus1(b.pres, 1, 147)))
    lanes.append(_with(b, "u0+1", u48=_plus1(b.u, 0)))
    lanes.append(_with(b, "a+1", attr48=_plus1(b.attr, 1)))
    lanes.append(_with(b, "U swapped", pres243=b.pres[:98] + b1.pres[98:147] + b.pres[147:]))
    A_, B_ = op.dec(b.pres[:49])[0], op.dec(b.pres[49:98])[0]
    lanes.append(_with(b, "A_ B_ scaled", pres243=op.enc(op.mul(A_, 7)) + op.enc(op.mul(B_, 7)) + b.pres[98:]))
    lanes.append(mk("pairing only fails", pres(op, key, b.msg, a, A, w, I, rnd, w_used=(w + 1) % R)))
    # degenerate
    lanes.append(mk("A at infinity", pres(op, key, b.msg, a, bytes(96), w, I, rnd)))
    r0 = pres(op, key, b.msg, a, A, w, I, [0] + rnd[1:])
    lanes.append(mk("r = 0", r0))
    assert r0[0][0] == 0 and r0[0][49] == 0
    lanes.append(mk("leading 00 + bytes", (b"\x00" + bytes(range(1, 49)) + r0[0][49:], r0[1])))
    x_big = int.from_bytes(A_[:48], "big") + FP                          # x >= p, same point
    lanes.append(_with(b, "x >= p", pres243=b.pres[:1] + x_big.to_bytes(48, "big") + b.pres[49:]))
    lanes.append(_with(b, "s = t = 0", pres243=_field(_field(b.pres, 0, 0, 147), 1, 0, 147)))
    lanes.append(_with(b, "u = 0", u48=bytes(48 * nJ)))
    # off the subgroup: a negated scalar in place of a negated point shows here
    t3 = enc96(point_of_order(3))
    te, _ = eigenpoint(10177)
    lanes.append(_with(b, "B_ + order 3", pres243=b.pres[:49] + op.enc(op.add(B_, t3)) + b.pres[98:]))
    lanes.append(_with(b, "A_ eigenpoint", pres243=op.enc(enc96(te)) + b.pres[49:]))
    # malformed
    lanes.append(_with(b, "U off curve", pres243=b.pres[:98] + off_curve_x() + b.pres[147:]))
    lanes.append(_with(b, "B_ bad tag", pres243=b.pres[:49] + b"\x05" + b.pres[50:]))
    lanes.append(_with(b, "t = r", pres243=_field(b.pres, 1, R, 147)))
    lanes.append(_with(b, "u1 = 2^384 - 1", u48=_field(b.u, 1, (1 << 384) - 1)))
    return lanes


VALID_KINDS = ("valid",)
ZERO_KINDS = ("flipped msg", "s+1", "t+1", "u0+1", "a+1", "U swapped", "A_ B_ scaled", "pairing only fails", "s = t = 0", "u = 0")
BAD_KINDS = ("U off curve", "B_ bad tag", "t = r", "u1 = 2^384 - 1")


def expect(op, key, I, lanes):
    """the expected byte of every lane"""
    return bytes(expected_verify(op, key.pk, key.Y49, I, ln.pres, ln.u, ln.attr, ln.msg) for ln in lanes)


def pack(lanes):
    """(pres_243, u_48, attr_48, msgs) of a list of lanes as the entry takes them"""
    return (b"".join(ln.pres for ln in lanes), b"".join(ln.u for ln in lanes), b"".join(ln.attr for ln in lanes), b"".join(ln.msg for ln in lanes))


def g2_outside():
    return cat(golden("g2")["offsubgroup_points"])[:192]
