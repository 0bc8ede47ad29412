"""Builders for the AC-rbbs tests (the reference's examples/AC-rbbs): keygen, issue, redact and pres as the reference writes them — scalars from
util.prng, points by the CPU oracle through ac_bbs_cases.Ops (multiply = PAIR_G1mul / PAIR_G2mul, add, compression, pair), c and the q_i by
hashlib's SHA3-512 mod r — and the expected results of the library's entries composed independently from the same primitives:
    expected_verify   verify.cpp:6-24 from the wire bytes: three equations, only the used records of pk.Y / pk.tilde_Y decoded
    expected_pres     pres.cpp:6-27 from the wire bytes and the caller's randomness
    expected_redact   redact.cpp:7-44 from the wire bytes, D over exactly the k the reference's filter keeps
tests/test_ac_rbbs_cases.py checks the builders against themselves on the CPU; the GPU tests compare the library with them."""
import hashlib

from ac_bbs_cases import MSG_LEN, G1GEN, G2GEN, Ops, _field, _fields, _plus1, attributes, b32, b48, g2_outside, hidden, message, off_curve_x  # noqa: F401
from g1_torsion import P as FP, eigenpoint, enc as enc96, point_of_order
from util import R, prng

# (nattr, I) of the GPU tests; redact takes nattr <= 16
SHAPES = [(1, ()), (1, (0,)), (2, (1,)), (2, (0,)), (4, (3, 0)), (4, ()), (4, (0, 1, 2, 3)), (16, (0, 3))]
VERIFY_ONLY_SHAPES = [(32, (0, 3)), (32, (0, 3, 5, 9, 17, 30, 31))]         # nI + 1 = 3 and 8: the product; SUM_SHAPE: the G2 sum
SUM_SHAPE = (32, (0, 3, 5, 9, 17, 29, 30, 31))                              # nI + 1 = 9 > C12381_FIXED_G2_MAX
NATTR, I_MAIN = 4, (0, 3)


def q_of(aI, i):
    """hash(a[j] (j.in(I)), i).to(Zp): the disclosed values as 48-byte fields in the order of I, then the size_t i, little-endian"""
    return int.from_bytes(hashlib.sha3_512(b"".join(b48(v) for v in aI) + i.to_bytes(8, "little")).digest(), "big") % R


def challenge(op, msg, A_, B_, CJ_, D_, U):
    return int.from_bytes(hashlib.sha3_512(msg + b"".join(op.enc(p) for p in (A_, B_, CJ_, D_, U))).digest(), "big") % R


class Key:
    """keygen.cpp: g, tilde_g, x, y, tilde_X = tilde_g^x, Y[k] = g^(y^(k+1)) for k < 2 n except Y[n] = g, tilde_Y[k] = tilde_g^(y^(k+1)) for k < n;
    g, tilde_g, tilde_X and single entries of Y / tilde_Y may be replaced (points outside G1 / G2)"""

    def __init__(self, op, seed, nattr, g=None, tilde_g=None, tilde_X=None, Y=None, tilde_Y=None):
        s = lambda i: prng(seed, i) % R
        self.nattr = nattr
        self.g = op.mul(G1GEN, s(0)) if g is None else g
        self.tilde_g = op.g2mul(G2GEN, s(1)) if tilde_g is None else tilde_g
        self.x, self.y = s(2), s(3)
        self.tilde_X = op.g2mul(self.tilde_g, self.x) if tilde_X is None else tilde_X
        self.Y = [self.g if k == nattr else op.mul(self.g, pow(self.y, k + 1, R)) for k in range(2 * nattr)]
        self.tilde_Y = [op.g2mul(self.tilde_g, pow(self.y, k + 1, R)) for k in range(nattr)]
        for k, v in (Y or {}).items():
            self.Y[k] = v
        for k, v in (tilde_Y or {}).items():
            self.tilde_Y[k] = v
        self.pk = op.enc(self.g) + op.o.g2_compress(self.tilde_g) + op.o.g2_compress(self.tilde_X)
        self.Y49 = b"".join(op.enc(v) for v in self.Y)
        self.tY97 = b"".join(op.o.g2_compress(v) for v in self.tilde_Y)


def issue(op, key, a, seed, w=None):
    """issue.cpp: A = (g * prod_(i < n) Y_i^a_i)^inverse(x + w); serialize(A, w)"""
    w = (prng(seed, 0) % (R - 1) + 1) if w is None else w
    inv = pow((key.x + w) % R, -1, R) if (key.x + w) % R else 0
    return op.enc(op.mul(op.prod(key.g, key.Y[:key.nattr], a), inv)) + b48(w)


def kept(nattr, I):
    """the k of sequence(2 n) the filter of redact.cpp:23-35 keeps, each with its valid_i"""
    J = hidden(nattr, I)
    out = []
    for k in range(2 * nattr):
        valid = [i for i in I if (k - nattr + i) in J]
        if valid:
            out.append((k, valid))
    return out


def redact_points(op, g, Y, a, A, w, I):
    """redact.cpp:7-44 on parsed values -> (C_I, C_J, B, D)"""
    n = len(a)
    J = hidden(n, I)
    C_I = op.prod(g, [Y[i] for i in I], [a[i] for i in I])
    B = op.add(C_I, op.mul(A, -w % R))
    C_J = op.prod(None, [Y[j] for j in J], [a[j] for j in J])
    aI = [a[i] for i in I]
    ks = kept(n, I)
    D = op.prod(None, [Y[k] for k, _ in ks], [sum(q_of(aI, i) * a[k - n + i] for i in valid) % R for k, valid in ks])
    return C_I, C_J, B, D


def redact(op, key, a, sig, I, w_used=None):
    """the cache bytes; w_used: another w in B — a cache whose presentations fail the first pairing equation alone"""
    w = int.from_bytes(sig[49:], "big") if w_used is None else w_used
    return b"".join(op.enc(p) for p in redact_points(op, key.g, key.Y, a, op.dec(sig[:49])[0], w, I))


def pres_points(op, msg, A, w, cache_pts, rnd):
    """pres.cpp:6-27 on parsed values, rnd = [r, alpha, beta] -> PresInfo bytes"""
    C_I, C_J, B, D = cache_pts
    r, alpha, beta = (v % R for v in rnd)
    A_, B_, CJ_, D_ = (op.mul(p, r) for p in (A, B, C_J, D))
    U = op.add(op.mul(C_I, alpha), op.mul(A_, beta))
    c = challenge(op, msg, A_, B_, CJ_, D_, U)
    return b"".join(op.enc(p) for p in (A_, B_, CJ_, D_, U)) + b48((alpha + r * c) % R) + b48((beta + (-w % R) * c) % R)


def pres(op, msg, sig, cache, rnd, w_used=None):
    w = int.from_bytes(sig[49:], "big") if w_used is None else w_used
    return pres_points(op, msg, op.dec(sig[:49])[0], w, [op.dec(cache[49 * k:49 * k + 49])[0] for k in range(4)], rnd)


def draw(seed):
    return [prng(seed, i) % R for i in range(3)]


def expected_verify(op, pk, Y49, tY97, nattr, I, pres341, attr48, msg):
    """verify.cpp:6-24 composed from the oracle on the wire bytes; attr48: the disclosed values in the order of I.  0xff where the reference would
    throw, None when g, tilde_g, tilde_X or a USED record of pk.Y / pk.tilde_Y does not decode (the others are never parsed)."""
    g, ok = op.dec(pk[:49])
    tg, ok1 = op.g2dec(pk[49:146])
    tX, ok2 = op.g2dec(pk[146:243])
    Y = [op.dec(Y49[49 * i:49 * i + 49]) for i in I]
    tY = [op.g2dec(tY97[97 * (nattr - 1 - i):97 * (nattr - i)]) for i in I]
    if not (ok and ok1 and ok2 and all(v[1] for v in Y + tY)):
        return None
    pts = []
    for k in range(5):
        pt, ok = op.dec(pres341[49 * k:49 * k + 49])
        if not ok:
            return 0xff
        pts.append(pt)
    A_, B_, CJ_, D_, U = pts
    s, t = _fields(pres341[245:], 2)
    a = _fields(attr48, len(I))
    if any(v >= R for v in [s, t] + a):
        return 0xff
    c = challenge(op, msg, A_, B_, CJ_, D_, U)
    eq1 = op.o.pair(A_, tX) == op.o.pair(op.add(CJ_, B_), tg)
    K = op.prod(g, [v[0] for v in Y], a)
    eq2 = op.add(U, op.mul(B_, c)) == op.add(op.mul(K, s), op.mul(A_, t))
    W = bytes(192)
    for (ty, _), i in zip(tY, I):
        W = op.o.g2_add(W, op.g2mul(ty, q_of(a, i)), 192)
    eq3 = op.o.pair(CJ_, W) == op.o.pair(D_, tg)
    return 1 if (eq1 and eq2 and eq3) else 0


def equations(op, key, I, pres341, attr48, msg):
    """which of the three equations hold, for the self-check of the lanes"""
    A_, B_, CJ_, D_, U = (op.dec(pres341[49 * k:49 * k + 49])[0] for k in range(5))
    s, t = _fields(pres341[245:], 2)
    a = _fields(attr48, len(I))
    c = challenge(op, msg, A_, B_, CJ_, D_, U)
    K = op.prod(key.g, [key.Y[i] for i in I], a)
    W = bytes(192)
    for i in I:
        W = op.o.g2_add(W, op.g2mul(key.tilde_Y[key.nattr - 1 - i], q_of(a, i)), 192)
    return (op.o.pair(A_, key.tilde_X) == op.o.pair(op.add(CJ_, B_), key.tilde_g),
            op.add(U, op.mul(B_, c)) == op.add(op.mul(K, s), op.mul(A_, t)),
            op.o.pair(CJ_, W) == op.o.pair(D_, key.tilde_g))


def expected_pres(op, sig97, cache196, msg, rnd96):
    """pres from the wire bytes: (PresInfo, status); rnd96: 3 x 32 bytes, any values.  0xff where the reference would throw."""
    pts = [op.dec(sig97[:49])] + [op.dec(cache196[49 * k:49 * k + 49]) for k in range(4)]
    w = int.from_bytes(sig97[49:], "big")
    if w >= R or not all(ok for _, ok in pts):
        return b"\xff" * 341, 0xff
    rnd = [int.from_bytes(rnd96[32 * i:32 * i + 32], "big") for i in range(3)]
    return pres_points(op, msg, pts[0][0], w, [p for p, _ in pts[1:]], rnd), 0


def expected_redact(op, pk, Y49, nattr, I, attr48, sig97):
    """redact from the wire bytes: (RedactCache, status), or None when g, tilde_g, tilde_X or ANY of the 2 n records of pk.Y does not decode"""
    g, ok = op.dec(pk[:49])
    ok1, ok2 = op.g2dec(pk[49:146])[1], op.g2dec(pk[146:243])[1]
    Y = [op.dec(Y49[49 * k:49 * k + 49]) for k in range(2 * nattr)]
    if not (ok and ok1 and ok2 and all(v[1] for v in Y)):
        return None
    a, (w,) = _fields(attr48, nattr), _fields(sig97[49:], 1)
    A, ok = op.dec(sig97[:49])
    if not ok or w >= R or any(v >= R for v in a):
        return b"\xff" * 196, 0xff
    return b"".join(op.enc(p) for p in redact_points(op, g, [v[0] for v in Y], a, A, w, I)), 0


# ---------------------------------------------------------------- lanes
class Lane:
    def __init__(self, kind, msg, pres341, attr48):
        self.kind, self.msg, self.pres, self.attr = kind, msg, pres341, attr48


class Cred:
    """one credential under key: attributes, signature, cache for the set I, message, randomness"""

    def __init__(self, op, key, I, seed, i, msg_len=MSG_LEN):
        self.a = attributes(seed + 1000 + i, key.nattr)
        self.sig = issue(op, key, self.a, seed + 2000 + i)
        self.cache = redact(op, key, self.a, self.sig, I)
        self.msg = message(seed, i, msg_len)
        self.rnd = draw(seed + 3000 + i)
        self.attr = b"".join(b48(self.a[k]) for k in I)
        self.attr_all = b"".join(b48(v) for v in self.a)


def valid_lanes(op, key, I, count, seed, msg_len=MSG_LEN):
    """`count` honest presentations under key with the disclosure set I"""
    out = []
    for i in range(count):
        cr = Cred(op, key, I, seed, i, msg_len)
        out.append(Lane("valid", cr.msg, pres(op, cr.msg, cr.sig, cr.cache, cr.rnd), cr.attr))
    return out


def _with(lane, kind, **kw):
    d = dict(msg=lane.msg, pres341=lane.pres, attr48=lane.attr)
    d.update(kw)
    return Lane(kind, d["msg"], d["pres341"], d["attr48"])


def _pt(p, k, rec):
    return p[:49 * k] + rec + p[49 * k + 49:]


def main_lanes(op, key):
    """valid, tampered, degenerate, off-subgroup and malformed lanes of the main shape, with their kinds"""
    I = I_MAIN
    lanes = valid_lanes(op, key, I, 6, 5100)
    b, b1 = lanes[0], lanes[1]
    cr = Cred(op, key, I, 5100, 0)
    mk = lambda kind, p: Lane(kind, b.msg, p, b.attr)
    # every field of PresInfo tampered, the message, a disclosed value
    names = ("A_", "B_", "C_J_", "D_", "U")
    for k in range(5):
        lanes.append(_with(b, names[k] + " swapped", pres341=_pt(b.pres, k, b1.pres[49 * k:49 * k + 49])))
    lanes.append(_with(b, "s+1", pres341=_plus1(b.pres, 0, 245)))                      # the Schnorr equation alone fails: s is not hashed
    lanes.append(_with(b, "t+1", pres341=_plus1(b.pres, 1, 245)))
    lanes.append(_with(b, "flipped msg", msg=bytes([b.msg[0] ^ 1]) + b.msg[1:]))
    lanes.append(_with(b, "a+1", attr48=_plus1(b.attr, 1)))
    # the pairing equations failing alone: a cache made with another w, a cache with another D, presented honestly
    w1 = (int.from_bytes(cr.sig[49:], "big") + 1) % R
    lanes.append(mk("eq1 only fails", pres(op, b.msg, cr.sig, redact(op, key, cr.a, cr.sig, I, w_used=w1), cr.rnd, w_used=w1)))
    D1 = op.enc(op.add(op.dec(cr.cache[147:])[0], G1GEN))
    lanes.append(mk("eq3 only fails", pres(op, b.msg, cr.sig, cr.cache[:147] + D1, cr.rnd)))
    # degenerate
    inf_sig = bytes(49) + cr.sig[49:]
    lanes.append(mk("A at infinity", pres(op, b.msg, inf_sig, redact(op, key, cr.a, inf_sig, I), cr.rnd)))
    r0 = pres(op, b.msg, cr.sig, cr.cache, [0] + cr.rnd[1:])
    lanes.append(mk("r = 0", r0))
    assert r0[0] == r0[49] == r0[98] == r0[147] == 0
    lanes.append(mk("leading 00 + bytes", b"\x00" + bytes(range(1, 49)) + r0[49:147] + b"\x00" + bytes(range(7, 55)) + r0[196:]))
    x_big = int.from_bytes(b.pres[1:49], "big") + FP                      # x >= p, same point
    lanes.append(_with(b, "x >= p", pres341=b.pres[:1] + x_big.to_bytes(48, "big") + b.pres[49:]))
    lanes.append(_with(b, "s = t = 0", pres341=_field(_field(b.pres, 0, 0, 245), 1, 0, 245)))
    # off the subgroup
    t3 = enc96(point_of_order(3))
    te = enc96(eigenpoint(10177)[0])
    dec = lambda k: op.dec(b.pres[49 * k:49 * k + 49])[0]
    for k in (0, 2, 3):
        lanes.append(_with(b, names[k] + " + order 3", pres341=_pt(b.pres, k, op.enc(op.add(dec(k), t3)))))
        lanes.append(_with(b, names[k] + " + eigenpoint", pres341=_pt(b.pres, k, op.enc(op.add(dec(k), te)))))
    # malformed
    lanes.append(_with(b, "U off curve", pres341=_pt(b.pres, 4, off_curve_x())))
    lanes.append(_with(b, "D_ off curve", pres341=_pt(b.pres, 3, off_curve_x())))
    lanes.append(_with(b, "B_ bad tag", pres341=b.pres[:49] + b"\x05" + b.pres[50:]))
    lanes.append(_with(b, "s = r", pres341=_field(b.pres, 0, R, 245)))
    lanes.append(_with(b, "t = 2^384 - 1", pres341=_field(b.pres, 1, (1 << 384) - 1, 245)))
    lanes.append(_with(b, "a = r", attr48=_field(b.attr, 0, R)))
    return lanes


ZERO_KINDS = ("A_ swapped", "B_ swapped", "C_J_ swapped", "D_ swapped", "U swapped", "s+1", "t+1", "flipped msg", "a+1", "eq1 only fails", "eq3 only fails",
              "s = t = 0", "A_ + order 3", "A_ + eigenpoint", "C_J_ + order 3", "C_J_ + eigenpoint", "D_ + order 3", "D_ + eigenpoint")
BAD_KINDS = ("U off curve", "D_ off curve", "B_ bad tag", "s = r", "t = 2^384 - 1", "a = r")
ONE_KINDS = ("valid", "r = 0", "leading 00 + bytes", "x >= p")


def expect(op, key, I, lanes):
    """the expected byte of every lane"""
    return bytes(expected_verify(op, key.pk, key.Y49, key.tY97, key.nattr, I, ln.pres, ln.attr, ln.msg) for ln in lanes)


def pack(lanes):
    """(pres_341, attr_48, msgs) of a list of lanes as the entry takes them"""
    return b"".join(ln.pres for ln in lanes), b"".join(ln.attr for ln in lanes), b"".join(ln.msg for ln in lanes)
