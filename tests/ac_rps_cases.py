"""Builders for the AC-rps tests (the reference's examples/AC-rps): keygen, user_keygen, issue, redact and pres as the reference writes them — scalars
from util.prng, points by the CPU oracle through ac_bbs_cases.Ops (multiply = PAIR_G1mul / PAIR_G2mul, add, compression, Miller loop, final
exponentiation), G2 negation as y -> p - y, the q_k and c0 by hashlib's SHA3-512 mod r — and the expected results of the library's entries
composed independently from the same primitives:
    expected_verify   verify.cpp:6-38 from the wire bytes: the c0 check in front of the attributes, two equations, only the used key records decoded
    expected_pres     pres.cpp:8-62 from the wire bytes and the caller's randomness
    expected_redact   redact.cpp:6-16 from the wire bytes
tests/test_ac_rps_cases.py checks the builders against themselves on the CPU; the GPU tests compare the library with them."""
import hashlib

from ac_bbs_cases import G1GEN, G2GEN, Ops, _field, _fields, _plus1, attributes, b32, b48, g2_outside, hidden, off_curve_x  # noqa: F401
from g1_torsion import P as FP, eigenpoint, enc as enc96, point_of_order
from util import R, prng

# (nattr, I) of the GPU tests; pres takes the shapes whose base list fits 32 positions
SHAPES = [(1, ()), (1, (0,)), (2, (1,)), (4, (3, 0)), (4, ()), (4, (0, 1, 2, 3)), (10, (0, 3)), (9, tuple(range(8)))]
BIG_SHAPES = [(32, (0, 3)), (32, tuple(range(31)))]                         # verify and redact only
REFUSED_PRES_SHAPES = [(13, tuple(range(1, 12))), (17, (0, 3))]             # 12 + 23 and 3 + 31 positions; (16, (0, 3)) fills the list exactly
NATTR, I_MAIN = 4, (0, 3)


def g2neg(q):
    """ECP2_neg on a 192-byte record x.b | x.a | y.b | y.a: both halves of y negated mod p, zero (and infinity) staying zero"""
    neg = lambda b: ((FP - int.from_bytes(b, "big")) % FP).to_bytes(48, "big")
    return q[:96] + neg(q[96:144]) + neg(q[144:])


def g2add(op, a, b):
    return op.o.g2_add(a, b, 192)


def g2enc(op, q):
    return op.o.g2_compress(q)


def q_of(op, s1, s2, ts, I, aI, ip):
    """hash(sigma1_, sigma2_, tilde_sigma_, indexes, a[j] (j.in(I)), i).to(Zp): the points as serialize writes them, every index and i as a size_t"""
    msg = op.enc(s1) + op.enc(s2) + g2enc(op, ts) + b"".join(i.to_bytes(8, "little") for i in I) + b"".join(b48(v) for v in aI)
    return int.from_bytes(hashlib.sha3_512(msg + ip.to_bytes(8, "little")).digest(), "big") % R


def q_tail_bytes(nI):
    """what the last block(s) of the q hash hold: the rest of the shared prefix and the 8 bytes of the index"""
    return (195 + 56 * nI) % 72 + 8


def c0_of(op, s1, C, C0):
    return int.from_bytes(hashlib.sha3_512(op.enc(s1) + op.enc(C) + op.enc(C0)).digest(), "big") % R


class Key:
    """keygen.cpp: g, tilde_g, x, y, tilde_X = tilde_g^x, Y[k] = g^(y^(k+1)) for k <= 2 n, tilde_Y[k] = tilde_g^(y^(k+1)) for k <= n; g, tilde_g,
    tilde_X and single entries of Y / tilde_Y may be replaced (points outside G1 / G2)"""

    def __init__(self, op, seed, nattr, g=None, tilde_g=None, tilde_X=None, Y=None, tilde_Y=None):
        s = lambda i: prng(seed, i) % R
        self.nattr = nattr
        self.g = op.mul(G1GEN, s(0)) if g is None else g
        self.tilde_g = op.g2mul(G2GEN, s(1)) if tilde_g is None else tilde_g
        self.x, self.y = s(2), s(3)
        self.tilde_X = op.g2mul(self.tilde_g, self.x) if tilde_X is None else tilde_X
        self.Y = [op.mul(self.g, pow(self.y, k + 1, R)) for k in range(2 * nattr + 1)]
        self.tilde_Y = [op.g2mul(self.tilde_g, pow(self.y, k + 1, R)) for k in range(nattr + 1)]
        for k, v in (Y or {}).items():
            self.Y[k] = v
        for k, v in (tilde_Y or {}).items():
            self.tilde_Y[k] = v
        self.pk = op.enc(self.g) + g2enc(op, self.tilde_g) + g2enc(op, self.tilde_X)
        self.Y49 = b"".join(op.enc(v) for v in self.Y)
        self.tY97 = b"".join(g2enc(op, v) for v in self.tilde_Y)


def user_keygen(op, key, seed, z=None):
    """user_keygen.cpp: usk = z, upk = g^z"""
    z = (prng(seed, 0) % (R - 1) + 1) if z is None else z
    return z, op.mul(key.g, z)


def issue(op, key, upk, a, seed):
    """issue.cpp: h = g^alpha, sigma = h^(x + sum a_i y^(i+1)) * upk^(alpha y^(n+1)), tilde_M = prod tilde_Y[i]^a_i; serialize(h, sigma, tilde_M)"""
    n = len(a)
    alpha = prng(seed, 0) % (R - 1) + 1
    h = op.mul(key.g, alpha)
    ym = sum(a[i] * pow(key.y, i + 1, R) for i in range(n)) % R
    sigma = op.add(op.mul(h, (key.x + ym) % R), op.mul(upk, alpha * pow(key.y, n + 1, R) % R))
    tM = bytes(192)
    for i in range(n):
        tM = g2add(op, tM, op.g2mul(key.tilde_Y[i], a[i]))
    return op.enc(h) + op.enc(sigma) + g2enc(op, tM)


def redact_point(op, tilde_Y, a, tM, I):
    """redact.cpp:6-16 on parsed values: tilde_M / prod_I tilde_Y[i]^a_i, the quotient as add-the-negative"""
    acc = bytes(192)
    for i in I:
        acc = g2add(op, acc, op.g2mul(tilde_Y[i], a[i]))
    return g2add(op, tM, g2neg(acc))


def redact(op, key, a, sig, I):
    return g2enc(op, redact_point(op, key.tilde_Y, a, op.g2dec(sig[98:])[0], I))


def cross_terms(nattr, I, a, q):
    """pres.cpp:38-55: the kept k ascending, each with its exponent (size_t arithmetic: a negative index is in no set)"""
    Ip, J = list(I) + [nattr], hidden(nattr, I)
    out = []
    for k in range(2 * nattr + 1):
        valid = [ii for ii in range(len(Ip)) if (k + Ip[ii] - nattr - 1) in J]
        if valid:
            out.append((k, sum(q[ii] * a[k + Ip[ii] - nattr - 1] for ii in valid) % R))
    return out


def pres_points(op, tg, Y, a, h, sigma, tH, z, I, rnd):
    """pres.cpp:8-62 on parsed values, rnd = [r, t, rho] -> PresInfo bytes"""
    n = len(a)
    r, t, rho = (v % R for v in rnd)
    Ip = list(I) + [n]
    s1 = op.mul(h, r)
    s2 = op.add(op.mul(sigma, r), op.mul(s1, t))
    ts = g2add(op, op.g2mul(tg, t), tH)
    q = [q_of(op, s1, s2, ts, I, [a[i] for i in I], ip) for ip in Ip]
    s3 = op.prod(None, [Y[n - ip] for ip in Ip], [t * qk % R for qk in q])
    cross = cross_terms(n, I, a, q)
    s3 = op.add(s3, op.prod(None, [Y[k] for k, _ in cross], [e for _, e in cross]))
    C, C0 = op.mul(s1, z), op.mul(s1, rho)
    c0 = c0_of(op, s1, C, C0)
    s0 = (rho + (-c0 % R) * z) % R
    return op.enc(s1) + op.enc(s2) + op.enc(s3) + op.enc(C) + g2enc(op, ts) + b48(c0) + b48(s0)


def pres(op, key, a, sig, cache, z, I, rnd):
    return pres_points(op, key.tilde_g, key.Y, a, op.dec(sig[:49])[0], op.dec(sig[49:98])[0], op.g2dec(cache)[0], z, I, rnd)


def draw(seed):
    return [prng(seed, i) % R for i in range(3)]


def gt_one(op):
    return op.o.pair(bytes(96), G2GEN)


def miller_eq(op, left, right):
    """liner_pair.hpp:336-350: the product of the Miller values on the left, the conjugate of the right one, one final exponentiation, is_unity"""
    acc = op.o.miller(*left[0])
    for g1, g2 in left[1:]:
        acc = op.o.gt_op("mul", acc, op.o.miller(g1, g2))
    acc = op.o.gt_op("mul", acc, op.o.gt_op("conj", op.o.miller(*right)))
    return op.o.fexp(acc) == gt_one(op)


def _parse_pres(op, p):
    pts = [op.dec(p[49 * k:49 * k + 49]) for k in range(4)] + [op.g2dec(p[196:293])]
    return pts, _fields(p[293:], 2)


def verify_steps(op, g2key, Yused, tYused, tYn, I, nattr, pres389, attr48, past_c0=False):
    """verify.cpp:14-38 on parsed key points -> (c0 matches, a in range, eq1, eq2); the equations are None behind a failed c0 or range check
    (past_c0: the equations are evaluated behind a failed c0 check too, for the self-check of the lanes)"""
    tg, tX = g2key
    pts, (c0, s0) = _parse_pres(op, pres389)
    s1, s2, s3, C, ts = (v[0] for v in pts)
    C0 = op.add(op.mul(s1, s0), op.mul(C, c0))
    c0ok = c0 == c0_of(op, s1, C, C0)
    if not c0ok and not past_c0:
        return False, None, None, None
    a = _fields(attr48, len(I))
    if any(v >= R for v in a):
        return c0ok, False, None, None
    q = [q_of(op, s1, s2, ts, I, a, ip) for ip in list(I) + [nattr]]
    S = op.prod(None, Yused, q)
    W = g2add(op, tX, ts)
    for ty, v in zip(tYused, a):
        W = g2add(op, W, op.g2mul(ty, v))
    return c0ok, True, miller_eq(op, [(s1, W), (C, tYn)], (s2, tg)), miller_eq(op, [(s3, tg)], (S, ts))


def expected_verify(op, pk, Y49, tY97, nattr, I, pres389, attr48):
    """verify.cpp:6-38 composed from the oracle on the wire bytes; attr48: the disclosed values in the order of I.  0xff where the reference would
    throw, None when g, tilde_g, tilde_X or a USED record of pk.Y / pk.tilde_Y does not decode (the others are never parsed)."""
    pub = [op.dec(pk[:49]), op.g2dec(pk[49:146]), op.g2dec(pk[146:243])]
    Y = [op.dec(Y49[49 * (nattr - i):49 * (nattr - i) + 49]) for i in list(I) + [nattr]]
    tY = [op.g2dec(tY97[97 * i:97 * i + 97]) for i in list(I) + [nattr]]
    if not all(v[1] for v in pub + Y + tY):
        return None
    pts, sc = _parse_pres(op, pres389)
    if not all(ok for _, ok in pts) or any(v >= R for v in sc):
        return 0xff
    c0ok, aok, eq1, eq2 = verify_steps(op, (pub[1][0], pub[2][0]), [v[0] for v in Y], [v[0] for v in tY[:-1]], tY[-1][0], I, nattr, pres389, attr48)
    if not c0ok:
        return 0
    if not aok:
        return 0xff
    return 1 if (eq1 and eq2) else 0


def checks(op, key, I, pres389, attr48, past_c0=False):
    """(c0 matches, eq1, eq2) for the self-check of the lanes"""
    n = key.nattr
    c0ok, _, eq1, eq2 = verify_steps(op, (key.tilde_g, key.tilde_X), [key.Y[n - i] for i in list(I) + [n]], [key.tilde_Y[i] for i in I], key.tilde_Y[n], I, n,
                                     pres389, attr48, past_c0)
    return c0ok, eq1, eq2


def expected_pres(op, pk, Y49, nattr, I, attr48, sig195, cache97, usk48, rnd96):
    """pres from the wire bytes: (PresInfo, status), or None when g, tilde_g, tilde_X or ANY of the 2 n + 1 records of pk.Y does not decode;
    rnd96: 3 x 32 bytes, any values.  0xff where the reference would throw."""
    pub = [op.dec(pk[:49]), op.g2dec(pk[49:146]), op.g2dec(pk[146:243])]
    Y = [op.dec(Y49[49 * k:49 * k + 49]) for k in range(2 * nattr + 1)]
    if not all(v[1] for v in pub + Y):
        return None
    a, (z,) = _fields(attr48, nattr), _fields(usk48, 1)
    pts = [op.dec(sig195[:49]), op.dec(sig195[49:98]), op.g2dec(sig195[98:]), op.g2dec(cache97)]
    if z >= R or any(v >= R for v in a) or not all(ok for _, ok in pts):
        return b"\xff" * 389, 0xff
    rnd = [int.from_bytes(rnd96[32 * i:32 * i + 32], "big") for i in range(3)]
    return pres_points(op, pub[1][0], [v[0] for v in Y], a, pts[0][0], pts[1][0], pts[3][0], z, I, rnd), 0


def expected_redact(op, tY97, nattr, I, attr48, sig195):
    """redact from the wire bytes: (RedactCache, status), or None when a USED record of pk.tilde_Y does not decode"""
    tY = {i: op.g2dec(tY97[97 * i:97 * i + 97]) for i in I}
    if not all(v[1] for v in tY.values()):
        return None
    a = _fields(attr48, nattr)
    pts = [op.dec(sig195[:49]), op.dec(sig195[49:98]), op.g2dec(sig195[98:])]
    if any(a[i] >= R for i in I) or not all(ok for _, ok in pts):
        return b"\xff" * 97, 0xff
    return g2enc(op, redact_point(op, {i: v[0] for i, v in tY.items()}, a, pts[2][0], I)), 0


# ---------------------------------------------------------------- lanes
class Lane:
    def __init__(self, kind, pres389, attr48):
        self.kind, self.pres, self.attr = kind, pres389, attr48


class Cred:
    """one credential under key: user key, attributes, signature, cache for the set I, randomness"""

    def __init__(self, op, key, I, seed, i, z=None):
        self.a = attributes(seed + 1000 + i, key.nattr)
        self.z, self.upk = user_keygen(op, key, seed + 4000 + i, z)
        self.sig = issue(op, key, self.upk, self.a, seed + 2000 + i)
        self.cache = redact(op, key, self.a, self.sig, I)
        self.rnd = draw(seed + 3000 + i)
        self.attr = b"".join(b48(self.a[k]) for k in I)
        self.attr_all = b"".join(b48(v) for v in self.a)
        self.usk = b48(self.z)
        self.rnd96 = b"".join(b32(v) for v in self.rnd)


def valid_lanes(op, key, I, count, seed):
    """`count` honest presentations under key with the disclosure set I"""
    out = []
    for i in range(count):
        cr = Cred(op, key, I, seed, i)
        out.append(Lane("valid", pres(op, key, cr.a, cr.sig, cr.cache, cr.z, I, cr.rnd), cr.attr))
    return out


def _with(lane, kind, **kw):
    d = dict(pres389=lane.pres, attr48=lane.attr)
    d.update(kw)
    return Lane(kind, d["pres389"], d["attr48"])


OFF = {"sigma1_": 0, "sigma2_": 49, "sigma3_": 98, "C": 147, "tilde_sigma_": 196}


def _pt(p, name, rec):
    return p[:OFF[name]] + rec + p[OFF[name] + len(rec):]


def _get(p, name):
    return p[OFF[name]:OFF[name] + (97 if name == "tilde_sigma_" else 49)]


def main_lanes(op, key):
    """valid, tampered, degenerate, off-subgroup and malformed lanes of the main shape, with their kinds"""
    I = I_MAIN
    lanes = valid_lanes(op, key, I, 3, 5100)
    b, b1 = lanes[0], lanes[1]
    cr = Cred(op, key, I, 5100, 0)
    mk = lambda kind, p: Lane(kind, p, b.attr)
    again = lambda **kw: pres(op, key, cr.a, kw.get("sig", cr.sig), kw.get("cache", cr.cache), kw.get("z", cr.z), I, kw.get("rnd", cr.rnd))
    # every field of PresInfo tampered, a disclosed value
    for name in OFF:
        lanes.append(_with(b, name + " swapped", pres389=_pt(b.pres, name, _get(b1.pres, name))))
    lanes.append(_with(b, "c0+1", pres389=_plus1(b.pres, 0, 293)))
    lanes.append(_with(b, "s0+1", pres389=_plus1(b.pres, 1, 293)))                    # the c0 check alone fails: s0 is in neither equation
    lanes.append(_with(b, "a+1", attr48=_plus1(b.attr, 1)))
    # each equation failing alone: a signature with another sigma presented honestly; sigma3_ (not hashed) moved
    sig1 = cr.sig[:49] + op.enc(op.add(op.dec(cr.sig[49:98])[0], G1GEN)) + cr.sig[98:]
    lanes.append(mk("eq1 only fails", again(sig=sig1)))
    lanes.append(_with(b, "eq2 only fails", pres389=_pt(b.pres, "sigma3_", op.enc(op.add(op.dec(_get(b.pres, "sigma3_"))[0], G1GEN)))))
    # the c0 check comes before the attributes are read
    lanes.append(_with(b, "c0 wrong and a = r", pres389=_plus1(b.pres, 1, 293), attr48=_field(b.attr, 0, R)))
    # degenerate
    r0 = again(rnd=[0] + cr.rnd[1:])
    lanes.append(mk("r = 0", r0))
    assert r0[0] == r0[49] == r0[147] == 0
    lanes.append(mk("leading 00 + bytes", b"\x00" + bytes(range(1, 49)) + r0[49:147] + b"\x00" + bytes(range(7, 55)) + r0[196:]))
    lanes.append(mk("t = 0", again(rnd=[cr.rnd[0], 0, cr.rnd[2]])))
    z0 = Cred(op, key, I, 5100, 0, z=0)
    lanes.append(mk("z = 0", pres(op, key, z0.a, z0.sig, z0.cache, 0, I, z0.rnd)))
    x_big = int.from_bytes(b.pres[1:49], "big") + FP                      # x >= p, same point
    lanes.append(_with(b, "x >= p", pres389=b.pres[:1] + x_big.to_bytes(48, "big") + b.pres[49:]))
    # off the subgroups
    t3 = enc96(point_of_order(3))
    te = enc96(eigenpoint(10177)[0])
    for name in ("sigma1_", "sigma3_", "C"):
        pt = op.dec(_get(b.pres, name))[0]
        lanes.append(_with(b, name + " + order 3", pres389=_pt(b.pres, name, op.enc(op.add(pt, t3)))))
        lanes.append(_with(b, name + " + eigenpoint", pres389=_pt(b.pres, name, op.enc(op.add(pt, te)))))
    lanes.append(_with(b, "tilde_sigma_ outside G2", pres389=_pt(b.pres, "tilde_sigma_", g2enc(op, g2_outside()))))
    lanes.append(mk("tilde_H outside G2", again(cache=g2enc(op, g2add(op, op.g2dec(cr.cache)[0], g2_outside())))))
    # malformed
    lanes.append(_with(b, "sigma3_ off curve", pres389=_pt(b.pres, "sigma3_", off_curve_x())))
    lanes.append(_with(b, "C bad tag", pres389=_pt(b.pres, "C", b"\x05" + _get(b.pres, "C")[1:])))
    lanes.append(_with(b, "tilde_sigma_ tag 04", pres389=_pt(b.pres, "tilde_sigma_", b"\x04" + _get(b.pres, "tilde_sigma_")[1:])))
    lanes.append(_with(b, "c0 = r", pres389=_field(b.pres, 0, R, 293)))
    lanes.append(_with(b, "s0 = 2^384 - 1", pres389=_field(b.pres, 1, (1 << 384) - 1, 293)))
    lanes.append(_with(b, "a = r", attr48=_field(b.attr, 0, R)))
    return lanes


ZERO_KINDS = ("sigma1_ swapped", "sigma2_ swapped", "sigma3_ swapped", "C swapped", "tilde_sigma_ swapped", "c0+1", "s0+1", "a+1", "eq1 only fails",
              "eq2 only fails", "c0 wrong and a = r", "sigma1_ + order 3", "sigma1_ + eigenpoint", "C + order 3", "C + eigenpoint", "tilde_sigma_ outside G2")
BAD_KINDS = ("sigma3_ off curve", "C bad tag", "tilde_sigma_ tag 04", "c0 = r", "s0 = 2^384 - 1", "a = r")
# sigma3_ is hashed nowhere and a cofactor-order component of it pairs to 1: the reference accepts these, and so must the library
ONE_KINDS = ("valid", "r = 0", "leading 00 + bytes", "t = 0", "z = 0", "x >= p", "sigma3_ + order 3", "sigma3_ + eigenpoint")


def expect(op, key, I, lanes):
    """the expected byte of every lane"""
    return bytes(expected_verify(op, key.pk, key.Y49, key.tY97, key.nattr, I, ln.pres, ln.attr) for ln in lanes)


def pack(lanes):
    """(pres_389, attr_48) of a list of lanes as the entry takes them"""
    return b"".join(ln.pres for ln in lanes), b"".join(ln.attr for ln in lanes)
