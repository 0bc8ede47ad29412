"""Builders for the MHAC-bbs tests (the reference's examples/MHAC-bbs): iss_setup, generate_attributes, cred_iss, make_pres_group, make_pres_type
and cred_pres as the reference writes them — scalars from util.prng, points by the CPU oracle (g1_mul = PAIR_G1mul, g1_add, compression, pair),
ch by hashlib's SHA3-512 mod r — and the expected results of the library's entries composed independently from the same primitives:
    expected_verify   verify_pres.cpp:6-46 from the wire bytes, the revealed values only
    expected_pres     cred_pres.cpp:6-113 from the wire bytes and the caller's randomness, term by term in one flat loop
tests/test_mhac_bbs_cases.py checks the builders against themselves on the CPU; the GPU tests compare the library with them."""
import hashlib

from ac_bbs_cases import G1GEN, G2GEN, Ops, b48, off_curve_x, g2_outside  # noqa: F401  (re-exported for the tests)
from util import R, prng

T_MAX = 8


def sets(m, Prv, Rev):
    """Pub, Hid, HidPub, RevPub (positions of Pub), I_Pub_in_Hid as the reference derives them"""
    Pub = [i for i in range(m) if i not in Prv]
    Hid = [i for i in range(m) if i not in Rev]
    HidPub = [i for i in Hid if i not in Prv]
    RevPub = [k for k in range(len(Pub)) if Pub[k] in Rev]
    PubHid = [k for k in range(len(Pub)) if Pub[k] in Hid]
    return Pub, Hid, HidPub, RevPub, PubHid


def inv(a):
    return pow(a % R, -1, R) if a % R else 0


def polynomial(x, c0, coeffs):
    return (c0 + sum(c * pow(x, k + 1, R) for k, c in enumerate(coeffs))) % R


def lagrange(xs, k):
    """prod_(y != k) (-x[y] / (x[k] - x[y]))"""
    lam = 1
    for y in range(len(xs)):
        if y != k:
            lam = lam * ((-xs[y]) % R) % R * inv(xs[k] - xs[y]) % R
    return lam


def challenge(op, U, A_, B_, revealed):
    """hash(U, A_, B_, pub_a[ii] (ii in I_Pub_in_Rev)).to(Zp): the points as serialize writes them, the values as 48-byte fields"""
    return int.from_bytes(hashlib.sha3_512(op.enc(U) + op.enc(A_) + op.enc(B_) + b"".join(b48(v) for v in revealed)).digest(), "big") % R


class World:
    """iss_setup: pp = (g1, g2, h_0 .. h_(m-1)), sk = gamma, pk = w = g2^gamma; h entries and w may be replaced (points outside G1 / G2)"""

    def __init__(self, op, seed, m, h=None, w=None):
        s = lambda i: prng(seed, i) % R
        self.m = m
        self.g1 = op.mul(G1GEN, s(0))
        self.g2 = op.g2mul(G2GEN, s(1))
        self.gamma = s(2)
        self.w = op.g2mul(self.g2, self.gamma) if w is None else w
        self.h = [op.mul(G1GEN, s(10 + i)) for i in range(m)]
        for i, p in (h or {}).items():
            self.h[i] = p
        self.pp = op.enc(self.g1) + op.o.g2_compress(self.g2)
        self.h49 = b"".join(op.enc(p) for p in self.h)
        self.pk = op.o.g2_compress(self.w)


def generate_attributes(op, wd, t, nparties, Prv, seed):
    """(public attributes in Pub order, shares[party][ii], commitments C[party])"""
    Pub = sets(wd.m, Prv, ())[0]
    attr = [prng(seed, i) % R for i in range(wd.m)]
    a = [prng(seed + 1, i) % R for i in range(len(Prv) * (t - 1))]
    share = [[polynomial(x, attr[Prv[ii]], a[ii * (t - 1):(ii + 1) * (t - 1)]) for ii in range(len(Prv))] for x in range(1, nparties + 1)]
    C = [op.prod(None, [wd.h[i] for i in Prv], share[k]) for k in range(nparties)]
    return [attr[i] for i in Pub], share, C


def cred_iss(op, wd, t, C, Pub, pub_a, seed, gamma=None):
    """(A, e_share[party], D[party]); gamma: another issuer key — a credential whose presentations keep the hash half and fail the pairing half"""
    xs = list(range(1, t + 1))
    C_a = op.prod(op.prod(wd.g1, C[:t], [lagrange(xs, i) for i in range(t)]), [wd.h[i] for i in Pub], pub_a)
    e = prng(seed, 0) % R
    A = op.mul(C_a, inv((wd.gamma if gamma is None else gamma) + e))
    a = [prng(seed, 1 + i) % R for i in range(t - 1)]
    e_share = [polynomial(x, e, a) for x in range(1, len(C) + 1)]
    D = [op.add(C[i], op.mul(A, -e_share[i])) for i in range(len(C))]
    return A, e_share, D


def make_pres_group(op, D_share, S):
    xs = [i + 1 for i in S]
    lam = [lagrange(xs, k) for k in range(len(S))]
    return lam, op.prod(None, [D_share[i] for i in S], lam)


def make_pres_type(op, wd, Rev, Prv, pub_a):
    Pub, _, _, RevPub, PubHid = sets(wd.m, Prv, Rev)
    C_rev = op.prod(wd.g1, [wd.h[Pub[k]] for k in RevPub], [pub_a[k] for k in RevPub])
    C_pub = op.prod(C_rev, [wd.h[Pub[k]] for k in PubHid], [pub_a[k] for k in PubHid])
    return C_rev, C_pub


def rnd_count(m, Prv, Rev, t):
    return 2 + (t - 1) * len(Prv) + (m - len(Rev)) + t


def draw(seed, count):
    return [prng(seed, i) % R for i in range(count)]


def cred_pres(op, wd, A, e_S, lam, D, C_rev, C_pub, Prv, Rev, pub_a, a_S, rnd):
    """cred_pres.cpp:6-113 on parsed values with j = 0: e_S[k], a_S[k][ii] are the rows of the parties in S; rnd = [r, alpha, beta_share ..,
    beta_share_j .., gamma_share ..].  Returns (fixed_242, z, zhp) as bytes."""
    Pub, Hid, HidPub, RevPub, _ = sets(wd.m, Prv, Rev)
    t, nP = len(lam), len(Prv)
    rnd = [v % R for v in rnd]
    r, alpha = rnd[0], rnd[1]
    beta = rnd[2:2 + (t - 1) * nP]
    beta_j = rnd[2 + (t - 1) * nP:2 + (t - 1) * nP + len(Hid)]
    gamma = rnd[2 + (t - 1) * nP + len(Hid):]
    assert len(gamma) == t
    beta_k = lambda k: beta[(k - 1) * nP:k * nP]
    A_ = op.mul(A, r)
    B_ = op.mul(op.add(C_pub, D), r)
    U = op.add(op.prod(op.mul(C_rev, alpha), [wd.h[i] for i in Hid], beta_j), op.mul(A_, gamma[0]))
    for k in range(1, t):
        U = op.add(U, op.add(op.prod(None, [wd.h[i] for i in Prv], beta_k(k)), op.mul(A_, gamma[k])))
    ch = challenge(op, U, A_, B_, [pub_a[k] for k in RevPub])
    zr = (alpha + ch * r) % R
    ze = sum(gamma[k] + ch * ((-e_S[k] % R) * lam[k]) for k in range(t)) % R
    z = [(beta_j[ii] + ch * (r * a_S[0][ii] * lam[0]) + sum(beta_k(k)[ii] + ch * (r * a_S[k][ii] * lam[k]) for k in range(1, t))) % R for ii in range(nP)]
    zhp = [(beta_j[Hid.index(i)] + ch * (pub_a[Pub.index(i)] * r)) % R for i in HidPub]
    return op.enc(A_) + op.enc(B_) + b48(ch) + b48(zr) + b48(ze), b"".join(b48(v) for v in z), b"".join(b48(v) for v in zhp)


def _fields(b, count):
    return [int.from_bytes(b[48 * i:48 * i + 48], "big") for i in range(count)]


def _parse_pub(op, pp, h49, used, pk=None):
    g1, ok = op.dec(pp[:49])
    g2, ok2 = op.g2dec(pp[49:146])
    w, ok3 = op.g2dec(pk) if pk is not None else (None, True)
    h = {i: op.dec(h49[49 * i:49 * i + 49]) for i in used}
    if not (ok and ok2 and ok3 and all(v[1] for v in h.values())):
        return None
    return g1, g2, w, {i: v[0] for i, v in h.items()}


def expected_verify(op, pp, h49, pk, Prv, Rev, crev49, fixed242, z48, zhp48, rev48):
    """verify_pres.cpp:6-46 composed from the oracle on the wire bytes; rev48: the revealed public values in ascending Pub position.  0xff where
    the reference would throw, None when pp / a used h / pk does not decode."""
    m = len(h49) // 49
    _, _, HidPub, RevPub, _ = sets(m, Prv, Rev)
    pub = _parse_pub(op, pp, h49, list(Prv) + HidPub, pk)
    if pub is None:
        return None
    _, g2, w, h = pub
    pts = []
    for rec in (fixed242[:49], fixed242[49:98], crev49):
        pt, ok = op.dec(rec)
        if not ok:
            return 0xff
        pts.append(pt)
    A_, B_, C_rev = pts
    ch, zr, ze = _fields(fixed242[98:], 3)
    z, zhp, rev = _fields(z48, len(Prv)), _fields(zhp48, len(HidPub)), _fields(rev48, len(RevPub))
    if any(v >= R for v in [ch, zr, ze] + z + zhp + rev):
        return 0xff
    C_hid = op.prod(op.prod(None, [h[i] for i in Prv], z), [h[i] for i in HidPub], zhp)
    U = op.add(op.add(op.add(op.mul(B_, (R - ch) % R), op.mul(C_rev, zr)), C_hid), op.mul(A_, ze))
    return 1 if ch == challenge(op, U, A_, B_, rev) and op.o.pair(A_, w) == op.o.pair(B_, g2) else 0


def expected_pres(op, pp, h49, Prv, Rev, t, A49, D49, lam48, es48, as48, crev49, cpub49, pub48, rnd):
    """cred_pres from the wire bytes of ONE presentation: (fixed_242, z, zhp, status); None when pp / a used h does not decode.  Where the
    reference would throw — A, D, C_rev or C_pub does not decode, a Zp field >= r — status 0xff and records of 0xff."""
    m, nP = len(h49) // 49, len(Prv)
    Pub, Hid, HidPub, RevPub, _ = sets(m, Prv, Rev)
    pub = _parse_pub(op, pp, h49, Hid)
    if pub is None:
        return None
    h = pub[3]
    bad = b"\xff" * 242, b"\xff" * (48 * nP), b"\xff" * (48 * len(HidPub)), 0xff
    pts = [op.dec(rec) for rec in (A49, D49, crev49, cpub49)]
    lam, es, a, pa = _fields(lam48, t), _fields(es48, t), _fields(as48, t * nP), _fields(pub48, len(Pub))
    if not all(ok for _, ok in pts) or any(v >= R for v in lam + es + a + pa):
        return bad
    A, D, C_rev, C_pub = (pt for pt, _ in pts)
    v = [int.from_bytes(rnd[32 * i:32 * i + 32], "big") % R for i in range(len(rnd) // 32)]
    assert len(v) == rnd_count(m, Prv, Rev, t)
    r, alpha, o_bj, o_g = v[0], v[1], 2 + (t - 1) * nP, 2 + (t - 1) * nP + len(Hid)
    A_, B_ = op.mul(A, r), op.mul(op.add(C_pub, D), r)
    # one flat list of (point, exponent) terms
    terms = [(C_rev, alpha)] + [(h[Hid[ii]], v[o_bj + ii]) for ii in range(len(Hid))] + [(A_, v[o_g + k]) for k in range(t)]
    terms += [(h[Prv[y % nP]], v[2 + y]) for y in range((t - 1) * nP)]
    U = bytes(96)
    for pt, k in terms:
        U = op.add(U, op.mul(pt, k))
    ch = challenge(op, U, A_, B_, [pa[k] for k in RevPub])
    zr = (alpha + ch * r) % R
    ze = (sum(v[o_g:o_g + t]) - ch * sum(es[k] * lam[k] for k in range(t))) % R
    z = [(v[o_bj + ii] + sum(v[2 + (k - 1) * nP + ii] for k in range(1, t)) + ch * r * sum(a[k * nP + ii] * lam[k] for k in range(t))) % R for ii in range(nP)]
    zhp = [(v[o_bj + Hid.index(i)] + ch * r * pa[Pub.index(i)]) % R for i in HidPub]
    return op.enc(A_) + op.enc(B_) + b48(ch) + b48(zr) + b48(ze), b"".join(map(b48, z)), b"".join(map(b48, zhp)), 0


# ---------------------------------------------------------------- whole chains: one holder group, one presentation per lane
M_MAIN, PRV_MAIN, REV_MAIN, T_MAIN = 4, (0, 2), (1,), 3        # the reference's own test.cpp


class Holder:
    """generate_attributes, cred_iss, make_pres_group and make_pres_type for one credential: what a presentation is made from.  S: the t parties
    of the group (default: 0, 2, 5 of 6 when t = 3 as in test.cpp, else 0 .. t-1 of t + 1); A may be replaced (a point outside G1)."""

    def __init__(self, op, wd, Prv, Rev, t, seed, S=None, A=None, gamma=None):
        nparties = 6 if t == 3 else t + 1
        S = ((0, 2, 5) if t == 3 else tuple(range(t))) if S is None else S
        Pub = sets(wd.m, Prv, Rev)[0]
        self.pub_a, share, C = generate_attributes(op, wd, t, nparties, Prv, seed)
        self.A, e_share, D_share = cred_iss(op, wd, t, C, Pub, self.pub_a, seed + 7, gamma)
        if A is not None:
            self.A = A
        self.lam, self.D = make_pres_group(op, D_share, S)
        self.e_S, self.a_S = [e_share[i] for i in S], [share[i] for i in S]
        self.C_rev, self.C_pub = make_pres_type(op, wd, Rev, Prv, self.pub_a)
        self.t, self.Prv, self.Rev = t, tuple(Prv), tuple(Rev)
        self.revealed = [self.pub_a[k] for k in sets(wd.m, Prv, Rev)[3]]

    def pres_inputs(self, op, rnd):
        """the wire records the pres entry takes for this holder, in its argument order behind the sets"""
        return dict(A49=op.enc(self.A), D49=op.enc(self.D), lam48=b"".join(map(b48, self.lam)), es48=b"".join(map(b48, self.e_S)),
                    as48=b"".join(b48(v) for row in self.a_S for v in row), crev49=op.enc(self.C_rev), cpub49=op.enc(self.C_pub),
                    pub48=b"".join(map(b48, self.pub_a)), rnd=b"".join(v.to_bytes(32, "big") for v in rnd))

    def present(self, op, wd, rnd):
        return cred_pres(op, wd, self.A, self.e_S, self.lam, self.D, self.C_rev, self.C_pub, self.Prv, self.Rev, self.pub_a, self.a_S, rnd)


class Lane:
    """one presentation as the verify entry takes it"""

    def __init__(self, kind, crev, fixed, z, zhp, rev):
        self.kind, self.crev, self.fixed, self.z, self.zhp, self.rev = kind, crev, fixed, z, zhp, rev


def lane_of(op, wd, hd, rnd, kind="valid"):
    fixed, z, zhp = hd.present(op, wd, rnd)
    return Lane(kind, op.enc(hd.C_rev), fixed, z, zhp, b"".join(map(b48, hd.revealed)))


def valid_lanes(op, wd, Prv, Rev, t, count, seed):
    return [lane_of(op, wd, Holder(op, wd, Prv, Rev, t, seed + 100 * i), draw(seed + 100 * i + 50, rnd_count(wd.m, Prv, Rev, t))) for i in range(count)]


def with_(lane, kind, **kw):
    d = dict(crev=lane.crev, fixed=lane.fixed, z=lane.z, zhp=lane.zhp, rev=lane.rev)
    d.update(kw)
    return Lane(kind, d["crev"], d["fixed"], d["z"], d["zhp"], d["rev"])


def field(b, i, value, base=0):
    return b[:base + 48 * i] + value.to_bytes(48, "big") + b[base + 48 * i + 48:]


def plus1(b, i, base=0):
    return field(b, i, (int.from_bytes(b[base + 48 * i:base + 48 * i + 48], "big") + 1) % R, base)


def expect(op, wd, Prv, Rev, lanes):
    return bytes(expected_verify(op, wd.pp, wd.h49, wd.pk, Prv, Rev, ln.crev, ln.fixed, ln.z, ln.zhp, ln.rev) for ln in lanes)


def pack(lanes):
    """(crev_49, fixed_242, z_48, zhp_48, pub_48) of a list of lanes as the verify entry takes them"""
    return tuple(b"".join(getattr(ln, f) for ln in lanes) for f in ("crev", "fixed", "z", "zhp", "rev"))


def main_lanes(op, wd):
    """valid, tampered, degenerate, off-subgroup and malformed lanes of the small world, with their kinds"""
    from g1_torsion import P as FP, eigenpoint, enc as enc96, point_of_order
    Prv, Rev, t = PRV_MAIN, REV_MAIN, T_MAIN
    lanes = valid_lanes(op, wd, Prv, Rev, t, 8, 7100)
    b, b1 = lanes[0], lanes[1]
    hd, rnd = Holder(op, wd, Prv, Rev, t, 7100), draw(7150, rnd_count(wd.m, Prv, Rev, t))          # lane 0 again
    A_, B_, C_rev = (op.dec(rec)[0] for rec in (b.fixed[:49], b.fixed[49:98], b.crev))
    # tampered: every field
    lanes.append(with_(b, "A_ swapped", fixed=b1.fixed[:49] + b.fixed[49:]))
    lanes.append(with_(b, "B_ swapped", fixed=b.fixed[:49] + b1.fixed[49:98] + b.fixed[98:]))
    lanes.append(with_(b, "C_rev swapped", crev=b1.crev))
    for k, name in enumerate(("ch+1", "zr+1", "ze+1")):
        lanes.append(with_(b, name, fixed=plus1(b.fixed, k, 98)))
    lanes.append(with_(b, "z0+1", z=plus1(b.z, 0)))
    lanes.append(with_(b, "z1+1", z=plus1(b.z, 1)))
    lanes.append(with_(b, "zhp0+1", zhp=plus1(b.zhp, 0)))
    lanes.append(with_(b, "rev0+1", rev=plus1(b.rev, 0)))
    # each half failing alone
    lanes.append(with_(b, "A_ B_ scaled", fixed=op.enc(op.mul(A_, 7)) + op.enc(op.mul(B_, 7)) + b.fixed[98:]))
    lanes.append(lane_of(op, wd, Holder(op, wd, Prv, Rev, t, 7100, gamma=wd.gamma + 1), rnd, "pairing only fails"))
    # degenerate
    r0 = lane_of(op, wd, hd, [0] + rnd[1:], "r = 0")                     # A_ = B_ = infinity
    assert r0.fixed[0] == 0 and r0.fixed[49] == 0
    lanes.append(r0)
    lanes.append(with_(r0, "leading 00 + bytes", fixed=b"\x00" + bytes(range(1, 49)) + r0.fixed[49:]))
    x_big = int.from_bytes(A_[:48], "big") + FP                          # x >= p, same point
    lanes.append(with_(b, "x >= p", fixed=b.fixed[:1] + x_big.to_bytes(48, "big") + b.fixed[49:]))
    lanes.append(with_(b, "ch = 0", fixed=field(b.fixed, 0, 0, 98)))
    # off the subgroup
    t3 = enc96(point_of_order(3))
    te, _ = eigenpoint(10177)
    lanes.append(with_(b, "A_ + order 3", fixed=op.enc(op.add(A_, t3)) + b.fixed[49:]))
    lanes.append(with_(b, "B_ + order 3", fixed=b.fixed[:49] + op.enc(op.add(B_, t3)) + b.fixed[98:]))
    lanes.append(with_(b, "C_rev + order 3", crev=op.enc(op.add(C_rev, t3))))
    lanes.append(with_(b, "A_ eigenpoint", fixed=op.enc(enc96(te)) + b.fixed[49:]))
    lanes.append(with_(b, "C_rev eigenpoint", crev=op.enc(enc96(te))))
    # malformed
    lanes.append(with_(b, "C_rev off curve", crev=off_curve_x()))
    lanes.append(with_(b, "A_ off curve", fixed=off_curve_x() + b.fixed[49:]))
    lanes.append(with_(b, "B_ bad tag", fixed=b.fixed[:49] + b"\x05" + b.fixed[50:]))
    lanes.append(with_(b, "ch = r", fixed=field(b.fixed, 0, R, 98)))
    lanes.append(with_(b, "ze = r", fixed=field(b.fixed, 2, R, 98)))
    lanes.append(with_(b, "z1 = 2^384 - 1", z=field(b.z, 1, (1 << 384) - 1)))
    lanes.append(with_(b, "zhp0 = r", zhp=field(b.zhp, 0, R)))
    lanes.append(with_(b, "rev0 = r", rev=field(b.rev, 0, R)))
    return lanes


ZERO_KINDS = ("A_ swapped", "B_ swapped", "C_rev swapped", "ch+1", "zr+1", "ze+1", "z0+1", "z1+1", "zhp0+1", "rev0+1", "A_ B_ scaled", "pairing only fails",
              "ch = 0", "A_ + order 3", "B_ + order 3", "A_ eigenpoint", "C_rev eigenpoint")
# "C_rev + order 3" is in neither list: multiply's GLV form sends the order-3 component where the scalar zr sends it, which for this lane is
# infinity — the reference's formulas accept the lane (1), and so must the entry

BAD_KINDS = ("C_rev off curve", "A_ off curve", "B_ bad tag", "ch = r", "ze = r", "z1 = 2^384 - 1", "zhp0 = r", "rev0 = r")
