"""Builders and labelled lanes for the BBS+ tests (the reference's examples/bbs-plus/src/bbs+.cpp): public parameters whose discrete logs are
kept — g1 = [t0]G, h0 = [th]G, h_i = [t_i]G, g2 = [s]G2, w = [gamma]g2 — so that a lane can be steered to the corners of the verification
equation e(A, w + x g2) == e(g1 + r h0 + sum m_i h_i, g2): A at infinity, B at infinity, w + x g2 at infinity, x A - B at infinity, two columns
of the per-lane sum colliding, the sum meeting +-g1, scalars at and above r.  Scalars are Python integers, points come from the CPU oracle.
Every lane carries the verdict its construction implies (ACCEPT / REJECT / THROWS); tests/test_bbs_cases.py checks those labels against the
oracle's evaluation of the equation on the CPU, the GPU tests compare the library with the oracle byte by byte.  Nothing here touches the
library under test."""
from g1_torsion import P as FP
from util import R, cat, golden, prng

G1GEN = bytes.fromhex(golden("g1")["generator"])
G2GEN = bytes.fromhex(golden("g2")["generator"])
ACCEPT, REJECT, THROWS = 1, 0, 0xff
TOP = (1 << 256) - 1

VARIANTS = ("standard", "h_k at infinity", "h0 == h_1", "h_2 == -h0", "g1 at infinity", "w at infinity")
OFF_G2_VARIANTS = ("w outside G2", "g2 outside G2")
NMSGS = (0, 1, 3, 4, 5)


def applicable(variant, nmsg):
    """the (variant, nmsg) pairs in which the variant differs from `standard`"""
    need = {"h_k at infinity": 1, "h0 == h_1": 1, "h_2 == -h0": 2}
    return nmsg >= need.get(variant, 0)


def b32(k):
    assert 0 <= k <= TOP
    return k.to_bytes(32, "big")


def inv(k):
    """mod_inverse of the reference: inverse(0) = 0"""
    return pow(k % R, R - 2, R)


def neg96(p):
    if p == bytes(96):
        return p
    return p[:48] + ((FP - int.from_bytes(p[48:], "big")) % FP).to_bytes(48, "big")


def no_point_x():
    """an x with no point on the curve"""
    x = 5
    while pow((x ** 3 + 4) % FP, (FP - 1) // 2, FP) == 1:
        x += 1
    return x


class Params:
    """setup + key_gen of bbs+.cpp:7-36 with the logs kept; t[0] belongs to g1, th to h0, t[i] to h_i (1-based)"""

    def __init__(self, orc, seed, nmsg, variant="standard"):
        assert variant in VARIANTS + OFF_G2_VARIANTS and applicable(variant, nmsg)
        self.orc, self.seed, self.nmsg, self.variant = orc, seed, nmsg, variant
        s = lambda i: prng(seed, i) % (R - 1) + 1
        self.t = [s(10 + i) for i in range(nmsg + 1)]
        self.th = s(1)
        self.gamma = s(2)
        if variant == "h_k at infinity":
            self.t[2 if nmsg >= 2 else 1] = 0
        elif variant == "h0 == h_1":
            self.t[1] = self.th
        elif variant == "h_2 == -h0":
            self.t[2] = R - self.th
        elif variant == "g1 at infinity":
            self.t[0] = 0
        elif variant == "w at infinity":
            self.gamma = 0
        pts = orc.g1_mul(G1GEN * (nmsg + 2), b"".join(b32(k) for k in [self.t[0], self.th] + self.t[1:]), 96)
        self.g1, self.h0, self.h = pts[:96], pts[96:192], pts[192:]
        self.hs = [self.h[96 * i:96 * i + 96] for i in range(nmsg)]
        self.g2 = orc.g2_mul(G2GEN, b32(s(3)), 192)
        self.w = orc.g2_mul(self.g2, b32(self.gamma), 192)
        off2 = cat(golden("g2")["offsubgroup_points"])
        if variant == "w outside G2":
            self.w = off2[192:384]
        elif variant == "g2 outside G2":
            self.g2 = off2[:192]
        self.in_g2 = variant not in OFF_G2_VARIANTS

    def public(self):
        return self.g1, self.g2, self.h0, self.h, self.w

    def b_log(self, r, m):
        """the log of B = g1 + r h0 + sum m_i h_i"""
        return (self.t[0] + r * self.th + sum(mi * ti for mi, ti in zip(m, self.t[1:]))) % R

    def a_log(self, x, r, m):
        """the log of sign()'s A = B^(1/(gamma + x))"""
        return self.b_log(r, m) * inv(self.gamma + x) % R

    def r_for(self, target, m):
        """r with b_log(r, m) == target"""
        return (target - self.b_log(0, m)) * inv(self.th) % R

    def point(self, k):
        return self.orc.g1_mul(G1GEN, b32(k % R), 96)


class Lane:
    """kind, tag and the inputs of one signature; A is 96 bytes (`a` its log where it has one)"""

    def __init__(self, kind, tag, A, x, r, m, a=None):
        self.kind, self.tag, self.A, self.x, self.r, self.m, self.a = kind, tag, A, x, r, list(m), a


def cofactor_component(orc):
    """[r]phi(P') for a point P' outside G1 (PAIR_G1mul by 1 returns P' + [r]phi(P')): it pairs to 1 with every element of G2"""
    off = cat(golden("g1")["offsubgroup_points"])[:96]
    T = orc.g1_add(orc.g1_mul(off, b32(1), 96), neg96(off), 96)
    assert T != bytes(96)
    return T


def lanes(p):
    """The main list.  Each entry is built from the logs so that its verdict follows from a (gamma + x) == b, by name:
    ACCEPT lanes satisfy it, REJECT lanes miss it, the THROWS lane has no point."""
    orc, nmsg, g = p.orc, p.nmsg, p.gamma
    rnd = lambda i, j=0: prng(p.seed + 100 + i, j) % (R - 1) + 1
    msg = lambda i: [rnd(20 + k, i) for k in range(nmsg)]
    spec = []                                                         # (kind, tag, a_log | bytes | callable, x, r, m)

    def signed(kind, x, r, m, tag=ACCEPT):
        spec.append((kind, tag, p.a_log(x, r, m), x, r, m))

    for i in range(4):
        signed("valid", rnd(0, i), rnd(1, i), msg(i))
    m = msg(10)
    r_inf = p.r_for(0, m)                                             # B at infinity: the sum meets -g1
    # the corners of the equation
    spec.append(("A inf, B inf", ACCEPT, 0, rnd(0, 10), r_inf, m))
    spec.append(("A inf, B != inf", REJECT, 0, rnd(0, 11), rnd(1, 11), m))
    spec.append(("A valid, B inf", REJECT, rnd(2, 12), rnd(0, 12), r_inf, m))
    spec.append(("x = -gamma, B inf", ACCEPT, rnd(2, 13), (R - g) % R, r_inf, m))
    spec.append(("x = -gamma, B != inf", REJECT, rnd(2, 14), (R - g) % R, rnd(1, 14), m))
    spec.append(("x = 2R - gamma, B inf", ACCEPT, rnd(2, 15), 2 * R - g, r_inf, m))
    if g:                                                             # with w at infinity these are the x = -gamma lanes again
        signed("x = gamma", g, rnd(1, 16), m)
        signed("x = 0", 0, rnd(1, 17), m)
        spec.append(("A = B / x", REJECT, p.b_log(rnd(1, 18), m) * inv(rnd(0, 18)) % R, rnd(0, 18), rnd(1, 18), m))
    spec.append(("-A", REJECT, R - p.a_log(rnd(0, 19), rnd(1, 19), m), rnd(0, 19), rnd(1, 19), m))
    # scalars at and above r: every one is reduced first
    spec.append(("x = R + 13", ACCEPT, p.a_log(13, rnd(1, 20), m), R + 13, rnd(1, 20), m))
    m_big = [R + 5] + m[1:] if nmsg else m
    spec.append(("r = R + 11, m_1 = R + 5", ACCEPT, p.a_log(rnd(0, 21), 11, [5] + m[1:] if nmsg else m), rnd(0, 21), R + 11, m_big))
    signed("r = 0, m = 0", rnd(0, 22), 0, [0] * nmsg)
    spec.append(("r = R, m = R", ACCEPT, p.a_log(rnd(0, 23), 0, [0] * nmsg), rnd(0, 23), R, [R] * nmsg))
    signed("x = R - 1", R - 1, rnd(1, 24), m)
    spec.append(("x = 2^256 - 1", ACCEPT, p.a_log(TOP % R, rnd(1, 25), m), TOP, rnd(1, 25), m))
    spec.append(("r, m = 2^256 - 1", ACCEPT, p.a_log(rnd(0, 26), TOP % R, [TOP % R] * nmsg), rnd(0, 26), TOP, [TOP] * nmsg))
    spec.append(("x = R - 1 unsigned", REJECT, p.a_log(rnd(0, 27), rnd(1, 27), m), R - 1, rnd(1, 27), m))
    # the per-lane column sum: collisions between columns, the sum meeting g1
    signed("sum = g1", rnd(0, 30), p.r_for(2 * p.t[0], m), m)          # g1_add_const doubles
    if nmsg:
        signed("r h0 = m_1 h_1", rnd(0, 31), m[0] * p.t[1] * inv(p.th) % R, m)
        signed("r h0 = -m_1 h_1", rnd(0, 32), (R - m[0] * p.t[1] * inv(p.th) % R) % R, m)
        signed("m_1 = 0", rnd(0, 33), rnd(1, 33), [0] + m[1:])
    if nmsg >= 4:                                                     # column nmsg comes from the generic kernel, column 1 from a table
        mc = m[:-1] + [(R - m[0] * p.t[1] * inv(p.t[nmsg]) % R) % R]
        signed("m_1 h_1 = -m_last h_last", rnd(0, 34), rnd(1, 34), mc)
    if nmsg >= 5:                                                     # two generic columns
        signed("m_4 h_4 = -m_5 h_5", rnd(0, 35), rnd(1, 35), m[:4] + [(R - m[3] * p.t[4] * inv(p.t[5]) % R) % R])
        signed("m_4 h_4 = m_5 h_5", rnd(0, 36), rnd(1, 36), m[:4] + [m[3] * p.t[4] * inv(p.t[5]) % R])
    # tamperings
    live = [i for i in range(nmsg) if p.t[i + 1]]                      # a block under an h_i at infinity cannot be wrong
    if live:
        i = live[-1]
        spec.append(("wrong message", REJECT, p.a_log(rnd(0, 40), rnd(1, 40), m), rnd(0, 40), rnd(1, 40), m[:i] + [(m[i] + 1) % R] + m[i + 1:]))
    if nmsg >= 2:
        spec.append(("m_1, m_2 swapped", REJECT, p.a_log(rnd(0, 41), rnd(1, 41), m), rnd(0, 41), rnd(1, 41), [m[1], m[0]] + m[2:]))
    spec.append(("wrong x", REJECT, p.a_log(rnd(0, 42), rnd(1, 42), m), (rnd(0, 42) + 5) % R, rnd(1, 42), m))
    spec.append(("wrong r", REJECT, p.a_log(rnd(0, 43), rnd(1, 43), m), rnd(0, 43), (rnd(1, 43) + 1) % R, m))
    spec.append(("2A", REJECT, 2 * p.a_log(rnd(0, 44), rnd(1, 44), m) % R, rnd(0, 44), rnd(1, 44), m))
    spec.append(("x, r swapped", REJECT, p.a_log(rnd(0, 45), rnd(1, 45), m), rnd(1, 45), rnd(0, 45), m))
    spec.append(("another key", REJECT, p.b_log(rnd(1, 46), m) * inv(g + 1 + rnd(0, 46)) % R, rnd(0, 46), rnd(1, 46), m))
    spec.append(("another lane's A", REJECT, p.a_log(rnd(0, 0), rnd(1, 0), msg(0)), rnd(0, 47), rnd(1, 47), m))
    # A as bytes: outside G1, with a cofactor component, not on the curve
    off1 = cat(golden("g1")["offsubgroup_points"])[:96]
    spec.append(("A outside G1", REJECT, off1, rnd(0, 50), rnd(1, 50), m))
    spec.append(("A + cofactor component", ACCEPT, lambda a: orc.g1_add(a, cofactor_component(orc), 96), rnd(0, 51), rnd(1, 51), m))
    spec.append(("A not on the curve", THROWS, no_point_x().to_bytes(48, "big") + (2).to_bytes(48, "big"), rnd(0, 52), rnd(1, 52), m))
    for i in range(4, 8):
        signed("valid", rnd(0, i), rnd(1, i), msg(i))

    logs = []
    for s in spec:
        a = s[2]
        logs.append(a if isinstance(a, int) else p.a_log(s[3], s[4], s[5]) if callable(a) else 0)
    pts = orc.g1_mul(G1GEN * len(spec), b"".join(b32(k) for k in logs), 96, 8)
    out = []
    for i, (kind, tag, a, x, r, m_) in enumerate(spec):
        pt = pts[96 * i:96 * i + 96]
        A = pt if isinstance(a, int) else a(pt) if callable(a) else a
        out.append(Lane(kind, tag, A, x, r, m_, logs[i] if isinstance(a, int) else None))
    return out


def valid_lanes(p, count, seed):
    """`count` further honest signatures (padding of the placement tests)"""
    sc = lambda i, j: prng(seed + i, j) % (R - 1) + 1
    rows = [(sc(0, j), sc(1, j), [sc(2 + k, j) for k in range(p.nmsg)]) for j in range(count)]
    pts = p.orc.g1_mul(G1GEN * count, b"".join(b32(p.a_log(*row)) for row in rows), 96, 8)
    return [Lane("valid", ACCEPT, pts[96 * j:96 * j + 96], *rows[j], a=p.a_log(*rows[j])) for j in range(count)]


def pack(lanes_, order=None):
    """(A, x, r, m) as the batch entries take them, m message-major; lane order[j] stands at position j"""
    order = range(len(lanes_)) if order is None else order
    sel = [lanes_[i] for i in order]
    nmsg = len(sel[0].m) if sel else 0
    return (b"".join(ln.A for ln in sel), b"".join(b32(ln.x) for ln in sel), b"".join(b32(ln.r) for ln in sel),
            b"".join(b32(ln.m[i]) for i in range(nmsg) for ln in sel))


def tags(lanes_, order=None):
    order = range(len(lanes_)) if order is None else order
    return bytes(lanes_[i].tag for i in order)


def expect(p, lanes_, order=None, nthreads=8):
    """the oracle's evaluation of the equation as written, one byte per lane"""
    return p.orc.bbs_plus_verify(*p.public(), *pack(lanes_, order), nthreads)


def sign_expect(p, lanes_, gamma=None):
    """sign() on the (x, r, m) of every lane: A = [b / (gamma + x)]G, inverse(0) = 0"""
    g = p.gamma if gamma is None else gamma
    return p.orc.g1_mul(G1GEN * len(lanes_), b"".join(b32(p.b_log(ln.r, ln.m) * inv(g + ln.x) % R) for ln in lanes_), 96, 8)


# ---------------------------------------------------------------- the wire form: serialize(A, x, r) = 49 + 48 + 48 bytes, raw message bytes
class WireLane:
    def __init__(self, kind, tag, sig, msg):
        self.kind, self.tag, self.sig, self.msg = kind, tag, bytes(sig), msg


def units(orc, msg):
    e = orc.encode_to_zp(msg)
    return [int.from_bytes(e[32 * i:32 * i + 32], "big") for i in range(len(e) // 32)]


def wire_public(p, spare_tag=None):
    """(pp.g1_g2_h0, pp.h, pk); spare_tag: the tag byte written over the LAST h entry"""
    orc = p.orc
    h49 = orc.g1_compress(p.h) if p.nmsg else b""
    if spare_tag is not None:
        h49 = h49[:-49] + bytes([spare_tag]) + h49[-48:]
    return orc.g1_compress(p.g1) + orc.g2_compress(p.g2) + orc.g1_compress(p.h0), h49, orc.g2_compress(p.w)


def wire_lanes(p, msg_len):
    """145-byte signatures over msg_len-byte messages under p (p.nmsg h entries, ceil(msg_len / 31) of them used): the parser's boundaries and
    the lanes of the main list that the wire can carry (every scalar below r, the message scalars fixed by the message bytes)"""
    orc, g = p.orc, p.gamma
    nblk = (msg_len + 30) // 31
    assert nblk <= p.nmsg
    rnd = lambda i, j=0: prng(p.seed + 300 + i, j) % (R - 1) + 1
    pad = [0] * (p.nmsg - nblk)                                        # unused h entries take no part
    spec = []                                                          # (kind, tag, a_log | bytes, x, r, msg, edit)

    def message(i):
        return prng(p.seed + 400 + msg_len, i, max(msg_len, 1)).to_bytes(max(msg_len, 1), "big")[:msg_len]

    def add(kind, tag, a, x, r, msg, edit=None):
        spec.append((kind, tag, a, x, r, msg, edit))

    def signed(kind, x, r, i, tag=ACCEPT, edit=None):
        msg = message(i)
        add(kind, tag, p.a_log(x, r, units(orc, msg) + pad), x, r, msg, edit)

    def put(off, data):
        def edit(sig):
            sig[off:off + len(data)] = data
        return edit

    def flip_tag(sig):
        sig[0] ^= 1

    def x_plus_p(sig):
        sig[1:49] = (int.from_bytes(sig[1:49], "big") + FP).to_bytes(48, "big")

    for i in range(3):
        signed("valid", rnd(0, i), rnd(1, i), i)
    # the parser
    signed("tag flipped", rnd(0, 10), rnd(1, 10), 10, REJECT, flip_tag)
    signed("padding byte in x", rnd(0, 11), rnd(1, 11), 11, THROWS, put(49 + 15, b"\x01"))
    signed("first padding byte in x", rnd(0, 12), rnd(1, 12), 12, THROWS, put(49, b"\x80"))
    signed("padding byte in r", rnd(0, 13), rnd(1, 13), 13, THROWS, put(97 + 7, b"\x01"))
    signed("x = r", 0, rnd(1, 14), 14, THROWS, put(49 + 16, b32(R)))
    signed("r-field = r", rnd(0, 15), 0, 15, THROWS, put(97 + 16, b32(R)))
    signed("x = r - 1", R - 1, rnd(1, 16), 16)
    signed("r-field = r - 1", rnd(0, 17), R - 1, 17)
    signed("r-field = 0", rnd(0, 18), 0, 18)
    signed("x = 1", 1, rnd(1, 19), 19)
    signed("A.x + p", rnd(0, 20), rnd(1, 20), 20, ACCEPT, x_plus_p)
    signed("tag 00, tail in place", rnd(0, 21), rnd(1, 21), 21, REJECT, put(0, b"\x00"))
    signed("tag 04", rnd(0, 22), rnd(1, 22), 22, THROWS, put(0, b"\x04"))
    signed("tag 05", rnd(0, 23), rnd(1, 23), 23, THROWS, put(0, b"\x05"))
    signed("x = -gamma on a valid signature", rnd(0, 24), rnd(1, 24), 24, REJECT, put(49 + 16, b32((R - g) % R)))
    # the corners of the equation that the wire can carry
    msg = message(30)
    m = units(orc, msg) + pad
    r_inf = p.r_for(0, m)
    add("A inf, B inf", ACCEPT, 0, rnd(0, 30), r_inf, msg)
    add("A inf, B != inf", REJECT, 0, rnd(0, 31), rnd(1, 31), msg)
    add("A valid, B inf", REJECT, rnd(2, 32), rnd(0, 32), r_inf, msg)
    add("x = -gamma, B inf", ACCEPT, rnd(2, 33), (R - g) % R, r_inf, msg)
    add("x = -gamma, B != inf", REJECT, rnd(2, 34), (R - g) % R, rnd(1, 34), msg)
    if g:
        add("x = gamma", ACCEPT, p.a_log(g, rnd(1, 35), m), g, rnd(1, 35), msg)
        add("x = 0", ACCEPT, p.a_log(0, rnd(1, 36), m), 0, rnd(1, 36), msg)
        add("A = B / x", REJECT, p.b_log(rnd(1, 37), m) * inv(rnd(0, 37)) % R, rnd(0, 37), rnd(1, 37), msg)
    add("-A", REJECT, R - p.a_log(rnd(0, 38), rnd(1, 38), m), rnd(0, 38), rnd(1, 38), msg)
    r2 = p.r_for(2 * p.t[0], m)
    add("sum = g1", ACCEPT, p.a_log(rnd(0, 39), r2, m), rnd(0, 39), r2, msg)
    if nblk:
        for kind, rr in (("r h0 = m_1 h_1", m[0] * p.t[1] * inv(p.th) % R), ("r h0 = -m_1 h_1", (R - m[0] * p.t[1] * inv(p.th) % R) % R)):
            add(kind, ACCEPT, p.a_log(rnd(0, 40), rr, m), rnd(0, 40), rr, msg)
    live = [i for i in range(nblk) if p.t[i + 1]]                      # a unit under an h_i at infinity cannot be wrong
    if live:
        o = 31 * live[-1]
        add("wrong message", REJECT, p.a_log(rnd(0, 41), rnd(1, 41), m), rnd(0, 41), rnd(1, 41), msg[:o] + bytes([msg[o] ^ 1]) + msg[o + 1:])
    add("wrong x", REJECT, p.a_log(rnd(0, 42), rnd(1, 42), m), (rnd(0, 42) + 5) % R, rnd(1, 42), msg)
    add("wrong r", REJECT, p.a_log(rnd(0, 43), rnd(1, 43), m), rnd(0, 43), (rnd(1, 43) + 1) % R, msg)
    add("A not on the curve", THROWS, b"\x02" + no_point_x().to_bytes(48, "big"), rnd(0, 44), rnd(1, 44), msg)
    add("A outside G1", REJECT, orc.g1_compress(cat(golden("g1")["offsubgroup_points"])[:96]), rnd(0, 45), rnd(1, 45), msg)
    a51 = orc.g1_add(p.point(p.a_log(rnd(0, 46), rnd(1, 46), m)), cofactor_component(orc), 96)
    add("A + cofactor component", ACCEPT, orc.g1_compress(a51), rnd(0, 46), rnd(1, 46), msg)
    for i in range(3, 5):
        signed("valid", rnd(0, i), rnd(1, i), i)

    logs = [s[2] if isinstance(s[2], int) else 0 for s in spec]
    c49 = orc.g1_compress(orc.g1_mul(G1GEN * len(spec), b"".join(b32(k) for k in logs), 96, 8))
    out = []
    for i, (kind, tag, a, x, r, msg_, edit) in enumerate(spec):
        sig = bytearray((c49[49 * i:49 * i + 49] if isinstance(a, int) else a) + x.to_bytes(48, "big") + r.to_bytes(48, "big"))
        if edit:
            edit(sig)
        out.append(WireLane(kind, tag, sig, msg_))
    return out


def wire_pack(wl, order=None):
    order = range(len(wl)) if order is None else order
    return b"".join(wl[i].sig for i in order), b"".join(wl[i].msg for i in order)


def wire_expect(p, wl, msg_len, checker=None, spare_tag=None):
    return (checker or p.orc).bbs_plus_verify_wire(*wire_public(p, spare_tag), *wire_pack(wl), msg_len, 8)
