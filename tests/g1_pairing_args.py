"""Structured G1 arguments for the pairing routes: the points on E: y^2 = x^3 + 4 that a formula right for a generic (px, py) can get
wrong.  (0, +-2) of order 3 has px = 0, so every line of the Miller loop has l2 = 3 X^2 px = 0 (and py = p - 2 sits two below the top of the
canonical range); G + T3 lies outside G1 with px != 0 and pairs like G only after the final exponentiation; points of order 11 and 10177
are controls outside G1; the curve points with the smallest and the largest x; the three points (x, y), (beta x, y), (beta^2 x, y) that
share one y; ordinary multiples of the generator; infinity; and P beside -P.  Plain affine arithmetic on Python integers (g1_torsion.py),
shared by the oracle, host-sim and GPU tests: every input these tests build comes from here, never from a kernel's output.

Three layouts: a 63-lane pattern (three wavefront groups of 21 pairings) for the entries that take one G2 point per lane, a 22-lane
placement that puts one class first in a group, last in it and alone in the next, and per-element column patterns for the K-way product
over fixed G2 points (K = 1, 2, 3, 8: each element of the batch is one pattern, so one call walks the prep kernel's mask word).

`python tests/g1_pairing_args.py` prints which class reaches which route at which placement."""
import functools

import g1_torsion as g1
import g2_twist as tw
from util import P, R, prng

TRI = 21                                    # pairings per wavefront (TRI_PER_WAVE)
QUEUE_WAVES = 2048                          # api_pair.hip PAIR_QUEUE_WAVES: more wavefront groups than this take the work queue
BIG = QUEUE_WAVES * TRI + 1                 # 2049 groups, the last one a single lane
KS = (1, 2, 3, 8)
RAGGED = (1, 20, 21, 22, 64)


def _sqrt(a):
    s = pow(a, (P + 1) // 4, P)
    return s if s * s % P == a % P else None


def on_curve(pt):
    return pt is None or (pt[1] * pt[1] - pt[0] ** 3 - 4) % P == 0


def _first_on_curve(xs):
    for x in xs:
        y = _sqrt((x ** 3 + 4) % P)
        if y:
            return x, min(y, P - y)


# ---------------------------------------------------------------- the points
@functools.lru_cache(maxsize=None)
def points():
    """name -> point (None = infinity), at most 40 values"""
    g = g1.generator()
    t3 = (0, 2)
    pts = {"inf": None, "t3a": t3, "t3b": (0, P - 2), "g": g, "-g": g1.ec_neg(g), "g+t3": g1.ec_add(g, t3),
           "t11": g1.point_of_order(11), "t10177": g1.point_of_order(10177), "e10177": g1.eigenpoint(10177)[0]}
    lo = _first_on_curve(range(1, 1 << 16))
    hi = _first_on_curve(range(P - 1, P - (1 << 16), -1))
    pts["xmin+"], pts["xmin-"], pts["xmax+"], pts["xmax-"] = lo, g1.ec_neg(lo), hi, g1.ec_neg(hi)
    b = g1.ec_mul(prng(9801, 0) % R, g)
    for j in range(3):
        pts["b%d" % j] = (pow(g1.BETA, j, P) * b[0] % P, b[1])
        pts["-b%d" % j] = g1.ec_neg(pts["b%d" % j])
    for j in range(4):
        pts["m%d" % j] = g1.ec_mul(prng(9802, j) % R, g)
    return pts


CLASSES = {                                  # class -> its points
    "order 3 (px = 0)": ("t3a", "t3b"),
    "G + T3": ("g+t3",),
    "small order": ("t11", "t10177", "e10177"),
    "extreme x": ("xmin+", "xmin-", "xmax+", "xmax-"),
    "beta triple": ("b0", "b1", "b2", "-b0", "-b1", "-b2"),
    "ordinary": ("g", "m0", "m1", "m2", "m3"),
    "infinity": ("inf",),
    "P and -P": ("g", "-g", "b0", "-b0"),
}
ORDERS = {"t3a": 3, "t3b": 3, "t11": 11, "t10177": 10177, "e10177": 10177}
OUTSIDE_G1 = ("t3a", "t3b", "g+t3", "t11", "t10177", "e10177", "xmin+", "xmin-", "xmax+", "xmax-")
OFF_CURVE = "off"                            # (x, y + 1) of m0: a lane the parse rejects


def self_check():
    """the premises, on Python integers"""
    pts = points()
    assert len(pts) <= 40 and len(set(pts.values())) == len(pts)
    assert all(on_curve(v) for v in pts.values())
    assert all(0 <= c < P for v in pts.values() if v for c in v)
    for k, q in ORDERS.items():
        assert g1.ec_mul(q, pts[k]) is None and pts[k] is not None, k
    assert [k for k, v in pts.items() if v and v[0] == 0] == ["t3a", "t3b"]
    assert g1.ec_add(pts["t3a"], pts["t3b"]) is None and g1.ec_add(pts["t3a"], pts["t3a"]) == pts["t3b"]
    for k, v in pts.items():
        if v is not None:
            assert (g1.ec_mul(R, v) is None) == (k not in OUTSIDE_G1), k
    assert g1.ec_mul(3 * R, pts["g+t3"]) is None and g1.ec_add(pts["g+t3"], pts["t3b"]) == pts["g"]
    # the extremes: no curve point with a smaller x >= 1, none with a larger x < p
    assert all(_sqrt((x ** 3 + 4) % P) is None for x in range(1, pts["xmin+"][0]))
    assert all(_sqrt((x ** 3 + 4) % P) is None for x in range(pts["xmax+"][0] + 1, P))
    assert pts["xmin-"] == (pts["xmin+"][0], P - pts["xmin+"][1]) and pts["xmax+"][0] > P - (1 << 16)
    # the triple shares y, its x coordinates are the three cube roots of x^3, and it is closed under the endomorphism up to sign
    assert len({pts["b%d" % j][1] for j in range(3)}) == 1 and len({pts["b%d" % j][0] for j in range(3)}) == 3
    assert sum(pts["b%d" % j][0] for j in range(3)) % P == 0 and g1.endo(pts["b0"]) == pts["-b1"]
    for k in ("g", "b0", "b1", "b2"):
        assert g1.ec_add(pts[k], pts["-" + k]) is None
    assert not on_curve(_off_curve())
    return True


def _off_curve():
    m = points()["m0"]
    return m[0], (m[1] + 1) % P


def enc(name):
    return g1.enc(_off_curve()) if name == OFF_CURVE else g1.enc(points()[name])


def enc_neg(name):
    """the encoding of -point: what a column of the product holds when the prep step is told to negate it"""
    return g1.enc(g1.ec_neg(_off_curve() if name == OFF_CURVE else points()[name]))


def compress(name, add_p=False):
    """49 bytes: 0x02 | parity of y, then x (or x + p, which the decoder takes mod p); infinity is all zero"""
    pt = points()[name]
    if pt is None:
        return bytes(49)
    return bytes([2 | (pt[1] & 1)]) + (pt[0] + (P if add_p else 0)).to_bytes(48, "big")


# ---------------------------------------------------------------- the G2 side
@functools.lru_cache(maxsize=None)
def g2_points():
    """name -> 192 bytes: eight ordinary points of G2, infinity, and a point of order 13 (the loop passes through infinity)"""
    g = tw.generator()
    q = {"q%d" % i: tw.enc192(tw.ec_mul(prng(9803, i) % R, g)) for i in range(8)}
    q["inf2"] = bytes(192)
    q["t13"] = tw.enc192(tw.point_of_order(13))
    return q


# ---------------------------------------------------------------- 63 lanes: three groups of 21
DEGENERATE = ("t3a", "t3b", "g+t3", "t11", "t10177", "e10177", "xmin+", "xmin-", "xmax+", "xmax-", "b0", "b1", "b2", "-b0", "-b1",
              "-b2", "inf", "t3a", "t3b", "-g", "g")             # group 2, one lane each
assert len(DEGENERATE) == TRI


def pattern():
    """[(G1 name, G2 name)] of 63 lanes.  Group 0: an order-3 lane first, infinity last.  Group 1: the controls outside G1 in the
    middle, an order-3 lane last.  Group 2: degenerate throughout — every class in turn, one order-3 lane against G2 infinity and one
    against the order-13 twist point.  The fillers are four ordinary pairs, so the distinct pairs stay few."""
    lanes = []
    for i in range(3 * TRI):
        grp, pos = divmod(i, TRI)
        fill = ("m%d" % (i % 4), "q%d" % (i % 4))
        if grp == 0:
            lanes.append(("t3a", "q5") if pos == 0 else ("inf", "q6") if pos == TRI - 1 else fill)
        elif grp == 1:
            mid = {8: "g+t3", 9: "t11", 10: "t10177", 11: "e10177", 12: "g"}
            lanes.append((mid[pos], "q%d" % (pos - 8)) if pos in mid else ("t3b", "q7") if pos == TRI - 1 else fill)
        else:
            lanes.append((DEGENERATE[pos], {17: "inf2", 18: "t13"}.get(pos, "q%d" % (pos % 8))))
    assert lanes[0][0] == "t3a" and lanes[TRI - 1][0] == "inf" and lanes[2 * TRI - 1][0] == "t3b"
    assert lanes[2 * TRI + 17] == ("t3a", "inf2") and lanes[2 * TRI + 18] == ("t3b", "t13")
    return lanes


def lane_bytes(lanes):
    q = g2_points()
    return b"".join(enc(a) for a, _ in lanes), b"".join(q[b] for _, b in lanes)


def distinct(lanes):
    return sorted(set(lanes))


def tile(buf, w, n):
    return (buf * (n // (len(buf) // w) + 1))[:w * n]


def rot(buf, w, j):
    return buf[w * j:] + buf[:w * j]


def placement(name, g2="q1"):
    """22 lanes: `name` first in a group, last in it and alone in the next; ordinary pairs between"""
    return [(name, g2)] + [("m%d" % (i % 4), "q%d" % (i % 4)) for i in range(TRI - 2)] + [(name, g2), (name, g2)]


def ragged(n):
    """n lanes with an order-3 lane last: alone in the last group for n = 1, 22 and 64"""
    return [("m%d" % (i % 4), "q%d" % (i % 4)) for i in range(n - 1)] + [("t3a", "q5")]


PLACED = ("t3a", "t3b", "g+t3", "t11", "e10177", "xmin+", "xmax-", "b1", "-b2", "inf", "-g", "m0")      # one point of each class


# ---------------------------------------------------------------- column patterns of the K-way product
def column_patterns(K):
    """[(label, [G1 name per column], claims)]: one element of a K-way batch each.  claims: "one" — the Miller value is 1 whatever the
    G2 points are; "gt_one" — the GT value is 1 whatever they are; "gt_one_twin" — it is 1 when columns 0 and 1 name the same G2 point;
    "off" — the element is rejected (0xff; its claims then speak of the value the
    loop holds before that, with the off-curve column skipped)."""
    live = ["m%d" % (c % 4) if c % 5 else "b%d" % (c % 3) for c in range(K)]
    out = []
    for c in range(K):
        out.append(("inf@%d" % c, live[:c] + ["inf"] + live[c + 1:], ("one",) if K == 1 else ()))
    out.append(("all inf", ["inf"] * K, ("one", "gt_one")))
    out.append(("all order 3", ["t3a" if c % 2 == 0 else "t3b" for c in range(K)], ("gt_one",)))
    for c in sorted({0, K // 2, K - 1}):
        out.append(("all inf but %d" % c, ["inf"] * c + [live[c]] + ["inf"] * (K - 1 - c), ()))
    out.append(("alternating", [live[c] if c % 2 == 0 else "inf" for c in range(K)], ()))
    out.append(("inf alternating", ["inf" if c % 2 == 0 else live[c] for c in range(K)], ("one",) if K == 1 else ()))
    out.append(("all four kinds", [(live[c], "inf", "t3b", "-b%d" % (c % 3))[c % 4] for c in range(K)], ()))
    out.append(("negated ordinary", ["-g" if c % 2 == 0 else "-b%d" % (c % 3) for c in range(K)], ()))
    if K >= 2:
        out.append(("P, -P, rest inf", ["b0", "-b0"] + ["inf"] * (K - 2), ("gt_one_twin",)))
        out.append(("-P, P, order 3 beside", ["-g", "g"] + ["t3a"] * (K - 2), ("gt_one_twin",)))
    if K >= 3:
        out.append(("P, -P, live beside", ["b0", "-b0"] + live[2:], ()))
    out.append(("off curve beside inf", [OFF_CURVE] + ["inf"] * (K - 1), ("off", "one")))
    if K >= 2:
        out.append(("off curve beside live", live[:K - 1] + [OFF_CURVE], ("off",)))
    return out


def column_g2(K, twin):
    """the K fixed G2 names: distinct, or (twin) the same point in columns 0 and 1"""
    names = ["q%d" % c for c in range(K)]
    if twin and K >= 2:
        names[1] = names[0]
    return names


def column_bytes(K, neg_mask=0):
    """column-major G1 bytes of the batch whose element i is pattern i; the columns in neg_mask hold the negated points, for a prep
    step that negates them back"""
    pats = column_patterns(K)
    return b"".join((enc_neg if (neg_mask >> c) & 1 else enc)(cols[c]) for c in range(K) for _, cols, _ in pats)


def column_mask_words(K):
    """the mask word of each pattern as the prep kernel forms it: bit c = column c at infinity or off the curve, bit 31 = off the curve"""
    return [sum(1 << c for c in range(K) if cols[c] in ("inf", OFF_CURVE)) | (0x80000000 if OFF_CURVE in cols else 0)
            for _, cols, _ in column_patterns(K)]


class Millers:
    """the oracle's Miller values of (G1 name, G2 name) pairs, each computed once"""

    def __init__(self, oracle):
        self.oracle, self.vals = oracle, {}

    def get(self, pairs):
        new = [p for p in dict.fromkeys(pairs) if p not in self.vals]
        if new:
            a, b = lane_bytes(new)
            m = self.oracle.miller(a, b)
            for i, p in enumerate(new):
                self.vals[p] = m[576 * i:576 * i + 576]
        return b"".join(self.vals[p] for p in pairs)

    def product(self, K, twin):
        """the product over the columns of the Miller values, one per pattern of column_patterns(K).  An off-curve column counts as
        skipped (the factor 1, like infinity): what the loop holds for such an element before the entry overwrites it with 0xff."""
        pats, qn = column_patterns(K), column_g2(K, twin)
        acc = None
        for c in range(K):
            col = self.get([("inf" if cols[c] == OFF_CURVE else cols[c], qn[c]) for _, cols, _ in pats])
            acc = col if acc is None else self.oracle.gt_op("mul", acc, col)
        return [acc[576 * i:576 * i + 576] for i in range(len(pats))]


ONE = bytes(575) + b"\x01"


def differs(got, want, w, labels):
    """the labels of the records that differ, as one string ("" when none does)"""
    assert len(got) == len(want) and len(got) % w == 0, (len(got), len(want), w)
    bad = [i for i in range(len(got) // w) if got[w * i:w * i + w] != want[w * i:w * i + w]]
    return "; ".join("%d:%s" % (i, labels[i % len(labels)]) for i in bad[:12])


# ---------------------------------------------------------------- coverage
ROUTES = ("running-point loop", "normalised table", "raw table")


def coverage():
    """class -> {route: placements}, worked out from the layouts above.  The 63-lane pattern goes through the running-point loop (pair,
    miller, pair_eq, pair_product) and, as the G1 column of pair_fixed_g2 and of the K = 3 product, through both table forms; tiled to
    BIG lanes its three groups land among the whole groups and among the queued ones.  placement() adds first / last / alone for one
    point of each class on every route; the column patterns add the mask word."""
    lanes = pattern()
    cov = {}
    for cls, names in CLASSES.items():
        where = set()
        for i, (a, _) in enumerate(lanes):
            if a in names:
                pos = i % TRI
                where.add("first" if pos == 0 else "last" if pos == TRI - 1 else "mid")
                where.update(("whole group", "queued group"))        # the tiled batch repeats every lane in both regimes
        if any(n in PLACED for n in names):
            where.update(("first", "last", "alone"))
        cols = sorted({K for K in KS for _, c, _ in column_patterns(K) if any(n in names for n in c)})
        row = {r: sorted(where) for r in ROUTES}
        row["column patterns, K"] = cols
        cov[cls] = row
    return cov


def coverage_complete():
    need = {"first", "last", "alone", "whole group", "queued group"}
    return all(need <= set(row[r]) for row in coverage().values() for r in ROUTES)


if __name__ == "__main__":
    self_check()
    for cls, row in coverage().items():
        print(cls)
        for r, where in row.items():
            print("    %-22s %s" % (r, ", ".join(str(w) for w in where)))
    print("distinct points: %d, distinct pairs of the 63-lane pattern: %d, column patterns: %s"
          % (len(points()), len(distinct(pattern())), ", ".join("K=%d: %d" % (K, len(column_patterns(K))) for K in KS)))
    print("every class on every route at first / last / alone / whole / queued:", coverage_complete())
