"""Expected results of the MHAC-bbs issuance entries (include/c12381_mhac.h), each composed term by term from op.mul, op.add and op.enc on the wire
bytes and the caller's randomness — independently of the builders in mhac_bbs_cases.py, which this module imports for worlds and lanes:
    expected_attr    generate_attributes.cpp:6-37    (pub_48, ashare_48, C_49) of ONE credential
    expected_iss     cred_iss.cpp:43-85              (A_49, eshare_48, D_49, status)
    expected_group   make_pres_group.cpp:6-21        (lam_48, Dg_49, eS_48, aS_48, status)
    expected_type    make_pres_type.cpp:6-38         (crev_49, cpub_49, status)
None where pp / a used h does not decode (the entry: every byte 0xff, C12381_E_POINT) or sk >= r (C12381_E_ARG); status 0xff and records of 0xff
where the reference would throw.  polynomial and the Lagrange coefficients are written out here with exact integer powers and Fractions-free
modular inverses of their own."""
import mhac_bbs_cases as mh
from mhac_bbs_cases import b48
from util import R, prng

PARTIES_MAX = 64


def rnd_values(rnd):
    return [int.from_bytes(rnd[32 * i:32 * i + 32], "big") % R for i in range(len(rnd) // 32)]


def rnd_bytes(vals):
    return b"".join(v.to_bytes(32, "big") for v in vals)


def poly(x, a0, coeffs):
    """a0 + sum a[i] x^(i + 1) with the exact integer power, as the reference's (type)std::pow(x, i) is for every accepted shape"""
    acc = a0
    for i, a in enumerate(coeffs):
        acc += a * (x ** (i + 1))
    return acc % R


def lam_at(xs, k):
    num = den = 1
    for y, xy in enumerate(xs):
        if y != k:
            num = num * (R - xy) % R
            den = den * ((xs[k] - xy) % R) % R
    return num * pow(den, R - 2, R) % R


def _fields(b, count):
    return [int.from_bytes(b[48 * i:48 * i + 48], "big") for i in range(count)]


def _pub(op, pp, h49, used):
    g1, ok = op.dec(pp[:49])
    _, ok2 = op.g2dec(pp[49:146])
    h = {i: op.dec(h49[49 * i:49 * i + 49]) for i in used}
    if not (ok and ok2 and all(v[1] for v in h.values())):
        return None
    return g1, {i: v[0] for i, v in h.items()}


def attr_rnd_count(m, Prv, t):
    return m + len(Prv) * (t - 1)


def expected_attr(op, pp, h49, Prv, t, nparties, rnd):
    m, nP = len(h49) // 49, len(Prv)
    pub = _pub(op, pp, h49, Prv)
    if pub is None:
        return None
    h = pub[1]
    v = rnd_values(rnd)
    assert len(v) == attr_rnd_count(m, Prv, t)
    attr, a = v[:m], v[m:]
    share = [[poly(k + 1, attr[Prv[ii]], a[ii * (t - 1):(ii + 1) * (t - 1)]) for ii in range(nP)] for k in range(nparties)]
    C = []
    for k in range(nparties):
        acc = bytes(96)
        for ii in range(nP):
            acc = op.add(acc, op.mul(h[Prv[ii]], share[k][ii]))
        C.append(op.enc(acc))
    return b"".join(b48(attr[i]) for i in range(m) if i not in Prv), b"".join(b48(s) for row in share for s in row), b"".join(C)


def expected_iss(op, pp, h49, sk48, pub_idx, t, nparties, C49, pub48, rnd):
    nPub = len(pub_idx)
    pub = _pub(op, pp, h49, pub_idx)
    gamma = int.from_bytes(sk48, "big")
    if pub is None or gamma >= R:
        return None
    g1, h = pub
    bad = b"\xff" * 49, b"\xff" * (48 * nparties), b"\xff" * (49 * nparties), 0xff
    C = [op.dec(C49[49 * i:49 * i + 49]) for i in range(nparties)]
    pa = _fields(pub48, nPub)
    if not all(ok for _, ok in C) or any(x >= R for x in pa):
        return bad
    C = [pt for pt, _ in C]
    v = rnd_values(rnd)
    assert len(v) == t
    e, a = v[0], v[1:]
    xs = list(range(1, t + 1))
    C_a = g1
    for i in range(t):
        C_a = op.add(C_a, op.mul(C[i], lam_at(xs, i)))
    for ii in range(nPub):
        C_a = op.add(C_a, op.mul(h[pub_idx[ii]], pa[ii]))
    s = (gamma + e) % R
    A = op.mul(C_a, pow(s, R - 2, R) if s else 0)
    es = [poly(i + 1, e, a) for i in range(nparties)]
    D = [op.add(C[i], op.mul(A, (R - es[i]) % R)) for i in range(nparties)]
    return op.enc(A), b"".join(map(b48, es)), b"".join(op.enc(d) for d in D), 0


def expected_group(op, S, nparties, nPrv, D49, es48, as48):
    """es48 / as48 may be None: their rows are then b\"\" """
    t = len(S)
    xs = [i + 1 for i in S]
    lam = [lam_at(xs, k) for k in range(t)]
    pts = [op.dec(D49[49 * i:49 * i + 49]) for i in S]
    eS = b"" if es48 is None else b"".join(es48[48 * i:48 * i + 48] for i in S)
    aS = b"" if as48 is None or not nPrv else b"".join(as48[48 * nPrv * i:48 * nPrv * (i + 1)] for i in S)
    if not all(ok for _, ok in pts):
        return b"\xff" * (48 * t), b"\xff" * 49, b"\xff" * len(eS), b"\xff" * len(aS), 0xff
    acc = bytes(96)
    for (pt, _), l in zip(pts, lam):
        acc = op.add(acc, op.mul(pt, l))
    return b"".join(map(b48, lam)), op.enc(acc), eS, aS, 0


def expected_type(op, pp, h49, Prv, Rev, pub48):
    m = len(h49) // 49
    Pub = [i for i in range(m) if i not in Prv]
    pub = _pub(op, pp, h49, Pub)
    if pub is None:
        return None
    g1, h = pub
    pa = _fields(pub48, len(Pub))
    if any(x >= R for x in pa):
        return b"\xff" * 49, b"\xff" * 49, 0xff
    C_rev = g1
    for k, i in enumerate(Pub):
        if i in Rev:
            C_rev = op.add(C_rev, op.mul(h[i], pa[k]))
    C_pub = C_rev
    for k, i in enumerate(Pub):
        if i not in Rev:
            C_pub = op.add(C_pub, op.mul(h[i], pa[k]))
    return op.enc(C_rev), op.enc(C_pub), 0


# ---------------------------------------------------------------- batches for the GPU tests
def attr_rnd(seed, m, Prv, t, count, big_first=True):
    """per-credential randomness for attr; the first credential has values at and above r (reduced first)"""
    out = []
    for j in range(count):
        v = [prng(seed + 10 * j, i) for i in range(attr_rnd_count(m, Prv, t))]
        if j == 0 and big_first:
            v[0] = R + 5
            v[-1] = (1 << 256) - 1
        out.append(rnd_bytes([x % (1 << 256) for x in v]))
    return out


def iss_rnd(seed, t, count, big_first=True):
    out = []
    for j in range(count):
        v = [prng(seed + 10 * j, i) % (1 << 256) for i in range(t)]
        if j == 0 and big_first:
            v[0] = R + 7
            v[-1] = (1 << 256) - 1 if t > 1 else v[-1]
        out.append(rnd_bytes(v))
    return out


def cat(rows, k):
    return b"".join(r[k] for r in rows)


def ctx_fixture():
    """the module-scoped context every GPU test file of the issuance entries uses"""
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    return Context(0)


def both(call, want):
    """the entry's host and _dev form are byte-equal to `want`, output by output"""
    for dev in (False, True):
        got = call(dev=dev)
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            if g != w:
                at = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
                raise AssertionError("output %d of the %s form: %d bytes for %d, first difference at byte %d: got %s, expected %s"
                                     % (k, "_dev" if dev else "host", len(g), len(w), at, g[at:at + 49].hex(), w[at:at + 49].hex()))


def want_attr(op, wd, Prv, t, nparties, rnds):
    rows = [expected_attr(op, wd.pp, wd.h49, Prv, t, nparties, r) for r in rnds]
    return tuple(cat(rows, k) for k in range(3))


def want_iss(op, wd, sk48, pub_idx, t, nparties, creds):
    """creds: (C49, pub48, rnd) per credential"""
    rows = [expected_iss(op, wd.pp, wd.h49, sk48, pub_idx, t, nparties, *c) for c in creds]
    return tuple(cat(rows, k) for k in range(3)) + (bytes(r[3] for r in rows),)


def want_group(op, S, nparties, nPrv, rows_in):
    """rows_in: (D49, es48 or None, as48 or None) per presentation"""
    rows = [expected_group(op, S, nparties, nPrv, *r) for r in rows_in]
    return tuple(cat(rows, k) for k in range(4)) + (bytes(r[4] for r in rows),)


def want_type(op, wd, Prv, Rev, pubs):
    rows = [expected_type(op, wd.pp, wd.h49, Prv, Rev, p) for p in pubs]
    return cat(rows, 0), cat(rows, 1), bytes(r[2] for r in rows)


def honest(op, wd, Prv, t, nparties, count, seed, pub_idx=None):
    """`count` honest credentials of a world: per credential (attr result, iss result, attr rnd, iss rnd), by the expected functions"""
    Pub = [i for i in range(wd.m) if i not in Prv] if pub_idx is None else list(pub_idx)
    asc = [i for i in range(wd.m) if i not in Prv]
    out = []
    for ra, ri in zip(attr_rnd(seed, wd.m, Prv, t, count), iss_rnd(seed + 5, t, count)):
        a = expected_attr(op, wd.pp, wd.h49, Prv, t, nparties, ra)
        pub48 = b"".join(a[0][48 * asc.index(i):48 * asc.index(i) + 48] for i in Pub)
        i = expected_iss(op, wd.pp, wd.h49, b48(wd.gamma), Pub, t, nparties, a[2], pub48, ri)
        out.append((a, i, ra, ri, pub48))
    return out
