"""PS signatures from the wire formats (examples/ps/src/ps.cpp): c12381_ps_verify_wire_batch, c12381_ps_sign_batch and
c12381_ps_randomize_batch.  Signatures are made with Python integers and the CPU oracle's multiply (ps_cases.py); every verdict is the
oracle's pair_eq on the decoded lane, every signed or randomised component the oracle's g1_mul + g1_compress.  n = 65: one wavefront and
one lane."""
import ctypes

import pytest

from g1_torsion import dec, ec_add, eigenpoint, enc
from ps_cases import (ENCODE, G1, HASH, T3, T_CORNERS, Keys, b32, expected_wire, messages, mixed_wire_lanes, msg_scalars, no_point_x, rec, sign_points,
                      to_wire)
from util import R, cat, golden, prng

pytestmark = pytest.mark.gpu

N = 65
sz = ctypes.c_size_t


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


_batches = {}


def batch(orc, mode, nY, length, n=N):
    """one batch of valid signatures per (mode, nY, length), shared by the tests: (keys, messages, signatures)"""
    key = (mode, nY, length, n)
    if key not in _batches:
        keys = Keys(orc, nY, 9100 + 10 * nY + mode)
        msgs = messages(9200 + length, n, length)
        ms = [msg_scalars(orc, mode, m) for m in msgs]
        s1, s2 = sign_points(orc, keys, ms, [1 + prng(9300 + length, j) % (R - 1) for j in range(n)])
        _batches[key] = (keys, msgs, to_wire(orc, s1, s2))
    return _batches[key]


# ---------------------------------------------------------------- verify
VERIFY_CASES = ([(HASH, 1, length) for length in (0, 1, 71, 72, 73, 143, 144, 145)] +           # the SHA3-512 rate is 72
                [(ENCODE, 3, length) for length in (0, 1, 30, 31, 32, 62, 63, 93)] +             # 0, 1, 2, 3 of the 3 units in use
                [(ENCODE, 7, 200)])                                                              # 7 units: beyond the k-way product


@pytest.mark.parametrize("mode,nY,length", VERIFY_CASES)
def test_verify_mixed_lanes(ctx, oracle_port, mode, nY, length):
    keys, msgs, sigs = batch(oracle_port, mode, nY, length)
    sigs, msgs, kinds = mixed_wire_lanes(oracle_port, sigs, msgs, length)
    want = expected_wire(oracle_port, mode, keys.g2_97, keys.X2_97, keys.Y2_97, sigs, msgs)
    got = ctx.ps_verify_wire(keys.g2_97, keys.X2_97, keys.Y2_97, sigs, b"".join(msgs), length, mode)
    assert got == want, [(kinds[j], got[j], want[j]) for j in range(N) if got[j] != want[j]]
    assert all(got[j] == 1 for j in range(N) if kinds[j] == "valid")
    assert got[kinds.index("wrong_msg")] == 0 and got[kinds.index("swapped")] == 0
    for kind in ("bad_tag", "bad_tag_s2", "no_point", "no_point_s2"):
        assert got[kinds.index(kind)] == 0xff, kind


def test_verify_single_message_key_layout(ctx, oracle_port):
    """PublicKey of the single-message scheme: serialize(g2, X2, Y2), 291 bytes, passed as interior pointers"""
    keys, msgs, sigs = batch(oracle_port, HASH, 1, 73)
    pk = ctypes.create_string_buffer(keys.g2_97 + keys.X2_97 + keys.Y2_97, 291)
    base = ctypes.addressof(pk)
    out = ctypes.create_string_buffer(N)
    rc = ctx.lib.c12381_ps_verify_wire_batch(ctx.h, N, 1, 73, HASH, ctypes.c_void_p(base), ctypes.c_void_p(base + 97), ctypes.c_void_p(base + 194), sigs,
                                             b"".join(msgs), out)
    assert rc == 0 and out.raw == b"\x01" * N


@pytest.mark.parametrize("which", ["X2", "Y2", "g2"])
def test_verify_key_outside_g2(ctx, oracle_port, which):
    """a key on the twist but outside G2: the generic route, the oracle's verdicts"""
    keys, msgs, sigs = batch(oracle_port, ENCODE, 3, 93)
    sigs, msgs, kinds = mixed_wire_lanes(oracle_port, sigs, msgs, 93)
    off = oracle_port.g2_compress(cat(golden("g2")["offsubgroup_points"])[:192])
    g2, X2, Y2 = keys.g2_97, keys.X2_97, keys.Y2_97
    if which == "X2":
        X2 = off
    elif which == "Y2":
        Y2 = Y2[:97] + off + Y2[194:]
    else:
        g2 = off
    want = expected_wire(oracle_port, ENCODE, g2, X2, Y2, sigs, msgs)
    assert ctx.ps_verify_wire(g2, X2, Y2, sigs, b"".join(msgs), 93, ENCODE) == want
    assert 0xff in want and 0 in want


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_verify_key_does_not_decode(ctx, oracle_port, which):
    from crypto12381_amd.capi import C12381Error, E_POINT
    keys, msgs, sigs = batch(oracle_port, ENCODE, 3, 62)          # two units: Y2[2] takes no part
    bad = b"\x04" + bytes(96) if which % 2 else b"\x02" + bytes(47) + b"\x02" + bytes(48)          # 0x04: the 193-byte form; x.b = 2, x.a = 0: no point on the twist
    assert oracle_port.g2_decompress(bad)[1] == b"\x00"
    pk = [keys.g2_97, keys.X2_97, keys.Y2_97[:97], keys.Y2_97[97:194], keys.Y2_97[194:]]
    pk[which] = bad
    args = (pk[0], pk[1], b"".join(pk[2:]), sigs, b"".join(msgs), 62, ENCODE)
    assert ctx.ps_verify_wire(*args, strict=False) == b"\xff" * N
    with pytest.raises(C12381Error) as e:
        ctx.ps_verify_wire(*args)
    assert e.value.code == E_POINT
    pk[which] = [keys.g2_97, keys.X2_97, keys.Y2_97[:97], keys.Y2_97[97:194]][which]
    pk[4] = bad                                                   # the entry the message does not reach is not decoded
    assert ctx.ps_verify_wire(pk[0], pk[1], b"".join(pk[2:]), sigs, b"".join(msgs), 62, ENCODE) == b"\x01" * N


def test_verify_argument_errors_and_empty_batch(ctx, oracle_port):
    from crypto12381_amd.capi import E_ARG
    keys, msgs, sigs = batch(oracle_port, ENCODE, 3, 93)
    m = b"".join(msgs)
    f = ctx.lib.c12381_ps_verify_wire_batch
    out = ctypes.create_string_buffer(b"\x5a" * N, N)
    good = [keys.g2_97, keys.X2_97, keys.Y2_97, sigs, m, out]
    for n in (N, 0):                                              # argument errors come before the empty-batch rule
        for i in range(6):
            a = list(good)
            a[i] = None
            assert f(ctx.h, n, 3, 93, ENCODE, *a) == E_ARG, i
        assert f(ctx.h, n, 3, 93, 2, *good) == E_ARG              # unknown mode
        assert f(ctx.h, n, 3, 93, -1, *good) == E_ARG
        assert f(ctx.h, n, 3, 93, HASH, *good) == E_ARG           # HASH needs nY = 1
        assert f(ctx.h, n, 0, 93, HASH, *good) == E_ARG
        assert f(ctx.h, n, 3, 94, ENCODE, *good) == E_ARG         # four units, three Y2: "message is too long"
        assert f(ctx.h, n, 0, 1, ENCODE, *good) == E_ARG
    assert out.raw == b"\x5a" * N
    assert f(ctx.h, 0, 3, 93, ENCODE, *good) == 0 and out.raw == b"\x5a" * N      # n = 0 touches nothing
    assert f(ctx.h, 0, 0, 0, ENCODE, keys.g2_97, keys.X2_97, None, sigs, None, out) == 0 and out.raw == b"\x5a" * N
    assert f(ctx.h, N, 3, 93, ENCODE, *good) == 0 and out.raw == b"\x01" * N


@pytest.mark.parametrize("mode,nY,length", [(HASH, 1, 145), (ENCODE, 3, 93), (ENCODE, 7, 200)])
def test_verify_dev_equals_host(ctx, oracle_port, mode, nY, length):
    import torch
    keys, msgs, sigs = batch(oracle_port, mode, nY, length)
    sigs, msgs, kinds = mixed_wire_lanes(oracle_port, sigs, msgs, length)
    host = ctx.ps_verify_wire(keys.g2_97, keys.X2_97, keys.Y2_97, sigs, b"".join(msgs), length, mode)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    t = [dev(b) for b in (keys.g2_97, keys.X2_97, keys.Y2_97, sigs, b"".join(msgs))]
    ok = torch.full((N,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.ps_verify_wire_dev(N, nY, length, mode, *[v.data_ptr() for v in t], ok.data_ptr())
    assert ctx.sync() == 0
    assert bytes(ok.cpu().numpy()) == host


# ---------------------------------------------------------------- sign
def sign_want(orc, mode, x, y, msgs, ts):
    """serialize(G^t, (G^t)^e) per lane, e = x + sum y_i m_i, by the oracle's multiply"""
    n = len(ts)
    es = [(x + sum(yi * mi for yi, mi in zip(y, msg_scalars(orc, mode, m)))) % R for m in msgs]
    s1 = orc.g1_mul(G1 * n, b"".join(b32(t) for t in ts), 96, 8)
    s2 = orc.g1_mul(s1, b"".join(b32(e) for e in es), 96, 8)
    c1, c2 = orc.g1_compress(s1), orc.g1_compress(s2)
    return b"".join(rec(c1, 49, j) + rec(c2, 49, j) for j in range(n)), es


def sign_ts(seed):
    return list(T_CORNERS) + [R + 1, 2, (1 << 255)] + [prng(seed, j, 32) for j in range(N - len(T_CORNERS) - 3)]


@pytest.mark.parametrize("mode,nY,length", [(HASH, 1, 73), (HASH, 1, 0), (ENCODE, 3, 93), (ENCODE, 3, 0)])
@pytest.mark.parametrize("variant", ["prng", "e0_lane", "y0_x0", "y0_x1", "y0_xmax"])
def test_sign(ctx, oracle_port, mode, nY, length, variant):
    """t at its corners in the first lanes; e at its corners through the key: x = -sum y_i m_i of ONE lane's message (e = 0 there), or y = 0 and
    x = 0, 1, r - 1 (e = x in every lane)"""
    keys = Keys(oracle_port, nY, 9400)
    msgs = messages(9500 + length, N, length)
    ts = sign_ts(9600)
    x, y = keys.x, list(keys.y)
    lane = 9
    if variant == "e0_lane":
        x = -sum(yi * mi for yi, mi in zip(y, msg_scalars(oracle_port, mode, msgs[lane]))) % R
    elif variant != "prng":
        y = [0] * nY
        x = {"y0_x0": 0, "y0_x1": 1, "y0_xmax": R - 1}[variant]
    want, es = sign_want(oracle_port, mode, x, y, msgs, ts)
    got = ctx.ps_sign(x.to_bytes(48, "big"), b"".join(v.to_bytes(48, "big") for v in y), b"".join(msgs), b"".join(b32(t) for t in ts), length, mode)
    assert got == want, [j for j in range(N) if rec(got, 98, j) != rec(want, 98, j)]
    assert rec(got, 98, 0) == bytes(98) and rec(got, 98, 3) == bytes(98)             # t = 0, t = r: both components at infinity
    if variant == "e0_lane":
        assert es[lane] == 0 and rec(got, 98, lane)[49:] == bytes(49) and rec(got, 98, lane)[0] in (2, 3)
    # the signatures verify wherever t and e are not 0 mod r (an infinite component does not round-trip as a valid signature)
    g2 = oracle_port.g2_mul(bytes.fromhex(golden("g2")["generator"]), b32(prng(9401, 0) % R), 192, 1)
    X2 = oracle_port.g2_mul(g2, b32(x), 192, 1)
    Y2 = b"".join(oracle_port.g2_mul(g2, b32(v), 192, 1) for v in y)
    ok = ctx.ps_verify_wire(*(oracle_port.g2_compress(v) for v in (g2, X2, Y2)), got, b"".join(msgs), length, mode)
    live = [j for j in range(N) if ts[j] % R and es[j]]
    assert all(ok[j] == 1 for j in live) and (len(live) >= N - 3 or not any(es))


def test_sign_secret_key_out_of_range(ctx, oracle_port):
    from crypto12381_amd.capi import C12381Error, E_ARG
    keys = Keys(oracle_port, 3, 9400)
    msgs = messages(9700, N, 62)                                   # two units: y_3 takes no part
    ts = sign_ts(9701)
    t32, m = b"".join(b32(t) for t in ts), b"".join(msgs)
    want, _ = sign_want(oracle_port, ENCODE, keys.x, keys.y, msgs, ts)
    y48 = keys.y48()
    for bad_x, bad_y in ((R, None), ((1 << 384) - 1, None), (None, (0, R)), (None, (1, (1 << 256) + 5))):
        x48 = keys.x48() if bad_x is None else bad_x.to_bytes(48, "big")
        yb = y48 if bad_y is None else y48[:48 * bad_y[0]] + bad_y[1].to_bytes(48, "big") + y48[48 * bad_y[0] + 48:]
        assert ctx.ps_sign(x48, yb, m, t32, 62, ENCODE, strict=False) == b"\xff" * (98 * N)
        with pytest.raises(C12381Error) as e:
            ctx.ps_sign(x48, yb, m, t32, 62, ENCODE)
        assert e.value.code == E_ARG
        assert ctx.ps_sign(keys.x48(), y48, m, t32, 62, ENCODE) == want                  # the context stays usable
    assert ctx.ps_sign(keys.x48(), y48[:96] + R.to_bytes(48, "big"), m, t32, 62, ENCODE) == want     # the unused y_3 is not checked
    assert ctx.ps_sign((R - 1).to_bytes(48, "big"), y48, m, t32, 62, ENCODE) == sign_want(oracle_port, ENCODE, R - 1, keys.y, msgs, ts)[0]


def test_sign_dev_reports_at_sync(ctx, oracle_port):
    import torch
    from crypto12381_amd.capi import C12381Error, E_ARG
    keys = Keys(oracle_port, 1, 9400)
    msgs = messages(9710, N, 73)
    ts = sign_ts(9711)
    want, _ = sign_want(oracle_port, HASH, keys.x, keys.y, msgs, ts)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    x, xbad, y, m, t = (dev(b) for b in (keys.x48(), R.to_bytes(48, "big"), keys.y48(), b"".join(msgs), b"".join(b32(v) for v in ts)))
    out = torch.full((98 * N,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.ps_sign_dev(N, 1, 73, HASH, x.data_ptr(), y.data_ptr(), m.data_ptr(), t.data_ptr(), out.data_ptr())
    assert ctx.sync() == 0 and bytes(out.cpu().numpy()) == want
    ctx.ps_sign_dev(N, 1, 73, HASH, xbad.data_ptr(), y.data_ptr(), m.data_ptr(), t.data_ptr(), out.data_ptr())
    with pytest.raises(C12381Error) as e:
        ctx.sync()
    assert e.value.code == E_ARG and bytes(out.cpu().numpy()) == b"\xff" * (98 * N)
    assert ctx.sync() == 0


def test_sign_keeps_the_table_of_g1_mul_fixed(ctx, oracle_port):
    """sign's generator table has a slot of its own: calls of c12381_g1_mul_fixed_batch on another base before, between and after two
    signing calls return the oracle's bytes, and so does signing"""
    keys = Keys(oracle_port, 3, 9400)
    msgs = messages(9720, N, 93)
    ts = sign_ts(9721)
    want, _ = sign_want(oracle_port, ENCODE, keys.x, keys.y, msgs, ts)
    base = oracle_port.g1_mul(G1, b32(prng(9722, 0) % R), 96, 1)
    sc = b"".join(b32(prng(9723, j, 32)) for j in range(N))
    want_fixed = oracle_port.g1_mul(base * N, sc, 49, 8)
    sign = lambda: ctx.ps_sign(keys.x48(), keys.y48(), b"".join(msgs), b"".join(b32(t) for t in ts), 93, ENCODE)
    assert ctx.g1_mul_fixed(base, sc, 49) == want_fixed
    assert sign() == want
    assert ctx.g1_mul_fixed(base, sc, 49) == want_fixed
    assert ctx.g1_mul_fixed(G1, sc, 49) == oracle_port.g1_mul(G1 * N, sc, 49, 8)        # the generator itself in the shared slot
    assert sign() == want
    assert ctx.g1_mul_fixed(base, sc, 49) == want_fixed


def test_sign_argument_errors(ctx, oracle_port):
    from crypto12381_amd.capi import E_ARG
    keys = Keys(oracle_port, 3, 9400)
    m, t = b"".join(messages(9730, N, 93)), b"".join(b32(v) for v in sign_ts(9731))
    out = ctypes.create_string_buffer(b"\x5a" * (98 * N), 98 * N)
    good = [keys.x48(), keys.y48(), m, t, out]
    f = ctx.lib.c12381_ps_sign_batch
    for n in (N, 0):
        for i in range(5):
            a = list(good)
            a[i] = None
            assert f(ctx.h, n, 3, 93, ENCODE, *a) == E_ARG, i
        assert f(ctx.h, n, 3, 93, 7, *good) == E_ARG
        assert f(ctx.h, n, 3, 93, HASH, *good) == E_ARG
        assert f(ctx.h, n, 3, 94, ENCODE, *good) == E_ARG
    assert f(ctx.h, 0, 3, 93, ENCODE, *good) == 0 and out.raw == b"\x5a" * (98 * N)


# ---------------------------------------------------------------- randomise
def test_randomize(ctx, oracle_port):
    keys, msgs, sigs = batch(oracle_port, ENCODE, 3, 93)
    sig = [bytearray(rec(sigs, 98, j)) for j in range(N)]
    te, _ = eigenpoint(10177)
    pt = lambda b49: dec(oracle_port.g1_decompress(bytes(b49))[0])
    cmp = lambda p: oracle_port.g1_compress(enc(p))
    sig[1][:49] = cmp(ec_add(pt(sig[1][:49]), T3))                 # off the subgroup: an order-3 component, an eigenpoint component
    sig[2][49:] = cmp(ec_add(pt(sig[2][49:]), te))
    sig[3][:49] = cmp(T3)
    sig[4][:49], sig[4][49:] = cmp(te), cmp(ec_add(te, T3))
    sig[5][0] = 0                                                  # σ1 at infinity with junk behind the tag
    sig[6] = bytearray(98)
    bad = {7: 0, 8: 49, 10: 0}
    sig[7][0] = 5                                                  # bad tag
    sig[8][49:] = b"\x03" + no_point_x().to_bytes(48, "big")       # no point on the curve
    sig[10][0], sig[10][49] = 4, 1
    rs = [prng(9800, j, 32) for j in range(N)]
    for j, v in zip((11, 12, 13, 14, 15, 1, 3), T_CORNERS + (R - 1, 3)):
        rs[j] = v
    sigs2 = b"".join(bytes(s) for s in sig)
    out, st = ctx.ps_randomize(sigs2, b"".join(b32(r) for r in rs))
    pts, dst = oracle_port.g1_decompress(b"".join(rec(sigs2, 49, i) for i in range(2 * N)))
    want = oracle_port.g1_mul(pts, b"".join(b32(rs[i // 2]) for i in range(2 * N)), 49, 8)
    for j in range(N):
        if j in bad:
            assert dst[2 * j] == 0 or dst[2 * j + 1] == 0
            assert st[j] == 0xff and rec(out, 98, j) == b"\xff" * 98, j
        else:
            assert st[j] == 0 and rec(out, 98, j) == rec(want, 98, j), j
    assert rec(out, 98, 11) == bytes(98) and rec(out, 98, 14) == bytes(98)              # r = 0, r = r
    # a randomised valid signature still verifies
    plain = [j for j in range(16, N)]
    ok = ctx.ps_verify_wire(keys.g2_97, keys.X2_97, keys.Y2_97, out, b"".join(msgs), 93, ENCODE)
    assert all(ok[j] == 1 for j in plain) and all(rec(out, 98, j) != rec(sigs, 98, j) for j in plain)


def test_randomize_dev_in_place_and_arguments(ctx, oracle_port):
    import torch
    from crypto12381_amd.capi import E_ARG
    keys, msgs, sigs = batch(oracle_port, HASH, 1, 73)
    r32 = b"".join(b32(prng(9810, j, 32)) for j in range(N))
    host, st = ctx.ps_randomize(sigs, r32)
    assert st == bytes(N)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    s, r = dev(sigs), dev(r32)
    status = torch.full((N,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.ps_randomize_dev(N, s.data_ptr(), r.data_ptr(), s.data_ptr(), status.data_ptr())             # out = sig
    assert ctx.sync() == 0
    assert bytes(s.cpu().numpy()) == host and bytes(status.cpu().numpy()) == bytes(N)
    f = ctx.lib.c12381_ps_randomize_batch
    out, stb = ctypes.create_string_buffer(b"\x5a" * 98, 98), ctypes.create_string_buffer(b"\x5a", 1)
    good = [sigs, r32, out, stb]
    for n in (1, 0):
        for i in range(4):
            a = list(good)
            a[i] = None
            assert f(ctx.h, n, *a) == E_ARG
    assert f(ctx.h, 0, *good) == 0 and out.raw == b"\x5a" * 98 and stb.raw == b"\x5a"
