"""c12381_bbs04_sign_batch / c12381_bbs04_issue_batch: bbs04 signing and member-key issuance (the reference's examples/bbs04/src/bbs.cpp:32-59
and :17-23) from the wire formats, with the caller's randomness.  The expected signature of every lane is the Python model of
test_gpu_bbs04.py (sign composed from the CPU oracle's primitives, c by hashlib's SHA3-512 mod r); where a lane needs a member key or a scalar
that model cannot express (a forced r_x, unreduced inputs, an A outside G1, keys from the wire), model_sign below restates those lines.
Signatures made on the device go back through c12381_bbs04_verify_batch and c12381_bbs04_open_batch."""
import ctypes
import hashlib

import pytest

from g1_torsion import P as FP, eigenpoint, enc, point_of_order
from test_gpu_bbs04 import Keys, Ops, expected_open, expected_verify, sign
from util import R, cat, golden, prng

pytestmark = pytest.mark.gpu

MSG_LEN = 32
TOP = (1 << 256) - 1


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


def _b48(k):
    return k.to_bytes(48, "big")


def rnd_bytes(rnd):
    return b"".join(v.to_bytes(32, "big") for v in rnd)


def seed_rnd(seed):
    """the seven scalars test_gpu_bbs04.sign draws: alpha, beta, r_alpha, r_beta, r_x, r_delta1, r_delta2"""
    return [prng(seed, i) % R for i in range(7)]


def gsk_of(op, k, member):
    A, x = k.members[member]
    return op.enc(A) + _b48(x)


def msg_of(seed, i, msg_len=MSG_LEN):
    return prng(seed, i, max(msg_len, 1)).to_bytes(max(msg_len, 1), "big")[:msg_len]


def model_sign(op, k, gsk97, msg, rnd):
    """sign (bbs.cpp:32-59) from a wire member key and seven scalars below 2^256 (reduced mod r first); None where parse<G1, Zp> terminates"""
    A, ok = op.dec(gsk97[:49])
    x = int.from_bytes(gsk97[49:], "big")
    if not ok or x >= R:
        return None
    a, b, ra, rb, rx, rd1, rd2 = (v % R for v in rnd)
    T1, T2 = op.mul(k.u, a), op.mul(k.v, b)
    T3 = op.add(A, op.mul(k.h, a + b))
    R1, R2 = op.mul(k.u, ra), op.mul(k.v, rb)
    R3 = op.pair2(op.add(op.mul(T3, rx), op.mul(k.h, -(rd1 + rd2))), k.g2, op.mul(k.h, -(ra + rb)), k.w)
    R4 = op.add(op.mul(T1, rx), op.mul(k.u, -rd1))
    R5 = op.add(op.mul(T2, rx), op.mul(k.v, -rd2))
    tr = msg + b"".join(op.enc(t) for t in (T1, T2, T3, R1, R2)) + R3 + op.enc(R4) + op.enc(R5)
    assert len(tr) == len(msg) + 919
    c = int.from_bytes(hashlib.sha3_512(tr).digest(), "big") % R
    cx = c * x % R
    f = [c, (ra + c * a) % R, (rb + c * b) % R, (rx + cx) % R, (rd1 + a * cx) % R, (rd2 + b * cx) % R]
    return op.enc(T1) + op.enc(T2) + op.enc(T3) + b"".join(_b48(v) for v in f)


def pack(lanes):
    """lanes (gsk97, msg, rnd7) -> the three input buffers"""
    return b"".join(ln[0] for ln in lanes), b"".join(ln[1] for ln in lanes), b"".join(rnd_bytes(ln[2]) for ln in lanes)


def device_sign(ctx, k, lanes, msg_len=MSG_LEN, **kw):
    gsk, msgs, rnd = pack(lanes)
    return ctx.bbs04_sign(k.gpk, gsk, msgs, rnd, msg_len, **kw)


def split(sig):
    return [sig[435 * j:435 * j + 435] for j in range(len(sig) // 435)]


@pytest.fixture(scope="module")
def world(oracle_port):
    """64 distinct lanes over three members: (gsk, msg, rnd) and the model's signature, computed once"""
    op = Ops(oracle_port)
    k = Keys(op, 9400)
    lanes, want = [], []
    for i in range(64):
        msg = msg_of(11000, i)
        lanes.append((gsk_of(op, k, i % 3), msg, seed_rnd(11100 + i)))
        want.append(sign(op, k, i % 3, msg, 11100 + i))
    assert model_sign(op, k, *lanes[5]) == want[5]          # the restatement is the model
    return op, k, lanes, want


def tiled(world, n):
    """n lanes drawn from the 64 distinct ones: their indices, the three input buffers, the expected signatures"""
    op, k, lanes, want = world
    idx = [(j * 37) % 64 for j in range(n)]
    one = [pack([ln]) for ln in lanes]
    return idx, tuple(b"".join(one[i][f] for i in idx) for f in range(3)), b"".join(want[i] for i in idx)


def dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")


def device_sign_dev(ctx, k, packed, msg_len=MSG_LEN):
    import torch
    gsk, msgs, rnd = packed
    n = len(gsk) // 97
    d_gpk, d_gsk, d_msg, d_rnd = dev(k.gpk), dev(gsk), dev(msgs or b"\0"), dev(rnd)
    d_sig = torch.full((435 * n,), 0x5a, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.bbs04_sign_dev(n, msg_len, d_gpk.data_ptr(), d_gsk.data_ptr(), d_msg.data_ptr(), d_rnd.data_ptr(), d_sig.data_ptr(), d_st.data_ptr())
    assert ctx.sync() == 0
    return d_sig, d_st


# ---------------------------------------------------------------- 1. byte parity
@pytest.mark.parametrize("msg_len", [0, 16, 17, 32])
def test_byte_parity(ctx, oracle_port, msg_len):
    """transcripts of 919, 935 (both SHA3 padding bits in one byte), 936 (a whole padding block) and 951 bytes"""
    op = Ops(oracle_port)
    k = Keys(op, 9400)
    lanes, want = [], []
    for i in range(24):
        msg = msg_of(11200 + msg_len, i, msg_len)
        lanes.append((gsk_of(op, k, i % 3), msg, seed_rnd(11300 + 100 * msg_len + i)))
        want.append(sign(op, k, i % 3, msg, 11300 + 100 * msg_len + i))
    sig, st = device_sign(ctx, k, lanes, msg_len)
    assert st == bytes(24)
    bad = [j for j in range(24) if split(sig)[j] != want[j]]
    assert not bad, bad


# ---------------------------------------------------------------- 2. round trip and sizes
@pytest.mark.parametrize("n", [1, 65, 4099])
def test_round_trip_host_and_dev(ctx, world, n):
    op, k, _, _ = world
    idx, packed, want = tiled(world, n)
    sig, st = ctx.bbs04_sign(k.gpk, packed[0], packed[1], packed[2], MSG_LEN)
    assert st == bytes(n)
    assert sig == want
    d_sig, d_st = device_sign_dev(ctx, k, packed)
    assert bytes(d_st.cpu().numpy().tobytes()) == bytes(n)
    assert bytes(d_sig.cpu().numpy().tobytes()) == want
    assert ctx.bbs04_verify(k.gpk, sig, packed[1], MSG_LEN) == b"\x01" * n
    out, ost = ctx.bbs04_open(k.gmsk, sig)
    assert ost == bytes(n)
    members = [op.enc(k.members[m][0]) for m in range(3)]
    assert out == b"".join(members[i % 3] for i in idx)


def test_two_chunks(ctx, world):
    """n = 2^18 + 3: the second chunk reads gsk, rnd and msgs and writes sig and status at its own offsets"""
    import torch
    op, k, _, _ = world
    n = (1 << 18) + 3
    idx, packed, want = tiled(world, n)
    d_sig, d_st = device_sign_dev(ctx, k, packed)
    assert bytes(d_st.cpu().numpy().tobytes()) == bytes(n)
    assert bytes(d_sig.cpu().numpy().tobytes()) == want
    d_gpk, d_msg = dev(k.gpk), dev(packed[1])
    d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.bbs04_verify_dev(n, MSG_LEN, d_gpk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), d_ok.data_ptr())
    assert ctx.sync() == 0
    assert bytes(d_ok.cpu().numpy().tobytes()) == b"\x01" * n


# ---------------------------------------------------------------- 3. edge lanes
def test_edge_lanes(ctx, world, oracle_port):
    op, k, _, _ = world
    A0, x0 = k.members[0]
    g0 = gsk_of(op, k, 0)
    base = seed_rnd(11400)
    names, lanes = [], []

    def lane(name, gsk, rnd, i):
        names.append(name); lanes.append((gsk, msg_of(11401, i), rnd))

    def forced(**kw):
        r = list(base)
        for pos, v in kw.items():
            r[int(pos[1:])] = v
        return r

    lane("alpha = 0", g0, forced(p0=0), 0)
    lane("beta = 0", g0, forced(p1=0), 1)
    lane("alpha + beta = 0", g0, forced(p1=R - base[0]), 2)                 # T3 = A
    lane("rx = 0", g0, forced(p4=0), 3)
    lane("all zero", g0, [0] * 7, 4)                                        # every R at infinity, R3 = 1
    lane("alpha = 2^256 - 1", g0, forced(p0=TOP), 5)
    lane("r_beta = r", g0, forced(p3=R), 6)
    lane("rx = r + 5, r_delta1 = 2r + 1", g0, forced(p4=R + 5, p5=2 * R + 1), 7)
    lane("every scalar 2^256 - 1", g0, [TOP] * 7, 8)
    lane("x = 0", op.enc(A0) + _b48(0), base, 9)
    lane("A = 49 zeros", bytes(49) + _b48(x0), base, 10)
    lane("A = 00 + bytes", b"\x00" + bytes(range(1, 49)) + _b48(x0), base, 11)
    t3 = enc(point_of_order(3))
    te, _ = eigenpoint(10177)
    lane("A + order 3", op.enc(op.add(A0, t3)) + _b48(x0), base, 12)
    lane("A = eigenpoint", op.enc(enc(te)) + _b48(x0), base, 13)
    lane("A = order 3", op.enc(t3) + _b48(x0), base, 14)
    a49 = op.enc(A0)
    x_big = int.from_bytes(a49[1:], "big") + FP
    assert x_big < 1 << 384
    lane("A with x >= p", a49[:1] + _b48(x_big) + _b48(x0), base, 15)
    lane("x = r - 1", a49 + _b48(R - 1), base, 16)
    want = [model_sign(op, k, *ln) for ln in lanes]
    assert all(w is not None for w in want)
    assert want[2][98:147] == a49 and want[4][:98] == bytes(98)            # T3 = A; T1 = T2 = infinity
    assert want[5] == model_sign(op, k, g0, lanes[5][1], forced(p0=TOP % R)) and want[15] == model_sign(op, k, g0, lanes[15][1], base)
    sig, st = device_sign(ctx, k, lanes)
    assert st == bytes(len(lanes))
    bad = [names[j] for j in range(len(lanes)) if split(sig)[j] != want[j]]
    assert not bad, bad
    ok = ctx.bbs04_verify(k.gpk, sig, b"".join(ln[1] for ln in lanes), MSG_LEN)
    want_ok = bytes(expected_verify(op, k.gpk, w, ln[1]) for w, ln in zip(want, lanes))
    assert ok == want_ok, [(nm, a, b) for nm, a, b in zip(names, ok, want_ok) if a != b]
    by = dict(zip(names, want_ok))
    for nm in ("alpha = 0", "beta = 0", "alpha + beta = 0", "rx = 0", "all zero", "alpha = 2^256 - 1", "r_beta = r", "every scalar 2^256 - 1",
               "A with x >= p"):
        assert by[nm] == 1, nm                                              # signatures of a real member key stay valid at the edges


# ---------------------------------------------------------------- 4. rejected lanes
def _off_curve_x():
    x = 5
    while pow((x ** 3 + 4) % FP, (FP - 1) // 2, FP) == 1:
        x += 1
    return b"\x02" + x.to_bytes(48, "big")


@pytest.mark.parametrize("kind", ["A off curve", "A tag 05", "x = r", "x = 2^384 - 1"])
def test_rejected_lane(ctx, world, kind):
    op, k, lanes, want = world
    good = gsk_of(op, k, 1)
    bad_gsk = {"A off curve": _off_curve_x() + good[49:], "A tag 05": b"\x05" + good[1:], "x = r": good[:49] + _b48(R),
               "x = 2^384 - 1": good[:49] + b"\xff" * 48}[kind]
    assert model_sign(op, k, bad_gsk, lanes[0][1], lanes[0][2]) is None
    batch = lanes[:2] + [(bad_gsk, lanes[2][1], lanes[2][2])] + lanes[3:5]
    sig, st = device_sign(ctx, k, batch)                                    # strict: the return code is OK
    assert st == b"\x00\x00\xff\x00\x00"
    got = split(sig)
    assert got[2] == b"\xff" * 435
    assert [got[j] for j in (0, 1, 3, 4)] == [want[j] for j in (0, 1, 3, 4)]
    d_sig, d_st = device_sign_dev(ctx, k, pack(batch))                      # over buffers filled with 0x5a: nothing stale
    assert bytes(d_st.cpu().numpy().tobytes()) == st and bytes(d_sig.cpu().numpy().tobytes()) == sig


# ---------------------------------------------------------------- 5. other keys
def _rekey(op, k):
    k.gpk = op.enc(k.g1) + op.o.g2_compress(k.g2) + op.enc(k.h) + op.enc(k.u) + op.enc(k.v) + op.o.g2_compress(k.w)
    return k


@pytest.mark.parametrize("kind", ["w at infinity", "w outside G2", "u + order 3", "h + order 3", "v eigenpoint"])
def test_other_keys(ctx, oracle_port, kind):
    """the generic route of the k = 2 product (w) and the generic G1 kernel behind a fixed-base column (u, h, v outside G1)"""
    op = Ops(oracle_port)
    if kind == "w at infinity":
        k = Keys(op, 9420, gamma=0)
        assert k.w == bytes(192)
    elif kind == "w outside G2":
        k = Keys(op, 9421, w=cat(golden("g2")["offsubgroup_points"])[:192])
    else:
        k = Keys(op, 9440)
        t3 = enc(point_of_order(3))
        if kind == "u + order 3":
            k.u = op.add(k.u, t3)
        elif kind == "h + order 3":
            k.h = op.add(k.h, t3)
        else:
            k.v = enc(eigenpoint(10177)[0])
        _rekey(op, k)
    lanes = [(gsk_of(op, k, i % 3), msg_of(11500, i), seed_rnd(11510 + i)) for i in range(5)]
    lanes.append((lanes[0][0], lanes[0][1], [3, 0, 0, 0, 1, 0, 0]))        # tiny scalars on the generic kernel
    want = [model_sign(op, k, *ln) for ln in lanes]
    sig, st = device_sign(ctx, k, lanes)
    assert st == bytes(len(lanes))
    assert split(sig) == want
    ok = ctx.bbs04_verify(k.gpk, sig, b"".join(ln[1] for ln in lanes), MSG_LEN)
    assert ok == bytes(expected_verify(op, k.gpk, w, ln[1]) for w, ln in zip(want, lanes))
    if kind == "w at infinity":
        assert ok == b"\x01" * len(lanes)


def test_undecodable_gpk(ctx, world):
    from crypto12381_amd.capi import C12381Error, E_POINT
    op, k, lanes, want = world

    class Bad:
        gpk = k.gpk[:195] + b"\x05" + k.gpk[196:]                           # u's tag
    sig, st = device_sign(ctx, Bad, lanes[:5], strict=False)
    assert st == b"\xff" * 5 and sig == b"\xff" * (435 * 5)
    with pytest.raises(C12381Error) as e:
        device_sign(ctx, Bad, lanes[:5])
    assert e.value.code == E_POINT
    sig, st = device_sign(ctx, k, lanes[:2])                                # the context recovers
    assert st == bytes(2) and split(sig) == want[:2]


# ---------------------------------------------------------------- 6. arguments
def test_arguments(ctx, world):
    from crypto12381_amd.capi import E_ARG
    op, k, lanes, want = world
    gsk, msg, rnd = lanes[0][0], lanes[0][1], rnd_bytes(lanes[0][2])
    lib = ctx.lib
    sig = ctypes.create_string_buffer(b"\x5a" * 435, 435)
    st = ctypes.create_string_buffer(b"\x5a", 1)
    args = [k.gpk, gsk, msg, rnd, sig, st]
    for i in range(6):
        a = list(args)
        a[i] = None
        assert lib.c12381_bbs04_sign_batch(ctx.h, 1, MSG_LEN, *a) == E_ARG, i
        assert lib.c12381_bbs04_sign_batch_dev(ctx.h, 1, MSG_LEN, *a) == E_ARG, i
    assert lib.c12381_bbs04_sign_batch(None, 1, MSG_LEN, *args) == E_ARG
    assert lib.c12381_bbs04_sign_batch(ctx.h, 0, MSG_LEN, *args) == 0
    assert sig.raw == b"\x5a" * 435 and st.raw == b"\x5a"                   # n = 0 touches nothing
    out = ctypes.create_string_buffer(b"\x5a" * 97, 97)
    gamma, x = (5).to_bytes(32, "big"), (7).to_bytes(32, "big")
    iargs = [k.gpk, gamma, x, out]
    for i in range(4):
        a = list(iargs)
        a[i] = None
        assert lib.c12381_bbs04_issue_batch(ctx.h, 1, *a) == E_ARG, i
        assert lib.c12381_bbs04_issue_batch_dev(ctx.h, 1, *a) == E_ARG, i
    assert lib.c12381_bbs04_issue_batch(ctx.h, 0, *iargs) == 0
    assert out.raw == b"\x5a" * 97
    # msg_len = 0 with msgs = NULL
    lane0 = (gsk, b"", lanes[0][2])
    assert lib.c12381_bbs04_sign_batch(ctx.h, 1, 0, k.gpk, gsk, None, rnd, sig, st) == 0
    assert st.raw == b"\x00" and sig.raw == model_sign(op, k, *lane0)
    assert device_sign(ctx, k, [lane0], 0) == (sig.raw, b"\x00")


# ---------------------------------------------------------------- 7. issuance
def expected_issue(op, k, gamma, xs):
    out = b""
    for x in xs:
        s = (gamma + x) % R
        out += op.enc(op.mul(k.g1, pow(s, -1, R) if s else 0)) + _b48(x % R)
    return out


@pytest.mark.parametrize("g1_kind", ["in G1", "g1 + order 3"])
def test_issue(ctx, oracle_port, g1_kind):
    from crypto12381_amd.capi import C12381Error, E_POINT
    import torch
    op = Ops(oracle_port)
    k = Keys(op, 9450)
    if g1_kind != "in G1":
        k.g1 = op.add(k.g1, enc(point_of_order(3)))
        _rekey(op, k)
    gamma = k.gamma
    xs = [prng(11600, i) % R for i in range(37)]
    xs += [R - gamma, 2 * R - gamma, 0, 1, R - 1, R, (prng(11601, 0) % R) + R, TOP]          # gamma + x = 0 (49 zeros), unreduced x
    for g in (gamma, gamma + R):                                                              # gamma is reduced as well
        want = expected_issue(op, k, gamma, xs)
        # gamma + x = 0: A = g1^0, infinity for g1 in G1; PAIR_G1mul sends a g1 outside G1 to the point of order 3 at x = 0 instead
        assert want[97 * 37:97 * 37 + 49] == (bytes(49) if g1_kind == "in G1" else b"\x03" + bytes(48))
        x32 = b"".join(x.to_bytes(32, "big") for x in xs)
        got = ctx.bbs04_issue(k.gpk, g.to_bytes(32, "big"), x32)
        bad = [j for j in range(len(xs)) if got[97 * j:97 * j + 97] != want[97 * j:97 * j + 97]]
        assert not bad, bad
    n = len(xs)
    d_gpk, d_g, d_x = dev(k.gpk), dev(gamma.to_bytes(32, "big")), dev(x32)
    d_out = torch.full((97 * n,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.bbs04_issue_dev(n, d_gpk.data_ptr(), d_g.data_ptr(), d_x.data_ptr(), d_out.data_ptr())
    assert ctx.sync() == 0
    assert bytes(d_out.cpu().numpy().tobytes()) == want
    bad_gpk = b"\x05" + k.gpk[1:]
    assert ctx.bbs04_issue(bad_gpk, gamma.to_bytes(32, "big"), x32, strict=False) == b"\xff" * (97 * n)
    with pytest.raises(C12381Error) as e:
        ctx.bbs04_issue(bad_gpk, gamma.to_bytes(32, "big"), x32)
    assert e.value.code == E_POINT
    assert ctx.bbs04_issue(k.gpk, gamma.to_bytes(32, "big"), x32[:64]) == want[:194]          # the context recovers


def test_issue_sign_verify_open(ctx, oracle_port):
    """key generation -> sign -> verify -> open on the device: the keys issued here sign, verify and open to the issued A"""
    op = Ops(oracle_port)
    k = Keys(op, 9460)
    n = 70
    xs = [prng(11700, i) % R for i in range(n)]
    gsk = ctx.bbs04_issue(k.gpk, k.gamma.to_bytes(32, "big"), b"".join(x.to_bytes(32, "big") for x in xs))
    assert gsk == expected_issue(op, k, k.gamma, xs)
    lanes = [(gsk[97 * j:97 * j + 97], msg_of(11701, j), seed_rnd(11710 + j)) for j in range(n)]
    sig, st = device_sign(ctx, k, lanes)
    assert st == bytes(n)
    assert split(sig)[:4] == [model_sign(op, k, *ln) for ln in lanes[:4]]
    assert ctx.bbs04_verify(k.gpk, sig, b"".join(ln[1] for ln in lanes), MSG_LEN) == b"\x01" * n
    out, ost = ctx.bbs04_open(k.gmsk, sig)
    assert ost == bytes(n)
    assert out == b"".join(gsk[97 * j:97 * j + 49] for j in range(n))
    assert expected_open(op, k.gmsk, sig[:435]) == (gsk[:49], 0)
