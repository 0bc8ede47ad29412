"""GPU test of the C ABI's contract (include/c12381_hip.h): argument errors and empty batches of every entry, invalid points
reported as C12381_E_POINT with an all-0xff output lane while the other lanes stay valid, host forms that compute exactly
what their _dev twins compute, status collection through c12381_sync for the device-pointer entry points, and independence
of contexts."""
import ctypes

import pytest

from util import P as P_MOD, cat, golden, prng, scalars

pytestmark = pytest.mark.gpu

E_ARG, E_POINT = -1, -3


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()             # torch brings its own HIP runtime: let it load first when both live in one process
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


class In(bytes):
    """an input buffer"""


class OptIn(In):
    """an input buffer the entry also accepts as NULL"""


class Out(int):
    """an output buffer of this many bytes"""


class Fmt(int):
    pass


class Op(int):
    pass


class Flags(int):
    pass


class K(int):
    pass


class NH(int):
    pass


class Count(int):
    """a count or mode the entry bounds; `bad`: values it refuses"""
    def __new__(cls, v, bad):
        o = int.__new__(cls, v)
        o.bad = bad
        return o


def _bad(rec):
    """the record of one point with its last byte changed: off the curve (test_invalid_points_poison_only_their_lane)"""
    return rec[:-1] + bytes([rec[-1] ^ 1])


def _entries(n, bad=True):
    """Every host entry of the C ABI with its _dev twin (None: no twin), the arguments after the context, and whether one lane holds an
    off-curve point (then both forms report C12381_E_POINT).  With `bad`, lane 1 of the per-lane point inputs is off the curve."""
    g1, g2, gp = golden("g1"), golden("g2"), golden("pairing")
    lane1 = (lambda recs: recs[0] + _bad(recs[1]) + b"".join(recs[2:])) if bad else b"".join
    P = [bytes.fromhex(h) for h in g1["points"]]
    Q = [bytes.fromhex(h) for h in g2["points"]]
    C1 = [bytes.fromhex(h) for h in g1["compressed"]]
    C2 = [bytes.fromhex(h) for h in g2["compressed"]]
    pts = (P * 4)[:n]
    qts = (Q * 4)[:n]
    p_n, q_n = lane1(pts), lane1(qts)
    good_p, good_q = b"".join(pts), b"".join(qts)
    c1 = b"".join((C1[:1] + C1[24:25] + C1[2:] if bad else C1)[:n])          # compressed lane 1: a rejected encoding
    c2 = b"".join((C2[:1] + C2[16:17] + C2[2:] if bad else C2)[:n])
    sc = scalars(301, n)
    fp = b"".join((prng(302, j) % P_MOD).to_bytes(48, "big") for j in range(n))
    gt = (cat(gp["gt"]) * 2)[:576 * n]
    gt2 = (cat(gp["gt"])[576:] * 2)[:576 * n]
    gen1, gen2 = bytes.fromhex(g1["generator"])[:96], bytes.fromhex(g2["generator"])[:192]
    k, nmsg, nh, msg_len = 2, 2, 3, 40
    prod_p = lane1((P * 4)[:n * k])
    prod_q = b"".join((Q * 4)[:n * k])
    h96 = b"".join(P[5:5 + nmsg])
    pub195 = C1[3] + C2[3] + C1[4]
    sigs = b"".join(C1[5 + j] + scalars(310 + j, 3) for j in range(n))
    if bad:
        sigs = sigs[:145] + C1[24] + sigs[145 + 49:]
    digests = scalars(320, 2 * n)
    nb, nY = 2, 2
    z48 = lambda sc32: b"".join(bytes(16) + sc32[32 * j:32 * j + 32] for j in range(len(sc32) // 32))     # 48-byte Zp fields below r
    sc_k = scalars(330, n * k)
    ps_pub = [In(Q[0]), In(Q[1]), In(Q[2] + Q[3])]                           # g2, X2, Y2_0, Y2_1
    ps_m = scalars(331, n * nmsg)
    ps_sigs = b"".join(C1[5 + j] + C1[9 + j] for j in range(n))             # 98-byte wire signatures
    if bad:
        ps_sigs = ps_sigs[:98] + C1[24] + ps_sigs[98 + 49:]
    msgs = digests[:msg_len * n]
    gpk = b"".join(C1[:4]) + C2[0] + C2[1]                                    # bbs04: g1, h, u, v | g2, w
    sig435 = b"".join(C1[5 + j] + C1[6 + j] + C1[7 + j] + z48(scalars(340 + j, 6)) for j in range(n))
    if bad:
        sig435 = sig435[:435] + C1[24] + sig435[435 + 49:]
    gsk = b"".join(C1[5 + j] + z48(scalars(350 + j, 1)) for j in range(n))
    E = [
        ("fp_op_batch", "fp_op_batch_dev", [Op(0), n, In(fp), In(fp[::-1]), Out(48 * n)], False),
        ("g1_mul_batch", "g1_mul_batch_dev", [n, In(p_n), In(sc), Out(49 * n), Fmt(49)], bad),
        ("g1_mul_batch_flags", "g1_mul_batch_flags_dev", [n, In(c1), In(sc), Out(96 * n), Fmt(96), Flags(4)], bad),
        ("g1_add_batch", None, [n, In(p_n), In(good_p), Out(96 * n), Fmt(96)], bad),
        ("g1_msm", "g1_msm_dev", [n, In(p_n), In(sc), Out(49), Fmt(49)], bad),
        ("g1_msm_flags", "g1_msm_flags_dev", [n, In(c1), In(sc), Out(96), Fmt(96), Flags(4)], bad),
        ("g1_sum", "g1_sum_dev", [n, In(p_n), Out(49), Fmt(49)], bad),
        ("g1_sum_of_products", "g1_sum_of_products_dev", [n, In(p_n), In(sc), Out(96), Fmt(96)], bad),
        ("g2_mul_batch", "g2_mul_batch_dev", [n, In(q_n), In(sc), Out(97 * n), Fmt(97)], bad),
        ("g2_mul_batch_flags", "g2_mul_batch_flags_dev", [n, In(c2), In(sc), Out(192 * n), Fmt(192), Flags(4)], bad),
        ("g2_msm", "g2_msm_dev", [n, In(q_n), OptIn(sc), Out(97), Fmt(97)], bad),
        ("g2_add_batch", None, [n, In(q_n), In(good_q), Out(192 * n), Fmt(192)], bad),
        ("pair_batch", "pair_batch_dev", [n, In(p_n), In(good_q), Out(576 * n)], bad),
        ("pair_batch_flags", "pair_batch_flags_dev", [n, In(c1), In(c2), Out(576 * n), Flags(4)], bad),
        ("pair_product_batch", "pair_product_batch_dev", [n, K(k), In(prod_p), In(prod_q), Out(576 * n), Flags(0)], bad),
        ("pair_eq_batch", "pair_eq_batch_dev", [n, In(p_n), In(good_q), In(good_p), In(good_q), Out(n)], bad),
        ("g1_decompress_batch", "g1_decompress_batch_dev", [n, In(c1), Out(96 * n), Out(n)], False),
        ("g2_decompress_batch", "g2_decompress_batch_dev", [n, In(c2), Out(192 * n), Out(n)], False),
        ("miller_batch", "miller_batch_dev", [n, In(p_n), In(good_q), Out(576 * n)], bad),
        ("fexp_batch", "fexp_batch_dev", [n, In(gt), Out(576 * n)], False),
        ("gt_op_batch", "gt_op_batch_dev", [Op(0), n, In(gt), In(gt2), Out(576 * n)], False),
        ("gt_op_batch", "gt_op_batch_dev", [Op(2), n, In(gt), In(sc), Out(576 * n)], False),
        ("gt_is_unity_batch", "gt_is_unity_batch_dev", [n, In(gt), Out(n)], False),
        ("pair_fixed_g2_batch", "pair_fixed_g2_batch_dev", [n, In(p_n), In(Q[0]), Out(576 * n)], bad),
        ("g1_mul_fixed_batch", "g1_mul_fixed_batch_dev", [n, In(gen1), In(sc), Out(49 * n), Fmt(49)], False),
        ("g2_mul_fixed_batch", "g2_mul_fixed_batch_dev", [n, In(gen2), In(sc), Out(97 * n), Fmt(97)], False),
        ("bbs_plus_verify_batch", "bbs_plus_verify_batch_dev",
         [n, nmsg, In(P[0]), In(Q[0]), In(P[1]), In(h96), In(Q[1]), In(p_n), In(sc), In(sc[::-1]), In(scalars(303, n * nmsg)), Out(n)], bad),
        ("bbs_plus_verify_aggregate", "bbs_plus_verify_aggregate_dev",
         [n, nmsg, In(P[0]), In(Q[0]), In(P[1]), In(h96), In(Q[1]), In(p_n), In(sc), In(sc[::-1]), In(scalars(303, n * nmsg)),
          In(scalars(304, n, 1 << 64)), Out(4)], bad),
        ("bbs_plus_verify_wire_batch", "bbs_plus_verify_wire_batch_dev",
         [n, NH(nh), msg_len, In(pub195), In(b"".join(C1[8:8 + nh])), In(C2[4]), In(sigs), In(digests[:msg_len * n]), Out(n)], False),
        ("bbs_plus_sign_batch", "bbs_plus_sign_batch_dev",
         [n, nmsg, In(P[0]), In(P[1]), In(h96), In(scalars(305, 1)), In(sc), In(sc[::-1]), In(scalars(303, n * nmsg)), Out(96 * n)], False),
        ("g1_from_hash_batch", "g1_from_hash_batch_dev", [n, In(digests), Out(96 * n), Fmt(96)], False),
        ("g1_map_to_point_batch", None, [n, In(fp), Out(96 * n)], False),
        ("g1_clear_cofactor_batch", None, [n, In(p_n), Out(96 * n)], bad),
        ("zp_op_batch", "zp_op_batch_dev", [Op(0), n, In(sc), In(sc[::-1]), Out(32 * n)], False),
        ("zp_op_batch", "zp_op_batch_dev", [Op(4), n, In(sc), OptIn(sc), Out(32 * n)], False),
        ("zp_from_hash_batch", None, [n, In(digests), Out(32 * n)], False),
        ("zp_inner_product", "zp_inner_product_dev", [n, In(sc), OptIn(sc[::-1]), Out(32)], False),
        ("g1_mul_sum_batch", "g1_mul_sum_batch_dev", [n, Count(k, (0, 5)), In(prod_p), In(sc_k), Out(49 * n), Fmt(49), Flags(0)], bad),
        ("pair_product_fixed_g2_batch", "pair_product_fixed_g2_batch_dev",
         [n, Count(k, (0, 9)), In(prod_p), In(Q[0] + Q[1]), Out(576 * n), Flags(0)], bad),
        ("ps_verify_batch", "ps_verify_batch_dev", [n, nmsg] + ps_pub + [In(p_n), In(good_p), In(ps_m), Out(n)], bad),
        ("g1_mul_fixed_sum_batch", "g1_mul_fixed_sum_batch_dev",
         [n, Count(nb, (0, 33)), In(P[0] + P[1]), OptIn(P[2]), In(scalars(332, n * nb)), Out(49 * n), Fmt(49)], False),
        ("g2_mul_fixed_sum_batch", "g2_mul_fixed_sum_batch_dev",
         [n, Count(nb, (0, 33)), In(Q[0] + Q[1]), OptIn(Q[2]), In(scalars(333, n * nb)), Out(97 * n), Fmt(97)], False),
        ("sha3_512_batch", "sha3_512_batch_dev", [n, msg_len, In(msgs), Out(64 * n)], False),
        # bad records of the wire entries below are reported through status bytes, not C12381_E_POINT
        ("bbs04_verify_batch", "bbs04_verify_batch_dev", [n, msg_len, In(gpk), In(sig435), In(msgs), Out(n)], False),
        ("bbs04_open_batch", "bbs04_open_batch_dev", [n, In(z48(scalars(341, 2))), In(sig435), Out(49 * n), Out(n)], False),
        ("bbs04_sign_batch", "bbs04_sign_batch_dev",
         [n, msg_len, In(gpk), In(gsk), In(msgs), In(scalars(342, 7 * n)), Out(435 * n), Out(n)], False),
        ("bbs04_issue_batch", "bbs04_issue_batch_dev", [n, In(gpk), In(scalars(343, 1)), In(sc), Out(97 * n)], False),
        ("ps_verify_wire_batch", "ps_verify_wire_batch_dev",
         [n, Count(nY, (1,)), msg_len, Count(1, (2,)), In(C2[0]), In(C2[1]), In(C2[2] + C2[3]), In(ps_sigs), In(msgs), Out(n)], False),
        ("ps_verify_wire_batch", "ps_verify_wire_batch_dev",
         [n, Count(1, (2,)), msg_len, Count(0, (2,)), In(C2[0]), In(C2[1]), In(C2[2]), In(ps_sigs), In(msgs), Out(n)], False),
        ("ps_sign_batch", "ps_sign_batch_dev",
         [n, Count(nY, (1,)), msg_len, Count(1, (2,)), In(z48(scalars(344, 1))), In(z48(scalars(345, nY))), In(msgs), In(sc), Out(98 * n)], False),
        ("ps_sign_batch", "ps_sign_batch_dev",
         [n, Count(1, (2,)), msg_len, Count(0, (2,)), In(z48(scalars(344, 1))), In(z48(scalars(345, 1))), In(msgs), In(sc), Out(98 * n)], False),
        ("ps_randomize_batch", "ps_randomize_batch_dev", [n, In(ps_sigs), In(sc), Out(98 * n), Out(n)], False),
        ("ps_verify_aggregate", "ps_verify_aggregate_dev",
         [n, nmsg] + ps_pub + [In(p_n), In(good_p), In(ps_m), In(scalars(334, n, 1 << 64)), Out(4)], bad),
    ]
    return E


def _run_host(ctx, host, args, fill=0):
    """host form: returns (rc, [output bytes])"""
    outs, cargs = [], []
    for a in args:
        if isinstance(a, Out):
            outs.append(ctypes.create_string_buffer(bytes([fill]) * (int(a) or 64), int(a) or 64))
            cargs.append(outs[-1])
        elif isinstance(a, In):
            cargs.append(bytes(a) or bytes(64))
        else:
            cargs.append(a)
    rc = getattr(ctx.lib, "c12381_" + host)(ctx.h, *[_arg(a) for a in cargs])
    return rc, [o.raw for o in outs]


def _arg(a):
    from crypto12381_amd.capi import _p
    return a if isinstance(a, int) or a is None else _p(a)


def _run_dev(ctx, dev, args, fill=0):
    """_dev form on device copies of the same buffers: returns (return code, status from c12381_sync, [output bytes])"""
    import torch
    d = torch.device("cuda", 0)
    outs, cargs, keep = [], [], []
    for a in args:
        if isinstance(a, Out):
            outs.append(torch.full((int(a) or 64,), fill, dtype=torch.uint8, device=d))
            cargs.append(outs[-1].data_ptr())
        elif isinstance(a, In):
            keep.append(torch.frombuffer(bytearray(bytes(a) or b"\0" * 64), dtype=torch.uint8).to(d))
            cargs.append(keep[-1].data_ptr())
        else:
            cargs.append(a)
    torch.cuda.synchronize(d)
    rc = getattr(ctx.lib, "c12381_" + dev)(ctx.h, *[_arg(a) for a in cargs])
    st = ctx.sync()
    return rc, st, [bytes(o.cpu().numpy()) for o in outs]


def _arg_error_cases(args):
    """argument lists that each break one condition of the entry"""
    for i, a in enumerate(args):
        if isinstance(a, In) and not isinstance(a, OptIn) or isinstance(a, Out):
            yield "null arg %d" % i, args[:i] + [None] + args[i + 1:]
        elif isinstance(a, Fmt):
            yield "fmt", args[:i] + [Fmt(50)] + args[i + 1:]
        elif isinstance(a, Op):
            yield "op 9", args[:i] + [Op(9)] + args[i + 1:]
            yield "op -1", args[:i] + [Op(-1)] + args[i + 1:]
        elif isinstance(a, Flags):
            yield "flags", args[:i] + [Flags(int(a) | 0x100)] + args[i + 1:]
        elif isinstance(a, K):
            yield "k 0", args[:i] + [K(0)] + args[i + 1:]
            yield "k MAX_PROD + 1", args[:i] + [K(4)] + args[i + 1:]
        elif isinstance(a, NH):
            yield "nblk > nh", args[:i] + [NH(1)] + args[i + 1:]
        elif isinstance(a, Count):
            for v in a.bad:
                yield "arg %d = %d" % (i, v), args[:i] + [v] + args[i + 1:]


_FORMS = [(host, dev) for host, dev, _, _ in _entries(3)]
# host entries whose empty batch has a value: identity bytes of the output format, the zero scalar, a "valid" verdict
_EMPTY_VALUES = {"g1_msm": bytes(49), "g1_msm_flags": bytes(96), "g1_sum": bytes(49), "g1_sum_of_products": bytes(96), "g2_msm": bytes(97),
                 "zp_inner_product": bytes(32), "bbs_plus_verify_aggregate": (1).to_bytes(4, "little"),
                 "ps_verify_aggregate": (1).to_bytes(4, "little")}


@pytest.mark.parametrize("i", [i for i, (_, dev) in enumerate(_FORMS) if dev])
def test_host_form_equals_dev_form(ctx, i):
    """a small golden batch, lane 1 off the curve where the entry takes per-lane points: the same bytes, the same 0xff lane and the same
    status from both forms — the host form through its return, the _dev form through c12381_sync"""
    host, dev, args, bad = _entries(3)[i]
    assert ctx.sync() == 0
    rc_h, out_h = _run_host(ctx, host, args)
    rc_d, st, out_d = _run_dev(ctx, dev, args)
    assert rc_d == 0, (dev, rc_d)
    assert rc_h == st, (host, rc_h, st)
    if bad:
        assert rc_h == E_POINT, host
    if host in ("bbs_plus_verify_aggregate", "ps_verify_aggregate"):
        # the host form's verdict is an int that is 1 only when the call succeeded; the _dev form writes the verdict byte
        assert out_h[0] == (0 if bad else out_d[0][0]).to_bytes(4, "little")
        return
    assert out_h == out_d, host
    if bad and host in ("g1_mul_batch", "g2_mul_batch", "pair_batch", "pair_eq_batch"):
        lane = len(out_h[0]) // 3
        assert out_h[0][lane:2 * lane] == b"\xff" * lane, host


def test_argument_errors(ctx):
    # every host entry and its _dev twin, each argument condition on its own: C12381_E_ARG and nothing launched (the other pointers
    # are real buffers of the right size, host or device, so a missed check computes garbage instead of faulting)
    assert ctx.sync() == 0
    for host, dev, args, _ in _entries(3, bad=False):
        for what, bad_args in _arg_error_cases(args):
            assert _run_host(ctx, host, bad_args)[0] == E_ARG, (host, what)
            if dev:
                assert _run_dev(ctx, dev, bad_args)[:2] == (E_ARG, 0), (dev, what)
    lib, h = ctx.lib, ctx.h
    buf = ctypes.create_string_buffer(4096)
    n = ctypes.c_size_t(1)
    assert lib.c12381_g1_mul_batch(h, n, None, buf, buf, 49) == E_ARG
    assert lib.c12381_g1_mul_batch(h, n, buf, buf, buf, 50) == E_ARG              # unknown output format
    assert lib.c12381_g2_mul_batch(h, n, buf, buf, buf, 96) == E_ARG
    assert lib.c12381_fp_op_batch(h, 9, n, buf, buf, buf) == E_ARG                # unknown op
    assert lib.c12381_zp_op_batch(h, 0, n, buf, None, buf) == E_ARG               # binary op without b
    assert lib.c12381_pair_batch(h, n, buf, None, buf) == E_ARG
    assert lib.c12381_g1_msm(h, n, None, buf, buf, 49) == E_ARG
    assert lib.c12381_gt_op_batch(h, 7, n, buf, buf, buf) == E_ARG
    assert lib.c12381_g1_mul_batch(None, n, buf, buf, buf, 49) == E_ARG           # no context
    assert lib.c12381_create(0, None) == E_ARG
    assert lib.c12381_create(99, ctypes.byref(ctypes.c_void_p())) < 0            # no such device: fails, never a CPU fallback


def test_empty_batches(ctx):
    assert ctx.g1_mul(b"", b"", 49) == b""
    assert ctx.g2_mul(b"", b"", 97) == b""
    assert ctx.pair(b"", b"") == b""
    assert ctx.pair_eq(b"", b"", b"", b"") == b""
    assert ctx.g1_msm(b"", b"", 49) == bytes(49)                                  # the empty product is the identity
    assert ctx.g1_msm(b"", b"", 96) == bytes(96)
    assert ctx.fp_op("mul", b"", b"") == b""
    assert ctx.zp_op("inv", b"") == b""
    dec, st = ctx.g1_decompress(b"")
    assert dec == b"" and st == b""
    assert ctx.g1_mul_fixed(bytes.fromhex(golden("g1")["generator"]), b"", 49) == b""
    # every host entry: 0 without touching the stream and the outputs, or the value of the empty batch
    for host, _, args, _ in _entries(0, bad=False):
        rc, outs = _run_host(ctx, host, args, fill=0xab)
        assert rc == 0, host
        want = _EMPTY_VALUES.get(host)
        assert outs[0] == want if want is not None else all(o == b"\xab" * len(o) for o in outs), host


def test_invalid_points_poison_only_their_lane(ctx):
    from crypto12381_amd import C12381Error
    g1, g2, gp = golden("g1"), golden("g2"), golden("pairing")
    p_good = bytes.fromhex(g1["points"][0])
    p_bad = p_good[:95] + bytes([p_good[95] ^ 1])
    q_good = bytes.fromhex(g2["points"][0])
    q_bad = q_good[:191] + bytes([q_good[191] ^ 1])
    sc = scalars(961, 2)
    with pytest.raises(C12381Error) as ei:
        ctx.g2_mul(q_good + q_bad, sc, 97)
    assert ei.value.code == E_POINT
    out = ctx.g2_mul(q_good + q_bad, sc, 97, strict=False)
    assert out[97:] == b"\xff" * 97 and out[:97] == ctx.g2_mul(q_good, sc[:32], 97)
    out = ctx.g1_add(p_good + p_bad, p_good + p_good, 96, strict=False)
    assert out[96:] == b"\xff" * 96 and out[:96] == ctx.g1_add(p_good, p_good, 96)
    gt = ctx.pair(p_good + p_bad + p_good, q_good + q_good + q_bad, strict=False)
    assert gt[576:] == b"\xff" * 1152 and gt[:576] == ctx.pair(p_good, q_good)
    ok = ctx.pair_eq(p_good + p_bad, q_good + q_good, p_good + p_good, q_good + q_good, strict=False)
    assert ok == b"\x01\xff"
    with pytest.raises(C12381Error):
        ctx.g1_msm(p_good + p_bad, sc, 49)
    # a valid call after an error starts clean
    assert ctx.g1_mul(p_good, sc[:32], 49) == ctx.g1_mul(p_good, sc[:32], 49)
    # large enough for the work-queue pairing kernels: one bad lane in the middle
    n = 21 * 2100
    P = (p_good * n)[: 96 * 1000] + p_bad + (p_good * n)[96 * 1001:]
    gt = ctx.pair(P, q_good * n, strict=False)
    one = ctx.pair(p_good, q_good)
    assert gt[576 * 1000:576 * 1001] == b"\xff" * 576 and gt[:576] == one and gt[-576:] == one and gt[576 * 999:576 * 1000] == one


def test_device_pointer_entry_points_report_through_sync(ctx):
    import torch
    dev = torch.device("cuda", 0)
    g = golden("g1")
    pts, sc = cat(g["points"]), cat(g["scalars"])
    n = len(sc) // 32
    bad = bytearray(pts); bad[95] ^= 1
    dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).to(dev)
    db = torch.frombuffer(bad, dtype=torch.uint8).to(dev)
    ds = torch.frombuffer(bytearray(sc), dtype=torch.uint8).to(dev)
    out = torch.empty(49 * n, dtype=torch.uint8, device=dev)
    ctx.g1_mul_dev(n, dp.data_ptr(), ds.data_ptr(), out.data_ptr(), 49)
    assert ctx.sync() == 0
    assert bytes(out.cpu().numpy()) == cat(g["mul49"])
    ctx.g1_mul_dev(n, db.data_ptr(), ds.data_ptr(), out.data_ptr(), 49)
    assert ctx.sync() == E_POINT                                                   # collected by the sync, then cleared
    assert ctx.sync() == 0
    res = bytes(out.cpu().numpy())
    assert res[:49] == b"\xff" * 49 and res[49:] == cat(g["mul49"])[49:]


def _event_case(c, entry, orc):
    """(arguments, the same with another valid batch in every input, expected outputs) of one entry of test_stream_ordering_through_events"""
    if entry == "g1_mul_batch_dev":                                                # the golden batch; the stale one is made by the library
        g = golden("g1")
        pts, sc = cat(g["points"]), cat(g["scalars"])
        n = len(sc) // 32
        stale_p = c.g1_mul(pts, scalars(77, n), 96)                                # another valid batch
        stale_s = scalars(78, n)
        want, stale_want = cat(g["mul96"]), c.g1_mul(stale_p, stale_s, 96)
        assert want != stale_want
        return [n, In(pts), In(sc), Out(96 * n), Fmt(96)], [n, In(stale_p), In(stale_s), Out(96 * n), Fmt(96)], [want]
    import stream_cases                                                            # entries with side-stream work: batches A and B of their rows
    row = stream_cases.BY_ID[{"bbs_plus_verify_wire_batch_dev": "bbs_plus_verify_wire", "g1_msm_dev[2^15]": "g1_msm[2^15]"}[entry]]
    a, want, _ = stream_cases.case(orc, row, v=0)
    b, stale_want, _ = stream_cases.case(orc, row, v=1)
    assert want != stale_want
    return a, b, want


@pytest.mark.parametrize("entry", ["g1_mul_batch_dev", "bbs_plus_verify_wire_batch_dev", "g1_msm_dev[2^15]"])
def test_stream_ordering_through_events(entry, oracle_port):
    """include/c12381_hip.h "Stream ordering": inputs filled on ANOTHER stream behind a long-running kernel, outputs consumed on a third one —
    c12381_wait_event / c12381_record_event are the only edges (no host-side wait anywhere between the fill and the read-back).  The input
    buffers hold a different valid batch beforehand, so a library that did not wait would return that batch's (wrong) results, not an error.
    g1_mul_batch_dev never leaves the context's stream; the wire verification forks the side stream per chunk and the bucket product of 2^15
    terms sorts its window segments on two streams: c12381_record_event covers that work too ("which is joined first")."""
    import torch
    from crypto12381_amd import Context
    dev = torch.device("cuda", 0)
    c = Context(0)                                                                 # its own stream, unknown to torch
    try:
        args, stale, want = _event_case(c, entry, oracle_port)
        ins = [i for i, a in enumerate(args) if isinstance(a, In)]
        outs = [i for i, a in enumerate(args) if isinstance(a, Out)]
        src = {i: torch.frombuffer(bytearray(bytes(args[i])), dtype=torch.uint8).pin_memory() for i in ins}
        d = {i: torch.frombuffer(bytearray(bytes(stale[i])), dtype=torch.uint8).to(dev) for i in ins}
        d.update({i: torch.zeros(int(args[i]), dtype=torch.uint8, device=dev) for i in outs})
        host = {i: torch.zeros(int(args[i]), dtype=torch.uint8).pin_memory() for i in outs}
        torch.cuda.synchronize(dev)
        prod, cons = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        ready, done = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(prod):
            torch.cuda._sleep(400_000_000)                                         # ~0.2 s of spinning in front of the fill
            for i in ins:
                d[i].copy_(src[i], non_blocking=True)
            ready.record(prod)
        c.wait_event(ready.cuda_event)
        rc = getattr(c.lib, "c12381_" + entry.split("[")[0])(c.h, *[_arg(d[i].data_ptr() if i in d else a) for i, a in enumerate(args)])
        assert rc == 0
        done.record(cons)                                                          # creates the handle; re-recorded on the library's stream below
        c.record_event(done.cuda_event)
        with torch.cuda.stream(cons):
            cons.wait_event(done)
            for i in outs:
                host[i].copy_(d[i], non_blocking=True)
        cons.synchronize()                                                         # the first host-side wait
        assert [bytes(host[i].numpy()) for i in outs] == want
        assert c.sync() == 0
        assert c.lib.c12381_wait_event(c.h, None) == E_ARG and c.lib.c12381_record_event(c.h, None) == E_ARG
    finally:
        c.close()


def test_trim_releases_the_workspaces_and_the_next_call_rebuilds_them():
    """c12381_trim (include/c12381_hip.h): workspaces and cached tables go, results stay the same afterwards"""
    import torch
    from crypto12381_amd import Context
    g, gp = golden("g1"), golden("pairing")
    pts, sc = cat(g["points"]), cat(g["scalars"])
    c = Context(0)
    try:
        gen = bytes.fromhex(g["generator"])
        fixed = c.g1_mul_fixed(gen, sc, 49)                                       # builds a cached fixed-base table
        assert c.g1_mul(pts, sc, 49) == cat(g["mul49"])
        k = len(gp["gt_pow_exp"])
        pw = c.gt_op("pow", cat(gp["gt"])[:576 * k], cat(gp["gt_pow_exp"]))
        assert pw == cat(gp["gt_pow"])
        lanes = 1 << 14                                                           # a table slab of 2816 B per lane (c12381_hip.hip, G1_CHUNK): 46 MB
        reps = lanes // (len(sc) // 32) + 1
        big = c.g1_mul((pts * reps)[:96 * lanes], (sc * reps)[:32 * lanes], 49)
        assert big[:len(cat(g["mul49"]))] == cat(g["mul49"])
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info(0)[0]
        c.trim()
        assert torch.cuda.mem_get_info(0)[0] >= free_before + 2816 * lanes       # at least that batch's table slab came back
        assert c.g1_mul_fixed(gen, sc, 49) == fixed
        assert c.g1_mul(pts, sc, 49) == cat(g["mul49"])
        assert c.gt_op("pow", cat(gp["gt"])[:576 * k], cat(gp["gt_pow_exp"])) == pw
        assert c.g1_msm(pts, sc, 49).hex() == g["msm49"]
    finally:
        c.close()


def test_contexts_are_independent(ctx):
    from crypto12381_amd import Context
    g = golden("g1")
    pts, sc = cat(g["points"]), cat(g["scalars"])
    other = Context(0)
    a = ctx.g1_mul(pts, sc, 49)
    b = other.g1_mul(pts, sc, 96)
    assert a == cat(g["mul49"]) and b == cat(g["mul96"])
    other.close()
    assert ctx.g1_mul(pts, sc, 49) == a                                            # closing one does not disturb the other


def test_device_pointer_decompress(ctx):
    import torch
    dev = torch.device("cuda", 0)
    for name, rec_in, rec_out, fn in (("g1", 49, 96, ctx.lib.c12381_g1_decompress_batch_dev), ("g2", 97, 192, ctx.lib.c12381_g2_decompress_batch_dev)):
        g = golden(name)
        comp = cat(g["compressed"])
        n = len(comp) // rec_in
        d_in = torch.frombuffer(bytearray(comp), dtype=torch.uint8).to(dev)
        d_out = torch.empty(rec_out * n, dtype=torch.uint8, device=dev)
        d_st = torch.empty(n, dtype=torch.uint8, device=dev)
        assert fn(ctx.h, n, ctypes.c_void_p(d_in.data_ptr()), ctypes.c_void_p(d_out.data_ptr()), ctypes.c_void_p(d_st.data_ptr())) == 0
        assert ctx.sync() == 0
        assert list(bytes(d_st.cpu().numpy())) == g["decompress_status"]
        assert bytes(d_out.cpu().numpy()) == cat(g["decompressed"])


def test_two_host_threads_two_contexts():
    """One context per host thread (include/c12381_hip.h, "thread-compatible"): two threads drive their own contexts at
    the same time — scalar multiplications and an MSM on one, pairings and Zp inversions on the other (ctypes releases
    the GIL inside the calls) — and every result equals the single-threaded one."""
    import threading
    from crypto12381_amd import Context
    g1g, g2g, gp = golden("g1"), golden("g2"), golden("pairing")
    pts, sc = cat(g1g["points"]), cat(g1g["scalars"])
    n = len(pts) // 96
    reps = 300
    big_pts, big_sc = pts * reps, sc * reps                          # 300 copies: above the bucket-method threshold
    ref = Context(0)
    want_mul = ref.g1_mul(big_pts, big_sc, 49)
    want_msm = ref.g1_msm(big_pts, big_sc, 96)
    p1, q2 = cat(gp["g1"]), cat(gp["g2"])
    want_gt = ref.pair(p1 * 20, q2 * 20)
    x = scalars(91, 5000, 1 << 256)
    want_inv = ref.zp_op("inv", x)
    ref.close()
    errors = []

    def worker_a():
        try:
            c = Context(0)
            for _ in range(3):
                assert c.g1_mul(big_pts, big_sc, 49) == want_mul
                assert c.g1_msm(big_pts, big_sc, 96) == want_msm
            c.close()
        except BaseException as e:                                   # noqa: BLE001 — reported by the main thread
            errors.append(("a", repr(e)))

    def worker_b():
        try:
            c = Context(0)
            for _ in range(3):
                assert c.pair(p1 * 20, q2 * 20) == want_gt
                assert c.zp_op("inv", x) == want_inv
            c.close()
        except BaseException as e:                                   # noqa: BLE001
            errors.append(("b", repr(e)))

    ta, tb = threading.Thread(target=worker_a), threading.Thread(target=worker_b)
    ta.start(); tb.start(); ta.join(); tb.join()
    assert not errors, errors
    assert n > 0


POISON_CODE = r"""
import ctypes, sys
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')
import tools.libsel  # C12381_LIB -> capi.use_library
from util import cat, golden
from crypto12381_amd import Context
from crypto12381_amd.capi import _p, E_INTERNAL
c = Context(0)
g = golden('pairing')
g1, g2 = cat(g['g1']), cat(g['g2'])
n = len(g1) // 96
# pairings: every hand-over of the work queue "times out" (C12381_PAIR_SPIN_LIMIT=-1): status E_INTERNAL, outputs poisoned
out = ctypes.create_string_buffer(576 * n)
rc = c.lib.c12381_pair_batch(c.h, n, _p(g1), _p(g2), _p(out))
assert rc == E_INTERNAL, rc
assert out.raw == b'\xff' * (576 * n), 'outputs of a failed hand-over must be poisoned'
assert b'internal' in c.lib.c12381_last_error(c.h)
# the status is cleared by the read: an operation that does not use the queue succeeds afterwards
gg = golden('g1')
assert c.g1_mul(cat(gg['points']), cat(gg['scalars']), 49) == cat(gg['mul49'])
# boolean form
m = len(g['eq'])
ok = ctypes.create_string_buffer(m)
rc = c.lib.c12381_pair_eq_batch(c.h, m, _p(cat(g['eq_a1'])), _p(cat(g['eq_a2'])), _p(cat(g['eq_b1'])), _p(cat(g['eq_b2'])), _p(ok))
assert rc == E_INTERNAL and ok.raw == b'\xff' * m, (rc, ok.raw)
# one fixed G2 argument
rc = c.lib.c12381_pair_fixed_g2_batch(c.h, n, _p(g1), _p(g2[:192]), _p(out))
assert rc == E_INTERNAL and out.raw == b'\xff' * (576 * n), rc
# the GT power through the queue (five tasks per group)
k = len(g['gt_pow_exp'])
out2 = ctypes.create_string_buffer(576 * k)
rc = c.lib.c12381_gt_op_batch(c.h, 2, k, _p(cat(g['gt'])[:576 * k]), _p(cat(g['gt_pow_exp'])), _p(out2))
assert rc == E_INTERNAL and out2.raw == b'\xff' * (576 * k), rc
c.close()
print('poison ok')
"""


def test_queue_timeout_is_an_internal_error_with_poisoned_outputs():
    """k_pair3.hip queue_wait: a hand-over that times out must not surface as 'invalid point' with plausible bytes.  The
    branch is forced in a child process (negative spin limit = every wait fails; queue forced on for a small batch)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    # the forced time-out exists in the experiments build only (crypto12381_amd/build.py); the product library has no such switch
    e.update({"C12381_PAIR_SPIN_LIMIT": "-1", "C12381_PAIR_QUEUE": "1", "C12381_LIB": os.path.join(root, "crypto12381_amd", "lib", "libc12381_hip_exp.so")})
    r = subprocess.run([sys.executable, "-c", POISON_CODE], env=e, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
