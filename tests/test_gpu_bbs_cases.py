"""GPU test of the BBS+ entries on the labelled lanes of tests/bbs_cases.py (tests/test_bbs_cases.py checks the labels on the CPU): the batch
entry — which evaluates e(A, w) e(x A - B, g2) == 1 where the reference writes e(A, w + x g2) == e(B, g2) — with A, B, w + x g2 and x A - B at
infinity, colliding columns in the per-lane sum, scalars at and above r, every lane at the ends of a 21-pairing group, of a wavefront and of the
batch, keys outside G2 (the generic route), the _dev form, the wire entry at its parser's boundaries, signing and the aggregate verdict on
degenerate-but-accepted lanes, and the routes the experiments library selects.  Every comparison is byte equality with the CPU oracle."""
import json
import os
import subprocess
import sys

import pytest

import bbs_cases as bc
from util import R, prng

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(v, k) for v in bc.VARIANTS for k in bc.NMSGS if bc.applicable(v, k)]
OFF_CURVE = "A not on the curve"
DEGENERATE = ("A inf, B inf", "x = -gamma, B inf", "x = 2R - gamma, B inf", "x = gamma", "r = 0, m = 0", "sum = g1", "r h0 = m_1 h_1",
              "r h0 = -m_1 h_1", "m_1 h_1 = -m_last h_last")


@pytest.fixture(scope="module")
def ctx():
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(oracle_port):
    """(params, lanes, the oracle's verdicts) per (variant, nmsg), evaluated once"""
    memo = {}

    def get(variant, nmsg):
        if (variant, nmsg) not in memo:
            p = bc.Params(oracle_port, 9100, nmsg, variant)
            ls = bc.lanes(p)
            memo[variant, nmsg] = (p, ls, bc.expect(p, ls))
        return memo[variant, nmsg]
    return get


def verify(ctx, p, ls, order=None, strict=False):
    return ctx.bbs_plus_verify(*p.public(), *bc.pack(ls, order), strict=strict)


@pytest.mark.parametrize("variant,nmsg", CASES)
def test_verify_every_lane(ctx, case, variant, nmsg):
    from crypto12381_amd.capi import C12381Error, E_POINT
    p, ls, want = case(variant, nmsg)
    assert want == bc.tags(ls)
    assert verify(ctx, p, ls) == want
    with pytest.raises(C12381Error) as e:                                   # the list holds the lane whose A is not on the curve
        verify(ctx, p, ls, strict=True)
    assert e.value.code == E_POINT
    rest = [j for j, ln in enumerate(ls) if ln.kind != OFF_CURVE]
    assert len(rest) == len(ls) - 1
    assert verify(ctx, p, ls, rest, strict=True) == bytes(want[j] for j in rest)


@pytest.fixture(scope="module")
def placed(case):
    """the main list of (standard, 4) padded with honest signatures to 85 lanes"""
    p, ls, want = case("standard", 4)
    more = bc.valid_lanes(p, 85 - len(ls), 9300)
    assert bc.expect(p, more) == b"\x01" * len(more)
    return p, ls + more, want + b"\x01" * len(more)


@pytest.mark.parametrize("pos", [0, 20, 21, 62, 63, 84])
def test_verify_lane_placement(ctx, placed, pos):
    """each accepted degenerate lane and the off-curve lane at the ends of a group of 21 pairings, of a wavefront and of the batch"""
    p, ls, want = placed
    n = len(ls)
    for kind in DEGENERATE + (OFF_CURVE,):
        i = [ln.kind for ln in ls].index(kind)
        order = [(i - pos + j) % n for j in range(n)]
        assert order[pos] == i
        assert verify(ctx, p, ls, order) == bytes(want[k] for k in order), kind


@pytest.mark.parametrize("n", [1, 21, 22, 63, 64, 65])
def test_verify_prefixes(ctx, placed, n):
    p, ls, want = placed
    for first in ("A inf, B inf", "valid"):
        i = [ln.kind for ln in ls].index(first)
        order = [(i + j) % len(ls) for j in range(n)]
        assert verify(ctx, p, ls, order) == bytes(want[k] for k in order), first


@pytest.mark.parametrize("variant", bc.OFF_G2_VARIANTS)
@pytest.mark.parametrize("nmsg", [1, 4, 5])
def test_verify_generic_route(ctx, oracle_port, variant, nmsg):
    """a key outside G2: the equation is evaluated as written (g2_mul + g2_add, two Miller loops per lane)"""
    p = bc.Params(oracle_port, 9100, nmsg, variant)
    ls = bc.lanes(p)
    want = bc.expect(p, ls)
    assert {0, 1, 0xff} == set(want)
    by = {ln.kind: b for ln, b in zip(ls, want)}
    assert by["A inf, B inf"] == 1
    assert verify(ctx, p, ls) == want


def test_verify_dev_form(ctx, case):
    """the _dev form on device buffers writes every byte of its output and equals the host form"""
    import torch
    from crypto12381_amd.capi import E_POINT
    p, ls, want = case("standard", 4)
    n = len(ls)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    d = [dev(b) for b in p.public() + bc.pack(ls)]
    for preset in (0x5a, 0x01):
        d_ok = torch.full((n,), preset, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.bbs_plus_verify_dev(n, 4, *(t.data_ptr() for t in d), d_ok.data_ptr())
        assert ctx.sync() == E_POINT                                        # the off-curve lane, reported once
        assert ctx.sync() == 0
        assert bytes(d_ok.cpu().numpy().tobytes()) == want == verify(ctx, p, ls)


# ---------------------------------------------------------------- the wire entry
def wire_params(orc, msg_len, setting, spare):
    nblk = (msg_len + 30) // 31
    variant = setting if setting in bc.VARIANTS else "standard"
    nh = nblk + (1 if spare else 0)
    if not bc.applicable(variant, nh):
        return None
    return bc.Params(orc, 9200 + msg_len, nh, variant)


@pytest.mark.parametrize("msg_len", [0, 1, 30, 31, 32, 62, 63])
def test_wire_every_lane(ctx, oracle_port, msg_len):
    """nh == nblk and nh == nblk + 1; a spare h entry that does not decode; a used h entry at infinity; the public key at infinity"""
    from oracle.bindings import Oracle, have_reference
    checkers = [oracle_port] + ([Oracle("reference")] if have_reference() else [])
    ran = 0
    for setting, spare in (("standard", False), ("standard", True), ("spare entry undecodable", True), ("h_k at infinity", False),
                           ("h_k at infinity", True), ("w at infinity", False), ("w at infinity", True)):
        p = wire_params(oracle_port, msg_len, setting, spare)
        if p is None:
            continue
        tag = 5 if setting == "spare entry undecodable" else None
        wl = bc.wire_lanes(p, msg_len)
        want = bc.tags(wl)
        for ck in checkers:
            assert bc.wire_expect(p, wl, msg_len, ck, tag) == want, (setting, ck.kind)
        assert ctx.bbs_plus_verify_wire(*bc.wire_public(p, tag), *bc.wire_pack(wl), msg_len) == want, (setting, spare)
        ran += 1
    assert ran >= 5


@pytest.mark.parametrize("msg_len", [1, 31, 32, 63])
def test_wire_used_h_entry_undecodable(ctx, oracle_port, msg_len):
    """tag 05 on an h entry in use: the reference throws before it looks at a signature"""
    from crypto12381_amd.capi import C12381Error, E_POINT
    p = wire_params(oracle_port, msg_len, "standard", False)
    wl = bc.wire_lanes(p, msg_len)
    pub = bc.wire_public(p, 5)
    with pytest.raises(RuntimeError):
        oracle_port.bbs_plus_verify_wire(*pub, *bc.wire_pack(wl), msg_len, 1)
    assert ctx.bbs_plus_verify_wire(*pub, *bc.wire_pack(wl), msg_len, strict=False) == b"\xff" * len(wl)
    with pytest.raises(C12381Error) as e:
        ctx.bbs_plus_verify_wire(*pub, *bc.wire_pack(wl), msg_len)
    assert e.value.code == E_POINT
    assert ctx.bbs_plus_verify_wire(*bc.wire_public(p), *bc.wire_pack(wl), msg_len) == bc.tags(wl)      # the context recovers


# ---------------------------------------------------------------- signing
@pytest.mark.parametrize("variant,nmsg", [(v, k) for v in ("standard", "h_k at infinity", "h0 == h_1", "g1 at infinity") for k in (0, 1, 4, 5)
                                          if bc.applicable(v, k)])
def test_sign_every_lane(ctx, case, variant, nmsg):
    """sign() on the (x, r, m) of every lane of the main list: gamma + x = 0 (reduced and not), B at infinity, r = 0 with m = 0, the column
    collisions, x = gamma; with gamma as it is and as gamma + R"""
    p, ls, _ = case(variant, nmsg)
    _, X, Rr, Mm = bc.pack(ls)
    want = bc.sign_expect(p, ls)
    by = {ln.kind: want[96 * j:96 * j + 96] for j, ln in enumerate(ls)}
    assert by["x = -gamma, B != inf"] == bytes(96) and by["x = 2R - gamma, B inf"] == bytes(96) and by["A inf, B inf"] == bytes(96)
    for gamma in (p.gamma, p.gamma + R):
        assert ctx.bbs_plus_sign(p.g1, p.h0, p.h, bc.b32(gamma), X, Rr, Mm) == want
    ok = ctx.bbs_plus_verify(*p.public(), want, X, Rr, Mm)
    assert ok == p.orc.bbs_plus_verify(*p.public(), want, X, Rr, Mm, 8)
    for j, ln in enumerate(ls):
        if want[96 * j:96 * j + 96] != bytes(96):
            assert ok[j] == 1, ln.kind


# ---------------------------------------------------------------- the aggregate verdict
def rho128(seed, n):
    return [prng(seed, j) % ((1 << 128) - 1) + 1 for j in range(n)]


def aggregate(ctx, p, ls, rho):
    return ctx.bbs_plus_verify_aggregate(*p.public(), *bc.pack(ls), b"".join(bc.b32(v) for v in rho))


def test_aggregate_accepts_every_accepted_lane(ctx, case):
    p, ls, _ = case("standard", 4)
    acc = [ln for ln in ls if ln.tag == bc.ACCEPT]
    n = len(acc)
    assert n >= 12 and set(DEGENERATE) <= {ln.kind for ln in acc}
    assert aggregate(ctx, p, acc, rho128(9400, n)) is True
    full = [prng(9401, j) % R for j in range(n)]
    assert aggregate(ctx, p, acc, [0, R, R + 5] + full[3:]) is True
    assert aggregate(ctx, p, acc, full[:-1] + [(R - sum(full[:-1]) % R) % R]) is True       # the coefficients sum to 0: g1 drops out
    assert aggregate(ctx, p, acc, [full[0], R - full[0]] + full[2:-1] + [(R - sum(full[2:-1]) % R) % R]) is True


def test_aggregate_follows_every_rejected_lane(ctx, case):
    """one rejected lane among twelve accepted ones: False with a non-zero coefficient, True with 0 or R — coefficients are reduced before use"""
    p, ls, _ = case("standard", 4)
    acc = [ln for ln in ls if ln.tag == bc.ACCEPT][:12]
    rej = [ln for ln in ls if ln.tag == bc.REJECT]
    assert len(rej) >= 12
    for i, ln in enumerate(rej):
        at = i % 13
        batch = acc[:at] + [ln] + acc[at:]
        rho = rho128(9410 + i, 13)
        assert aggregate(ctx, p, batch, rho) is False, ln.kind
        for zero in (0, R):
            assert aggregate(ctx, p, batch, rho[:at] + [zero] + rho[at + 1:]) is True, (ln.kind, zero)
    assert aggregate(ctx, p, acc[4:5], rho128(9440, 1)) is True             # n = 1
    assert aggregate(ctx, p, rej[:1], rho128(9441, 1)) is False


def test_aggregate_off_curve_signature(ctx, case):
    """include/c12381_hip.h: C12381_E_POINT is the code for an input point that is not on the curve, and *all_ok = 0 for an invalid signature:
    the call returns that code, writes 0 over the caller's value and leaves the context usable"""
    import ctypes
    from crypto12381_amd.capi import C12381Error, E_POINT, _p
    p, ls, _ = case("standard", 4)
    acc = [ln for ln in ls if ln.tag == bc.ACCEPT][:12]
    bad = [ln for ln in ls if ln.kind == OFF_CURVE]
    for at in (0, 5, 12):
        batch = acc[:at] + bad + acc[at:]
        with pytest.raises(C12381Error) as e:
            aggregate(ctx, p, batch, rho128(9450, 13))
        assert e.value.code == E_POINT
        args = p.public() + bc.pack(batch) + (b"".join(bc.b32(v) for v in rho128(9450, 13)),)
        all_ok = ctypes.c_int(1)
        rc = ctx.lib.c12381_bbs_plus_verify_aggregate(ctx.h, 13, 4, *(_p(b) for b in args), ctypes.byref(all_ok))
        assert rc == E_POINT and all_ok.value == 0
        assert aggregate(ctx, p, acc, rho128(9451, 12)) is True


# ---------------------------------------------------------------- the routes of the experiments library
EXP_LIB = os.path.join(ROOT, "crypto12381_amd", "lib", "libc12381_hip_exp.so")
CHILD = r"""
import json, sys
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')
import tools.libsel  # C12381_LIB -> capi.use_library
from crypto12381_amd import Context
d = {k: bytes.fromhex(v) if isinstance(v, str) else v for k, v in json.load(open(sys.argv[1])).items()}
c = Context(0)
got = c.bbs_plus_verify(d['g1'], d['g2'], d['h0'], d['h'], d['w'], d['A'], d['x'], d['r'], d['m'], strict=False)
assert got == d['verify'], ('verify', got.hex(), d['verify'].hex())
got = c.bbs_plus_verify_wire(d['pp'], d['h49'], d['pk'], d['sigs'], d['msgs'], d['msg_len'])
assert got == d['wire'], ('wire', got.hex(), d['wire'].hex())
got = c.bbs_plus_sign(d['g1'], d['h0'], d['h'], d['gamma'], d['x'], d['r'], d['m'])
assert got == d['sign'], 'sign'
c.close()
print('bbs ok')
"""


@pytest.fixture(scope="module")
def child_inputs(case, oracle_port, tmp_path_factory):
    p, ls, want = case("standard", 4)
    A, X, Rr, Mm = bc.pack(ls)
    pw = bc.Params(oracle_port, 9200 + 32, 3, "standard")
    wl = bc.wire_lanes(pw, 32)
    pp, h49, pk = bc.wire_public(pw)
    sigs, msgs = bc.wire_pack(wl)
    d = dict(g1=p.g1, g2=p.g2, h0=p.h0, h=p.h, w=p.w, A=A, x=X, r=Rr, m=Mm, verify=want, gamma=bc.b32(p.gamma), sign=bc.sign_expect(p, ls),
             pp=pp, h49=h49, pk=pk, sigs=sigs, msgs=msgs, wire=bc.wire_expect(pw, wl, 32))
    assert d["wire"] == bc.tags(wl)
    path = tmp_path_factory.mktemp("bbs_cases") / "inputs.json"
    with open(path, "w") as f:
        json.dump(dict({k: v.hex() for k, v in d.items()}, msg_len=32), f)
    return str(path)


@pytest.mark.parametrize("env", [{"C12381_FIXED_BASE": "0"}, {"C12381_PAIR_LANES": "1"}, {"C12381_PAIR_QUEUE": "0"}, {"C12381_PAIR_QUEUE": "1"},
                                 {"C12381_G2_LANES": "1"}],
                         ids=["fixed-base-off", "one-lane-pairing", "pair-queue-off", "pair-queue-on", "g2-one-lane"])
def test_experiments_library_routes(child_inputs, env):
    """verify, the wire entry and sign through g2_mul + g2_add (fixed base off), the G2 table with w as addend (one-lane pairing), the queue on and
    off and the one-lane G2 kernel: x = +-gamma reaches the doubling and the cancellation of w + x g2 there"""
    e = dict(os.environ)
    for k in [k for k in e if k.startswith("C12381_")]:
        del e[k]
    e["C12381_LIB"] = EXP_LIB
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD, child_inputs], env=e, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "bbs ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
