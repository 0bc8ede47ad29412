"""c12381_ac_rbbs_pres_batch: AC-rbbs presentations (the reference's examples/AC-rbbs/src/pres.cpp) from the wire formats with the caller's
randomness: every output byte equals pres composed from the CPU oracle's primitives and hashlib (tests/ac_rbbs_cases.py expected_pres).  Lanes:
honest credentials, randomness at 0, r and 2^256 - 1, A and cache points at infinity, w = 0, cache points outside G1 (order 3, eigenpoint), A or a
cache point that does not decode and w >= r (0xff records, the other lanes unaffected); message lengths 0, 32, 42, 43; one tiled run of 2^12 + 1
lanes in host and _dev form and a second chunk."""
import pytest

import ac_rbbs_cases as rc
from g1_torsion import eigenpoint, enc as enc96, point_of_order
from util import R, prng

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    from crypto12381_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def op(oracle_port):
    return rc.Ops(oracle_port)


def rnd96(vals):
    return b"".join(v.to_bytes(32, "big") for v in vals)


def lanes_of(op, msg_len=rc.MSG_LEN):
    """(sig, cache, msg, rnd) per lane"""
    key = rc.Key(op, 5000, rc.NATTR)
    creds = [rc.Cred(op, key, rc.I_MAIN, 6100, i, msg_len) for i in range(4)]
    out = [(c.sig, c.cache, c.msg, rnd96(c.rnd)) for c in creds]
    c = creds[0]
    for vals in ([0, 5, 7], [R, R + 1, (1 << 256) - 1], [(1 << 256) - 1, 0, 0], [1, R - 1, R - 1], [R - 1, 0, 1]):
        out.append((c.sig, c.cache, c.msg, rnd96(vals)))
    out.append((bytes(49) + c.sig[49:], c.cache, c.msg, rnd96(c.rnd)))                      # A at infinity
    out.append((c.sig[:49] + bytes(48), c.cache, c.msg, rnd96(c.rnd)))                      # w = 0
    out.append((c.sig[:49] + rc.b48(R - 1), bytes(196), c.msg, rnd96(c.rnd)))                # every cache point at infinity
    t3, te = enc96(point_of_order(3)), enc96(eigenpoint(10177)[0])
    pts = [op.dec(c.cache[49 * k:49 * k + 49])[0] for k in range(4)]
    for k in range(4):                                                                      # off the subgroup
        off = list(pts)
        off[k] = op.add(pts[k], t3 if k % 2 == 0 else te)
        out.append((c.sig, b"".join(op.enc(p) for p in off), c.msg, rnd96(c.rnd)))
    out.append((op.enc(op.add(op.dec(c.sig[:49])[0], t3)) + c.sig[49:], c.cache, c.msg, rnd96(c.rnd)))
    # where the reference would throw
    out.append((b"\x05" + c.sig[1:], c.cache, c.msg, rnd96(c.rnd)))
    out.append((rc.off_curve_x() + c.sig[49:], c.cache, c.msg, rnd96(c.rnd)))
    for k in range(4):
        out.append((c.sig, c.cache[:49 * k] + rc.off_curve_x() + c.cache[49 * k + 49:], c.msg, rnd96(c.rnd)))
    out.append((c.sig[:49] + rc.b48(R), c.cache, c.msg, rnd96(c.rnd)))
    out.append((c.sig[:49] + rc.b48((1 << 384) - 1), c.cache, c.msg, rnd96(c.rnd)))
    out.append(out[1])                                                                      # a good lane behind the refused ones
    return out


def expected(op, lanes):
    res = [rc.expected_pres(op, *ln) for ln in lanes]
    return b"".join(p for p, _ in res), bytes(s for _, s in res)


def call(ctx, lanes, msg_len):
    return ctx.ac_rbbs_pres(*(b"".join(ln[k] for ln in lanes) for k in range(4)), msg_len)


@pytest.fixture(scope="module")
def main(op):
    lanes = lanes_of(op)
    return lanes, expected(op, lanes)


def test_bytes_equal_the_builders(ctx, main):
    lanes, (want_p, want_s) = main
    got_p, got_s = call(ctx, lanes, rc.MSG_LEN)
    assert got_s == want_s
    bad = [j for j in range(len(lanes)) if got_p[341 * j:341 * j + 341] != want_p[341 * j:341 * j + 341]]
    assert not bad, bad
    assert want_s == bytes(17) + b"\xff" * 8 + bytes(1)


@pytest.mark.parametrize("msg_len", [0, 42, 43])
def test_message_lengths(ctx, op, msg_len):
    key = rc.Key(op, 5000, rc.NATTR)
    creds = [rc.Cred(op, key, rc.I_MAIN, 6200, i, msg_len) for i in range(3)]
    lanes = [(c.sig, c.cache, c.msg, rnd96([prng(6300 + msg_len, 3 * i + k, 32) for k in range(3)])) for i, c in enumerate(creds)]
    assert call(ctx, lanes, msg_len) == expected(op, lanes)


def test_large_tiled_host_and_dev_and_second_chunk(ctx, main):
    import torch
    lanes, (want_p, want_s) = main
    m = len(lanes)
    for n in ((1 << 12) + 1, (1 << 18) + 3):
        idx = [(j * 37) % m for j in range(n)] if n < (1 << 18) else [j % m for j in range(n)]
        ins = [b"".join(lanes[i][k] for i in idx) for k in range(4)]
        want = b"".join(want_p[341 * i:341 * i + 341] for i in idx), bytes(want_s[i] for i in idx)
        assert ctx.ac_rbbs_pres(*ins, rc.MSG_LEN) == want
        if n > (1 << 12) + 1:
            continue
        d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda") for b in ins]
        d_p = torch.full((341 * n,), 7, dtype=torch.uint8, device="cuda")
        d_s = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.ac_rbbs_pres_dev(n, rc.MSG_LEN, *(t.data_ptr() for t in d), d_p.data_ptr(), d_s.data_ptr())
        assert ctx.sync() == 0
        assert (bytes(d_p.cpu().numpy().tobytes()), bytes(d_s.cpu().numpy().tobytes())) == want
