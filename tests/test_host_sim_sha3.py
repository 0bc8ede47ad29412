"""CPU tests of the device SHA3-512 (crypto12381_amd/csrc/sha3.hpp) compiled for the host with the bounds checker (tests/host_sim/sha3.cpp,
C12381_CHECK_BOUNDS): its digests equal the compiled reference's (hash_state -> MIRACL SHA3, tests/golden/sha3_512.json, recorded by
tools/gen_sha3_golden.py) and hashlib's FIPS 202 SHA3-512 for every length from 0 to 600 bytes, at every misalignment of a batch."""
import ctypes
import hashlib
import os
import subprocess

import pytest

from util import golden, prng

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "host_sim")
CSRC = os.path.join(os.path.dirname(HERE), "crypto12381_amd", "csrc")
sz = ctypes.c_size_t


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(SIM_DIR, "libsim_sha3.so")
    src = os.path.join(SIM_DIR, "sha3.cpp")
    srcs = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-DC12381_CHECK_BOUNDS", "-fPIC", "-shared", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def sim_sha3(sim, msgs: bytes, n: int, length: int) -> bytes:
    # 8 bytes of slack: full blocks are read in aligned words, up to 3 bytes past the last message (sha3.hpp)
    buf = ctypes.create_string_buffer(msgs + bytes(8), len(msgs) + 8)
    out = ctypes.create_string_buffer(max(64 * n, 1))
    assert sim.sim_sha3_512(sz(n), sz(length), buf, out) == 0
    return out.raw[:64 * n]


def test_fixture_is_fips202():
    """MIRACL's SHA3 as the reference drives it is FIPS 202 SHA3-512 at every recorded length (the reference's own unit test checks the empty
    string only)"""
    g = golden("sha3_512")
    assert [len(bytes.fromhex(m)) for m in g["msgs"]] == g["lengths"]
    for m, d in zip(g["msgs"], g["digests"]):
        assert hashlib.sha3_512(bytes.fromhex(m)).hexdigest() == d


def test_fixture_lengths(sim):
    g = golden("sha3_512")
    for m, d in zip(g["msgs"], g["digests"]):
        msg = bytes.fromhex(m)
        assert sim_sha3(sim, msg, 1, len(msg)).hex() == d, len(msg)
        # three copies: the second and third start misaligned unless the length is a multiple of 4
        assert sim_sha3(sim, msg * 3, 3, len(msg)) == bytes.fromhex(d) * 3, len(msg)


def test_every_length_to_600(sim):
    for length in range(601):
        n = 5
        msgs = b"".join(prng(31, 1000 * length + j, 640).to_bytes(640, "big")[:length] for j in range(n))
        got = sim_sha3(sim, msgs, n, length)
        want = b"".join(hashlib.sha3_512(msgs[length * j:length * j + length]).digest() for j in range(n))
        assert got == want, length


def test_digest_words_feed_zp_from_hash(sim):
    """the words handed to fr_from_digest_words are the digest as a big-endian integer (Zp from_hash, zp_number.hpp:540-548)"""
    msg = b"bbs04 transcript"
    w = (ctypes.c_uint32 * 16)()
    buf = ctypes.create_string_buffer(msg + bytes(8), len(msg) + 8)
    assert sim.sim_sha3_512_words(sz(len(msg)), buf, w) == 0
    assert b"".join(int(x).to_bytes(4, "big") for x in w) == hashlib.sha3_512(msg).digest()
