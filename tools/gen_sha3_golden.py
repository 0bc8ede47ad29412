"""Record tests/golden/sha3_512.json: SHA3-512 digests computed by the compiled reference (hash_state's miracl_core::sha3_*, through
oracle/ref_wrap.cpp ref_sha3_512) for deterministic messages whose lengths straddle the 72-byte rate of SHA3-512.

    python tools/gen_sha3_golden.py          (needs oracle/_ref, built by `make -C oracle` where the reference's sources are)"""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = [0, 1, 71, 72, 73, 135, 136, 143, 144, 145, 575, 576, 577, 919, 1000, 1500]


def message(length: int) -> bytes:
    out = b""
    ctr = 0
    while len(out) < length:
        out += hashlib.sha256(b"c12381 sha3|%d|%d" % (length, ctr)).digest()
        ctr += 1
    return out[:length]


def main() -> None:
    from oracle.bindings import Oracle
    lib = Oracle("reference").lib
    lib.ref_sha3_512.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    msgs, digests = [], []
    for length in LENGTHS:
        m = message(length)
        out = ctypes.create_string_buffer(64)
        assert lib.ref_sha3_512(m, length, out) == 0
        msgs.append(m.hex())
        digests.append(out.raw[:64].hex())
    path = os.path.join(ROOT, "tests", "golden", "sha3_512.json")
    with open(path, "w") as f:
        json.dump({"source": "reference hash_state: miracl_core::sha3_init(64) / sha3_process / sha3_hash (oracle/ref_wrap.cpp ref_sha3_512)",
                   "lengths": LENGTHS, "msgs": msgs, "digests": digests}, f, indent=1)
        f.write("\n")
    print("wrote %s (%d digests)" % (path, len(digests)))


if __name__ == "__main__":
    main()
