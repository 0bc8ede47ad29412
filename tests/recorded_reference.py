"""The compiled reference's answers, stored: where oracle/_ref/libc12381_ref.so cannot be built (its sources are not part of this
repository) the `oracle_ref` fixture replays, for exactly the calls this suite makes, what the compiled reference returned when the
calls were recorded (tests/golden/reference_calls.bin).  A call is looked up by its method and the exact bytes of its arguments: a call
that was not recorded — new inputs, or an input that came out of a GPU kernel and differs from the recorded run's — raises instead of
answering.

Recording (where oracle/_ref exists, on the GPU box for the -m gpu tests): C12381_RECORD_REFERENCE=<file> python -m pytest tests ...
writes the calls of that run to <file>, merged with what <file> already holds (point several runs at one file, or merge files with
`python tests/recorded_reference.py OUT IN...`)."""
from __future__ import annotations

import gzip
import hashlib
import inspect
import os
import struct
import sys

STORE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_calls.bin")
MAGIC = b"c12381 recorded reference calls v1\n"


def _signature(name):
    from oracle.bindings import Oracle
    fn = getattr(Oracle, name, None)
    if name.startswith("_") or not callable(fn):
        raise AttributeError(name)
    return inspect.signature(fn)


def call_key(name, args, kwargs) -> bytes:
    """sha256 over the method name and every argument after binding (defaults applied, so positional and keyword forms agree)"""
    bound = _signature(name).bind(None, *args, **kwargs)
    bound.apply_defaults()
    h = hashlib.sha256(name.encode() + b"\0")
    for pname, v in list(bound.arguments.items())[1:]:
        h.update(pname.encode() + b"=")
        if isinstance(v, (bytes, bytearray, memoryview)):
            v = bytes(v)
            h.update(b"b%d:" % len(v) + v)
        elif isinstance(v, bool) or v is None or isinstance(v, (int, str)):
            h.update(b"v" + repr(v).encode())
        else:
            raise TypeError("%s: argument %s of type %s cannot be keyed" % (name, pname, type(v).__name__))
        h.update(b"\0")
    return h.digest()


def _enc(v) -> bytes:
    if isinstance(v, (bytes, bytearray)):
        return b"B" + struct.pack("<I", len(v)) + bytes(v)
    if isinstance(v, tuple):
        return b"T" + struct.pack("<B", len(v)) + b"".join(_enc(x) for x in v)
    raise TypeError("cannot store a result of type %s" % type(v).__name__)


def _dec(buf, i):
    tag = buf[i:i + 1]
    if tag == b"B":
        (n,) = struct.unpack_from("<I", buf, i + 1)
        return bytes(buf[i + 5:i + 5 + n]), i + 5 + n
    if tag == b"T":
        out, i = [], i + 2
        for _ in range(buf[i - 1]):
            v, i = _dec(buf, i)
            out.append(v)
        return tuple(out), i
    raise ValueError("corrupt record at byte %d" % i)


def load(path=STORE) -> dict:
    with gzip.open(path, "rb") as f:
        buf = f.read()
    if not buf.startswith(MAGIC):
        raise ValueError("%s: not a recorded-reference file" % path)
    rec, i = {}, len(MAGIC)
    while i < len(buf):
        key = bytes(buf[i:i + 32])
        rec[key], i = _dec(buf, i + 32)
    return rec


def save(rec: dict, path=STORE) -> None:
    body = b"".join(k + _enc(rec[k]) for k in sorted(rec))
    with gzip.GzipFile(path, "wb", mtime=0) as f:                     # mtime 0: the same records give the same file
        f.write(MAGIC + body)


class RecordingReference:
    """the compiled reference, with every public call's result kept for save()"""

    def __init__(self, ref):
        self._ref, self._rec = ref, {}

    def __getattr__(self, name):
        attr = getattr(self._ref, name)
        if name.startswith("_") or not callable(attr):
            return attr

        def call(*args, **kwargs):
            out = attr(*args, **kwargs)
            self._rec[call_key(name, args, kwargs)] = out
            return out
        return call

    def save(self, path) -> None:
        rec = load(path) if os.path.exists(path) else {}
        rec.update(self._rec)
        save(rec, path)


class RecordedReference:
    """the stored answers of the compiled reference; an unrecorded call is an error, never a substitute"""
    kind = "reference (recorded)"

    def __init__(self, path=STORE):
        self._path, self._rec = path, load(path)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        _signature(name)

        def call(*args, **kwargs):
            key = call_key(name, args, kwargs)
            if key not in self._rec:
                raise LookupError("%s(...): no recorded reference result for these arguments (%s) — either an input differs from the "
                                  "recorded run's or the call is new: re-record where oracle/_ref exists (C12381_RECORD_REFERENCE)"
                                  % (name, os.path.relpath(self._path)))
            return self._rec[key]
        return call


if __name__ == "__main__":
    # merge: python tests/recorded_reference.py OUT IN [IN ...]
    merged = {}
    for p in sys.argv[2:]:
        merged.update(load(p))
    save(merged, sys.argv[1])
    print("%s: %d calls" % (sys.argv[1], len(merged)))
