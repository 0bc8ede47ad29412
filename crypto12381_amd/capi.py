"""ctypes binding of the C ABI in include/c12381_hip.h.

This module is plumbing: it loads the in-tree HIP library and moves bytes.  There is NO CPU
fallback — if the library is missing or no HIP device is usable, construction fails loudly.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libc12381_hip.so")
# The binding reads NO environment variable.  Tools, A/B runs and the variant tests that need another build of the same ABI (the
# experiments library, tools/build_variant.sh outputs) say so explicitly with use_library(path) before the first Context — see
# tools/libsel.py, which is where their C12381_LIB convention lives now.

E_ARG, E_HIP, E_POINT, E_NOMEM, E_INTERNAL = -1, -2, -3, -4, -5
F_IN_SUBGROUP = 1
F_MILLER_ONLY = 2
F_COMPRESSED_IN = 4
PS_MSG_HASH, PS_MSG_ENCODE = 0, 1


class C12381Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"c12381 error {code}: {msg}")
        self.code = code


_lib = None
_lib_path = LIB_PATH


def use_library(path: str) -> None:
    """Select another build of the same C ABI (experiments / A-B library) for this process; must precede the first load."""
    global _lib_path
    if _lib is not None and os.path.abspath(path) != os.path.abspath(_lib_path):
        raise RuntimeError("use_library(%s): %s is already loaded in this process" % (path, _lib_path))
    _lib_path = path


def load_library() -> ctypes.CDLL:
    """Load libc12381_hip.so (built by crypto12381_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_lib_path):
            raise FileNotFoundError(
                f"{_lib_path} not found: the HIP extension is not built (run `python -m crypto12381_amd.build`). "
                "There is no CPU fallback.")
        lib = ctypes.CDLL(_lib_path)
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        lib.c12381_create.argtypes = [ci, ctypes.POINTER(vp)]
        lib.c12381_destroy.argtypes = [vp]
        lib.c12381_destroy.restype = None
        lib.c12381_last_error.argtypes = [vp]
        lib.c12381_last_error.restype = ctypes.c_char_p
        lib.c12381_set_stream.argtypes = [vp, vp]
        lib.c12381_sync.argtypes = [vp]
        lib.c12381_wait_event.argtypes = [vp, vp]
        lib.c12381_record_event.argtypes = [vp, vp]
        lib.c12381_trim.argtypes = [vp]
        lib.c12381_profile.argtypes = [vp, ci]
        lib.c12381_profile_read.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]
        for name in ("c12381_fp_op_batch", "c12381_fp_op_batch_dev"):
            getattr(lib, name).argtypes = [vp, ci, sz, vp, vp, vp]
        lib.c12381_fp_mulchain_dev.argtypes = [vp, sz, ci, vp, vp, vp]
        for name in ("c12381_g1_mul_batch", "c12381_g1_mul_batch_dev", "c12381_g1_add_batch", "c12381_g1_msm",
                     "c12381_g1_msm_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp, ci]
        for name in ("c12381_g2_mul_batch", "c12381_g2_mul_batch_dev", "c12381_g2_add_batch"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp, ci]
        for name in ("c12381_g1_sum", "c12381_g1_sum_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, ci]
        for name in ("c12381_g1_sum_of_products", "c12381_g1_sum_of_products_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp, ci]
        for name in ("c12381_g2_msm", "c12381_g2_msm_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp, ci]
        for name in ("c12381_g1_mul_batch_flags", "c12381_g1_mul_batch_flags_dev", "c12381_g2_mul_batch_flags", "c12381_g2_mul_batch_flags_dev",
                     "c12381_g1_msm_flags", "c12381_g1_msm_flags_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp, ci, ctypes.c_uint]
        for name in ("c12381_g1_mul_sum_batch", "c12381_g1_mul_sum_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, ci, vp, vp, vp, ci, ctypes.c_uint]
        for name in ("c12381_pair_batch_flags", "c12381_pair_batch_flags_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp, ctypes.c_uint]
        for name in ("c12381_pair_batch", "c12381_pair_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp]
        for name in ("c12381_pair_product_batch", "c12381_pair_product_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, ci, vp, vp, vp, ctypes.c_uint]
        for name in ("c12381_pair_eq_batch", "c12381_pair_eq_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp, vp, vp]
        for name in ("c12381_g1_decompress_batch", "c12381_g2_decompress_batch"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp]
        for name in ("c12381_miller_batch", "c12381_miller_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp]
        for name in ("c12381_fexp_batch", "c12381_fexp_batch_dev", "c12381_gt_is_unity_batch", "c12381_gt_is_unity_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp]
        for name in ("c12381_gt_op_batch", "c12381_gt_op_batch_dev"):
            getattr(lib, name).argtypes = [vp, ci, sz, vp, vp, vp]
        for name in ("c12381_g1_from_hash_batch", "c12381_g1_from_hash_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, ci]
        for name in ("c12381_g1_mul_fixed_batch", "c12381_g1_mul_fixed_batch_dev", "c12381_g2_mul_fixed_batch", "c12381_g2_mul_fixed_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp, ci]
        for name in ("c12381_g1_mul_fixed_sum_batch", "c12381_g1_mul_fixed_sum_batch_dev", "c12381_g2_mul_fixed_sum_batch",
                     "c12381_g2_mul_fixed_sum_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, vp, vp, vp, vp, ci]
        for name in ("c12381_pair_fixed_g2_batch", "c12381_pair_fixed_g2_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp]
        for name in ("c12381_pair_product_fixed_g2_batch", "c12381_pair_product_fixed_g2_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, ci, vp, vp, vp, ctypes.c_uint]
        for name in ("c12381_ps_verify_batch", "c12381_ps_verify_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz] + [vp] * 7
        for name in ("c12381_bbs_plus_sign_batch", "c12381_bbs_plus_sign_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp]
        for name in ("c12381_g1_decompress_batch_dev", "c12381_g2_decompress_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp]
        lib.c12381_g1_msm_multi.argtypes = [ctypes.POINTER(vp), ci, sz, vp, vp, vp, ci]
        lib.c12381_g1_map_to_point_batch.argtypes = [vp, sz, vp, vp]
        lib.c12381_g1_clear_cofactor_batch.argtypes = [vp, sz, vp, vp]
        for name in ("c12381_zp_op_batch", "c12381_zp_op_batch_dev"):
            getattr(lib, name).argtypes = [vp, ci, sz, vp, vp, vp]
        lib.c12381_zp_from_hash_batch.argtypes = [vp, sz, vp, vp]
        for name in ("c12381_zp_inner_product", "c12381_zp_inner_product_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp]
        for name in ("c12381_bbs_plus_verify_batch", "c12381_bbs_plus_verify_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz] + [vp] * 10
        for name in ("c12381_bbs_plus_verify_wire_batch", "c12381_bbs_plus_verify_wire_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, sz] + [vp] * 6
        for name in ("c12381_bbs_plus_verify_aggregate", "c12381_bbs_plus_verify_aggregate_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz] + [vp] * 11
        for name in ("c12381_sha3_512_batch", "c12381_sha3_512_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, vp, vp]
        for name in ("c12381_bbs04_verify_batch", "c12381_bbs04_verify_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, vp, vp, vp, vp]
        for name in ("c12381_bbs04_open_batch", "c12381_bbs04_open_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp, vp]
        for name in ("c12381_bbs04_sign_batch", "c12381_bbs04_sign_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp]
        for name in ("c12381_bbs04_issue_batch", "c12381_bbs04_issue_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp, vp]
        for name in ("c12381_ps_verify_wire_batch", "c12381_ps_verify_wire_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, sz, ci] + [vp] * 6
        for name in ("c12381_ps_sign_batch", "c12381_ps_sign_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, sz, ci] + [vp] * 5
        for name in ("c12381_ps_randomize_batch", "c12381_ps_randomize_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, vp, vp, vp, vp]
        for name in ("c12381_ps_verify_aggregate", "c12381_ps_verify_aggregate_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz] + [vp] * 8
        for name in ("c12381_ac_bbs_verify_batch", "c12381_ac_bbs_verify_batch_dev"):      # include/c12381_ac.h
            getattr(lib, name).argtypes = [vp, sz, sz, sz, vp, sz] + [vp] * 7
        for name in ("c12381_ac_bbs_pres_batch", "c12381_ac_bbs_pres_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, sz, vp, sz] + [vp] * 9
        for name in ("c12381_ac_rbbs_verify_batch", "c12381_ac_rbbs_verify_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, sz, vp, sz] + [vp] * 7
        for name in ("c12381_ac_rbbs_pres_batch", "c12381_ac_rbbs_pres_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz] + [vp] * 6
        for name in ("c12381_ac_rbbs_redact_batch", "c12381_ac_rbbs_redact_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, sz, vp] + [vp] * 6
        for name in ("c12381_ac_rps_verify_batch", "c12381_ac_rps_verify_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, sz, vp] + [vp] * 6
        for name in ("c12381_ac_rps_pres_batch", "c12381_ac_rps_pres_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, sz, vp] + [vp] * 9
        for name in ("c12381_ac_rps_redact_batch", "c12381_ac_rps_redact_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, sz, vp] + [vp] * 5
        for name in ("c12381_mhac_bbs_verify_batch", "c12381_mhac_bbs_verify_batch_dev"):      # include/c12381_mhac.h
            getattr(lib, name).argtypes = [vp, sz, sz, sz, vp, sz, vp] + [vp] * 9
        for name in ("c12381_mhac_bbs_pres_batch", "c12381_mhac_bbs_pres_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, sz, sz, vp, sz, vp] + [vp] * 15
        for name in ("c12381_mhac_bbs_attr_batch", "c12381_mhac_bbs_attr_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, sz, sz, sz, vp] + [vp] * 6
        for name in ("c12381_mhac_bbs_iss_batch", "c12381_mhac_bbs_iss_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, sz, sz, sz, vp] + [vp] * 10
        for name in ("c12381_mhac_bbs_group_batch", "c12381_mhac_bbs_group_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, sz, vp, sz] + [vp] * 8
        for name in ("c12381_mhac_bbs_type_batch", "c12381_mhac_bbs_type_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz, sz, vp, sz, vp] + [vp] * 6
        for name in ("c12381_ac_bbs_issue_batch", "c12381_ac_bbs_issue_batch_dev", "c12381_ac_rbbs_issue_batch", "c12381_ac_rbbs_issue_batch_dev"):      # include/c12381_ac_issue.h
            getattr(lib, name).argtypes = [vp, sz, sz] + [vp] * 7
        for name in ("c12381_ac_rps_user_keygen_batch", "c12381_ac_rps_user_keygen_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz] + [vp] * 4
        for name in ("c12381_ac_rps_issue_batch", "c12381_ac_rps_issue_batch_dev"):
            getattr(lib, name).argtypes = [vp, sz, sz] + [vp] * 8
        if hasattr(lib, "c12381_exp_fp_raw_batch"):           # experiments library only: raw-limb test entry of the Fp / Fp2 leaf (tests/test_gpu_fp_raw.py)
            lib.c12381_exp_fp_raw_batch.argtypes = [vp, ci, sz, ci, ci, vp, vp, vp]
        _lib = lib
    return _lib


def _p(b):
    """bytes / ctypes buffer / int device address -> c_void_p"""
    if b is None:
        return None
    if isinstance(b, int):
        return ctypes.c_void_p(b)
    if isinstance(b, (bytes, bytearray)):
        return ctypes.cast(ctypes.c_char_p(bytes(b)), ctypes.c_void_p)
    return ctypes.cast(b, ctypes.c_void_p)


class Context:
    """One context per process/GPU (mirrors c12381_ctx)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.h = ctypes.c_void_p()
        rc = self.lib.c12381_create(device, ctypes.byref(self.h))
        if rc != 0:
            self.h = None
            raise C12381Error(rc, "c12381_create failed (no usable HIP device?)")

    def close(self):
        if getattr(self, "h", None):
            self.lib.c12381_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, allow_point=False):
        if rc == 0 or (allow_point and rc == E_POINT):
            return rc
        raise C12381Error(rc, (self.lib.c12381_last_error(self.h) or b"").decode())

    def set_stream(self, hip_stream):
        self._ck(self.lib.c12381_set_stream(self.h, _p(hip_stream)))

    def sync(self) -> int:
        return self._ck(self.lib.c12381_sync(self.h), allow_point=True)

    def trim(self):
        """free the context's device workspaces (they grow to the largest call served; the next call allocates what it needs)"""
        self._ck(self.lib.c12381_trim(self.h))

    def wait_event(self, hip_event):
        """everything this context launches from now on waits for `hip_event` (a hipEvent_t as an integer, e.g. torch.cuda.Event.cuda_event
        after record()): the device-side edge from the stream that produced a _dev call's inputs to the context's stream"""
        self._ck(self.lib.c12381_wait_event(self.h, _p(hip_event)))

    def record_event(self, hip_event):
        """record `hip_event` on the context's stream behind everything launched so far: the edge to a stream that consumes the outputs"""
        self._ck(self.lib.c12381_record_event(self.h, _p(hip_event)))

    def profile(self, enable: bool):
        self._ck(self.lib.c12381_profile(self.h, 1 if enable else 0))

    def profile_read(self, kind: int):
        ms, cnt = ctypes.c_double(), ctypes.c_uint64()
        self._ck(self.lib.c12381_profile_read(self.h, kind, ctypes.byref(ms), ctypes.byref(cnt)))
        return ms.value, cnt.value

    # ---- host-buffer entry points (bytes in, bytes out)
    FP_OPS = {"mul": 0, "add": 1, "sub": 2, "sqr": 3, "neg": 4, "inv": 5}

    def fp_op(self, op: str, a: bytes, b: bytes | None = None) -> bytes:
        n = len(a) // 48
        out = ctypes.create_string_buffer(max(48 * n, 1))
        self._ck(self.lib.c12381_fp_op_batch(self.h, self.FP_OPS[op], n, _p(a), _p(b), _p(out)))
        return out.raw[:48 * n]

    def g1_mul(self, pts: bytes, scalars: bytes, fmt: int = 49, strict: bool = True) -> bytes:
        n = len(pts) // 96
        out = ctypes.create_string_buffer(max(fmt * n, 1))
        self._ck(self.lib.c12381_g1_mul_batch(self.h, n, _p(pts), _p(scalars), _p(out), fmt), allow_point=not strict)
        return out.raw[:fmt * n]

    def g1_mul_flags(self, pts: bytes, scalars: bytes, fmt: int = 49, flags: int = 0, strict: bool = True) -> bytes:
        n = len(scalars) // 32
        out = ctypes.create_string_buffer(max(fmt * n, 1))
        self._ck(self.lib.c12381_g1_mul_batch_flags(self.h, n, _p(pts), _p(scalars), _p(out), fmt, flags), allow_point=not strict)
        return out.raw[:fmt * n]

    def g2_mul_flags(self, pts: bytes, scalars: bytes, fmt: int = 97, flags: int = 0, strict: bool = True) -> bytes:
        n = len(scalars) // 32
        out = ctypes.create_string_buffer(max(fmt * n, 1))
        self._ck(self.lib.c12381_g2_mul_batch_flags(self.h, n, _p(pts), _p(scalars), _p(out), fmt, flags), allow_point=not strict)
        return out.raw[:fmt * n]

    def g1_sum(self, pts: bytes, fmt: int = 49) -> bytes:
        n = len(pts) // 96
        out = ctypes.create_string_buffer(fmt)
        self._ck(self.lib.c12381_g1_sum(self.h, n, _p(pts), _p(out), fmt))
        return out.raw[:fmt]

    def g1_sum_dev(self, n, pts_ptr, out_ptr, fmt=49):
        self._ck(self.lib.c12381_g1_sum_dev(self.h, n, _p(pts_ptr), _p(out_ptr), fmt))

    def g1_msm_flags(self, pts: bytes, scalars: bytes, fmt: int = 49, flags: int = 0, strict: bool = True) -> bytes:
        n = len(scalars) // 32
        out = ctypes.create_string_buffer(fmt)
        self._ck(self.lib.c12381_g1_msm_flags(self.h, n, _p(pts), _p(scalars), _p(out), fmt, flags), allow_point=not strict)
        return out.raw[:fmt]

    def pair_flags(self, g1: bytes, g2: bytes, flags: int = 0, strict: bool = True) -> bytes:
        n = len(g1) // (49 if flags & F_COMPRESSED_IN else 96)
        out = ctypes.create_string_buffer(max(576 * n, 1))
        self._ck(self.lib.c12381_pair_batch_flags(self.h, n, _p(g1), _p(g2), _p(out), flags), allow_point=not strict)
        return out.raw[:576 * n]

    def g1_mul_flags_dev(self, n, pts_ptr, sc_ptr, out_ptr, fmt=49, flags=0):
        self._ck(self.lib.c12381_g1_mul_batch_flags_dev(self.h, n, _p(pts_ptr), _p(sc_ptr), _p(out_ptr), fmt, flags))

    def g2_mul_flags_dev(self, n, pts_ptr, sc_ptr, out_ptr, fmt=97, flags=0):
        self._ck(self.lib.c12381_g2_mul_batch_flags_dev(self.h, n, _p(pts_ptr), _p(sc_ptr), _p(out_ptr), fmt, flags))

    def g1_mul_sum(self, pts: bytes, scalars: bytes, k: int, fmt: int = 49, flags: int = 0, strict: bool = True) -> bytes:
        """out[i] = sum over j < k of scalars[j n + i] * pts[j n + i]: k powers per lane under one doubling chain (the reference's
        g^x * h^y, double_multiply).  pts / scalars: k argument-major arrays of n records; 1 <= k <= 4; returns n points of `fmt` bytes.
        Every lane equals multiply on each term followed by add; flags: F_IN_SUBGROUP only"""
        n = len(scalars) // (32 * k) if k > 0 else 0
        out = ctypes.create_string_buffer(max(fmt * n, 1))
        self._ck(self.lib.c12381_g1_mul_sum_batch(self.h, n, k, _p(pts), _p(scalars), _p(out), fmt, flags), allow_point=not strict)
        return out.raw[:fmt * n]

    def g1_mul_sum_dev(self, n, k, pts_ptr, sc_ptr, out_ptr, fmt=49, flags=0):
        self._ck(self.lib.c12381_g1_mul_sum_batch_dev(self.h, n, k, _p(pts_ptr), _p(sc_ptr), _p(out_ptr), fmt, flags))

    def g1_add(self, a: bytes, b: bytes, fmt: int = 96, strict: bool = True) -> bytes:
        n = len(a) // 96
        out = ctypes.create_string_buffer(max(fmt * n, 1))
        self._ck(self.lib.c12381_g1_add_batch(self.h, n, _p(a), _p(b), _p(out), fmt), allow_point=not strict)
        return out.raw[:fmt * n]

    def g1_msm(self, pts: bytes, scalars: bytes, fmt: int = 49) -> bytes:
        n = len(pts) // 96
        out = ctypes.create_string_buffer(fmt)
        self._ck(self.lib.c12381_g1_msm(self.h, n, _p(pts), _p(scalars), _p(out), fmt))
        return out.raw[:fmt]

    def g2_mul(self, pts: bytes, scalars: bytes, fmt: int = 97, strict: bool = True) -> bytes:
        n = len(pts) // 192
        out = ctypes.create_string_buffer(max(fmt * n, 1))
        self._ck(self.lib.c12381_g2_mul_batch(self.h, n, _p(pts), _p(scalars), _p(out), fmt), allow_point=not strict)
        return out.raw[:fmt * n]

    def g1_sum_of_products(self, pts: bytes, scalars: bytes, fmt: int = 49) -> bytes:
        n = len(pts) // 96
        out = ctypes.create_string_buffer(fmt)
        self._ck(self.lib.c12381_g1_sum_of_products(self.h, n, _p(pts) if n else None, _p(scalars) if n else None, _p(out), fmt))
        return out.raw[:fmt]

    def g2_msm(self, pts: bytes, scalars: bytes | None, fmt: int = 97) -> bytes:
        n = len(pts) // 192
        out = ctypes.create_string_buffer(fmt)
        self._ck(self.lib.c12381_g2_msm(self.h, n, _p(pts) if n else None, _p(scalars) if scalars else None, _p(out), fmt))
        return out.raw[:fmt]

    def g2_add(self, a: bytes, b: bytes, fmt: int = 192, strict: bool = True) -> bytes:
        n = len(a) // 192
        out = ctypes.create_string_buffer(max(fmt * n, 1))
        self._ck(self.lib.c12381_g2_add_batch(self.h, n, _p(a), _p(b), _p(out), fmt), allow_point=not strict)
        return out.raw[:fmt * n]

    def pair(self, g1: bytes, g2: bytes, strict: bool = True) -> bytes:
        n = len(g1) // 96
        out = ctypes.create_string_buffer(max(576 * n, 1))
        self._ck(self.lib.c12381_pair_batch(self.h, n, _p(g1), _p(g2), _p(out)), allow_point=not strict)
        return out.raw[:576 * n]

    def pair_product(self, g1s: bytes, g2s: bytes, k: int, flags: int = 0) -> bytes:
        """g1s / g2s: k argument-major arrays of n points; returns n GT (or Miller) values"""
        n = len(g1s) // (96 * k)
        out = ctypes.create_string_buffer(max(576 * n, 1))
        self._ck(self.lib.c12381_pair_product_batch(self.h, n, k, _p(g1s), _p(g2s), _p(out), flags))
        return out.raw[:576 * n]

    def pair_fixed_g2(self, g1: bytes, g2_one: bytes, strict: bool = True) -> bytes:
        n = len(g1) // 96
        out = ctypes.create_string_buffer(max(576 * n, 1))
        self._ck(self.lib.c12381_pair_fixed_g2_batch(self.h, n, _p(g1), _p(g2_one), _p(out)), allow_point=not strict)
        return out.raw[:576 * n]

    def pair_fixed_g2_dev(self, n, g1_ptr, g2_ptr, gt_ptr):
        self._ck(self.lib.c12381_pair_fixed_g2_batch_dev(self.h, n, _p(g1_ptr), _p(g2_ptr), _p(gt_ptr)))

    def pair_product_fixed_g2(self, g1s: bytes, g2s: bytes, k: int, flags: int = 0, strict: bool = True) -> bytes:
        """g1s: k argument-major arrays of n points, g2s: k points shared by the batch; returns n GT (or, with MILLER_ONLY, Miller) values"""
        n = len(g1s) // (96 * k) if k > 0 else 0
        out = ctypes.create_string_buffer(max(576 * n, 1))
        self._ck(self.lib.c12381_pair_product_fixed_g2_batch(self.h, n, k, _p(g1s), _p(g2s), _p(out), flags), allow_point=not strict)
        return out.raw[:576 * n]

    def pair_product_fixed_g2_dev(self, n, k, g1s_ptr, g2s_ptr, gt_ptr, flags: int = 0):
        self._ck(self.lib.c12381_pair_product_fixed_g2_batch_dev(self.h, n, k, _p(g1s_ptr), _p(g2s_ptr), _p(gt_ptr), flags))

    def ps_verify(self, g2: bytes, X2: bytes, Y2: bytes, s1: bytes, s2: bytes, m: bytes, strict: bool = True) -> bytes:
        """PS: Y2 holds nmsg points, m is message-major (scalar i of signature j at m[32*(i*n + j)]); one byte per signature"""
        n = len(s1) // 96
        nmsg = len(Y2) // 192
        out = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_ps_verify_batch(self.h, n, nmsg, _p(g2), _p(X2), _p(Y2) if nmsg else None, _p(s1), _p(s2),
                                                 _p(m) if nmsg else None, _p(out)), allow_point=not strict)
        return out.raw[:n]

    def ps_verify_dev(self, n, nmsg, g2, X2, Y2, s1, s2, m, ok):
        self._ck(self.lib.c12381_ps_verify_batch_dev(self.h, n, nmsg, _p(g2), _p(X2), _p(Y2), _p(s1), _p(s2), _p(m), _p(ok)))

    def ps_verify_wire(self, g2_97: bytes, X2_97: bytes, Y2_97: bytes, sigs98: bytes, msgs: bytes, msg_len: int, mode: int, strict: bool = True) -> bytes:
        """PS verify from the wire formats: key points (97 B each, Y2 holds nY of them), signatures (98 B each), messages of msg_len bytes each;
        mode PS_MSG_HASH (nY = 1) or PS_MSG_ENCODE.  One byte per signature: 1 / 0, or 0xff where the reference would throw.  A key point that
        does not decode is C12381_E_POINT (every byte 0xff): raised when strict, returned as bytes otherwise."""
        n, nY = len(sigs98) // 98, len(Y2_97) // 97
        out = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_ps_verify_wire_batch(self.h, n, nY, msg_len, mode, _p(g2_97), _p(X2_97), _p(Y2_97) if nY else None, _p(sigs98),
                                                      _p(msgs) if msg_len else None, _p(out)), allow_point=not strict)
        return out.raw[:n]

    def ps_verify_wire_dev(self, n, nY, msg_len, mode, g2_ptr, X2_ptr, Y2_ptr, sig_ptr, msg_ptr, ok_ptr):
        self._ck(self.lib.c12381_ps_verify_wire_batch_dev(self.h, n, nY, msg_len, mode, _p(g2_ptr), _p(X2_ptr), _p(Y2_ptr), _p(sig_ptr), _p(msg_ptr),
                                                          _p(ok_ptr)))

    def ps_sign(self, x48: bytes, y48: bytes, msgs: bytes, t32: bytes, msg_len: int, mode: int, strict: bool = True) -> bytes:
        """PS sign: secret key x (48 B) and y (nY x 48 B), messages of msg_len bytes each, the caller's randomness t (32 B per signature) ->
        n x 98-byte signatures serialize(G^t, G^(t e)).  x or a used y_i >= r is C12381_E_ARG (every byte 0xff): raised when strict, returned
        as bytes otherwise.  Not constant-time."""
        n, nY = len(t32) // 32, len(y48) // 48
        out = ctypes.create_string_buffer(max(98 * n, 1))
        rc = self.lib.c12381_ps_sign_batch(self.h, n, nY, msg_len, mode, _p(x48), _p(y48) if nY else None, _p(msgs) if msg_len else None, _p(t32), _p(out))
        if not (rc == E_ARG and not strict and out.raw[:98 * n] == b"\xff" * (98 * n) and n):
            self._ck(rc)
        return out.raw[:98 * n]

    def ps_sign_dev(self, n, nY, msg_len, mode, x_ptr, y_ptr, msg_ptr, t_ptr, sig_ptr):
        self._ck(self.lib.c12381_ps_sign_batch_dev(self.h, n, nY, msg_len, mode, _p(x_ptr), _p(y_ptr), _p(msg_ptr), _p(t_ptr), _p(sig_ptr)))

    def ps_randomize(self, sigs98: bytes, r32: bytes):
        """PS randomnize: (n x 98-byte signatures serialize(σ1^r, σ2^r), n status bytes: 0, or 0xff — and 98 bytes of 0xff — where σ1 or σ2
        does not decode)"""
        n = len(sigs98) // 98
        out = ctypes.create_string_buffer(max(98 * n, 1))
        st = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_ps_randomize_batch(self.h, n, _p(sigs98), _p(r32), _p(out), _p(st)))
        return out.raw[:98 * n], st.raw[:n]

    def ps_randomize_dev(self, n, sig_ptr, r_ptr, out_ptr, status_ptr):
        self._ck(self.lib.c12381_ps_randomize_batch_dev(self.h, n, _p(sig_ptr), _p(r_ptr), _p(out_ptr), _p(status_ptr)))

    def ps_verify_aggregate(self, g2: bytes, X2: bytes, Y2: bytes, s1: bytes, s2: bytes, m: bytes, rho: bytes, strict: bool = True) -> bool:
        """ONE verdict for a PS batch by a random linear combination (rho: n x 32 B caller-drawn scalars; inputs as ps_verify).  True: every
        signature verifies (up to 2^-k for k-bit rho); False settles nothing — run ps_verify.  A signature point off the curve is
        C12381_E_POINT: raised when strict, False otherwise."""
        n = len(s1) // 96
        nmsg = len(Y2) // 192
        out = ctypes.c_int(0)
        self._ck(self.lib.c12381_ps_verify_aggregate(self.h, n, nmsg, _p(g2), _p(X2), _p(Y2) if nmsg else None, _p(s1) if n else None,
                                                     _p(s2) if n else None, _p(m) if nmsg and n else None, _p(rho) if n else None, ctypes.byref(out)),
                 allow_point=not strict)
        return out.value == 1

    def ps_verify_aggregate_dev(self, n, nmsg, g2, X2, Y2, s1, s2, m, rho, all_ok):
        self._ck(self.lib.c12381_ps_verify_aggregate_dev(self.h, n, nmsg, _p(g2), _p(X2), _p(Y2), _p(s1), _p(s2), _p(m), _p(rho), _p(all_ok)))

    def pair_eq(self, a1: bytes, a2: bytes, b1: bytes, b2: bytes, strict: bool = True) -> bytes:
        n = len(a1) // 96
        out = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_pair_eq_batch(self.h, n, _p(a1), _p(a2), _p(b1), _p(b2), _p(out)), allow_point=not strict)
        return out.raw[:n]

    def g1_decompress(self, c: bytes):
        n = len(c) // 49
        out, st = ctypes.create_string_buffer(max(96 * n, 1)), ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_g1_decompress_batch(self.h, n, _p(c), _p(out), _p(st)))
        return out.raw[:96 * n], st.raw[:n]

    def g2_decompress(self, c: bytes):
        n = len(c) // 97
        out, st = ctypes.create_string_buffer(max(192 * n, 1)), ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_g2_decompress_batch(self.h, n, _p(c), _p(out), _p(st)))
        return out.raw[:192 * n], st.raw[:n]

    def g1_from_hash(self, digests: bytes, fmt: int = 96) -> bytes:
        n = len(digests) // 64
        out = ctypes.create_string_buffer(max(fmt * n, 1))
        self._ck(self.lib.c12381_g1_from_hash_batch(self.h, n, _p(digests), _p(out), fmt))
        return out.raw[:fmt * n]

    def g1_mul_fixed(self, base: bytes, scalars: bytes, fmt: int = 49, strict: bool = True) -> bytes:
        n = len(scalars) // 32
        out = ctypes.create_string_buffer(max(fmt * n, 1))
        self._ck(self.lib.c12381_g1_mul_fixed_batch(self.h, n, _p(base), _p(scalars), _p(out), fmt), allow_point=not strict)
        return out.raw[:fmt * n]

    def g2_mul_fixed(self, base: bytes, scalars: bytes, fmt: int = 97, strict: bool = True) -> bytes:
        n = len(scalars) // 32
        out = ctypes.create_string_buffer(max(fmt * n, 1))
        self._ck(self.lib.c12381_g2_mul_fixed_batch(self.h, n, _p(base), _p(scalars), _p(out), fmt), allow_point=not strict)
        return out.raw[:fmt * n]

    def g1_mul_fixed_dev(self, n, base_ptr, sc_ptr, out_ptr, fmt=49):
        self._ck(self.lib.c12381_g1_mul_fixed_batch_dev(self.h, n, _p(base_ptr), _p(sc_ptr), _p(out_ptr), fmt))

    def g2_mul_fixed_dev(self, n, base_ptr, sc_ptr, out_ptr, fmt=97):
        self._ck(self.lib.c12381_g2_mul_fixed_batch_dev(self.h, n, _p(base_ptr), _p(sc_ptr), _p(out_ptr), fmt))

    def g1_mul_fixed_sum(self, bases: bytes, scalars: bytes, addend: bytes | None = None, fmt: int = 49, strict: bool = True) -> bytes:
        """out[j] = addend + sum over i < nb of scalars[i n + j] * bases[i]: per-lane products over nb = len(bases) // 96 public bases shared by
        the batch (1 <= nb <= 32), served from nb fixed-base tables when every base is a subgroup point.  scalars: base-major, nb arrays of n
        records; addend: one 96-byte point or None; returns n points of `fmt` bytes.  Every lane equals multiply on each term followed by add"""
        nb = len(bases) // 96
        n = len(scalars) // (32 * nb) if nb > 0 else 0
        out = ctypes.create_string_buffer(max(fmt * n, 1))
        self._ck(self.lib.c12381_g1_mul_fixed_sum_batch(self.h, n, nb, _p(bases), _p(addend), _p(scalars), _p(out), fmt), allow_point=not strict)
        return out.raw[:fmt * n]

    def g1_mul_fixed_sum_dev(self, n, nb, bases_ptr, sc_ptr, out_ptr, addend_ptr=None, fmt=49):
        self._ck(self.lib.c12381_g1_mul_fixed_sum_batch_dev(self.h, n, nb, _p(bases_ptr), _p(addend_ptr), _p(sc_ptr), _p(out_ptr), fmt))

    def g2_mul_fixed_sum(self, bases: bytes, scalars: bytes, addend: bytes | None = None, fmt: int = 97, strict: bool = True) -> bytes:
        """The G2 form of g1_mul_fixed_sum: nb = len(bases) // 192 public G2 bases shared by the batch (1 <= nb <= 32), served from nb fixed-base
        tables when every base is an element of G2.  scalars: base-major, nb arrays of n records; addend: one 192-byte point or None; returns
        n points of `fmt` bytes (97 or 192).  Every lane equals multiply on each term followed by add, for every point of the twist"""
        nb = len(bases) // 192
        n = len(scalars) // (32 * nb) if nb > 0 else 0
        out = ctypes.create_string_buffer(max(fmt * n, 1))
        self._ck(self.lib.c12381_g2_mul_fixed_sum_batch(self.h, n, nb, _p(bases), _p(addend), _p(scalars), _p(out), fmt), allow_point=not strict)
        return out.raw[:fmt * n]

    def g2_mul_fixed_sum_dev(self, n, nb, bases_ptr, sc_ptr, out_ptr, addend_ptr=None, fmt=97):
        self._ck(self.lib.c12381_g2_mul_fixed_sum_batch_dev(self.h, n, nb, _p(bases_ptr), _p(addend_ptr), _p(sc_ptr), _p(out_ptr), fmt))

    def g1_map_to_point(self, u48: bytes) -> bytes:
        n = len(u48) // 48
        out = ctypes.create_string_buffer(max(96 * n, 1))
        self._ck(self.lib.c12381_g1_map_to_point_batch(self.h, n, _p(u48), _p(out)))
        return out.raw[:96 * n]

    def g1_clear_cofactor(self, pts: bytes, strict: bool = True) -> bytes:
        n = len(pts) // 96
        out = ctypes.create_string_buffer(max(96 * n, 1))
        self._ck(self.lib.c12381_g1_clear_cofactor_batch(self.h, n, _p(pts), _p(out)), allow_point=not strict)
        return out.raw[:96 * n]

    ZP_OPS = {"mul": 0, "add": 1, "sub": 2, "neg": 3, "inv": 4}

    def zp_op(self, op: str, a: bytes, b: bytes | None = None) -> bytes:
        n = len(a) // 32
        out = ctypes.create_string_buffer(max(32 * n, 1))
        self._ck(self.lib.c12381_zp_op_batch(self.h, self.ZP_OPS[op], n, _p(a), _p(b), _p(out)))
        return out.raw[:32 * n]

    def zp_from_hash(self, digests: bytes) -> bytes:
        n = len(digests) // 64
        out = ctypes.create_string_buffer(max(32 * n, 1))
        self._ck(self.lib.c12381_zp_from_hash_batch(self.h, n, _p(digests), _p(out)))
        return out.raw[:32 * n]

    def zp_inner_product(self, a: bytes, b: bytes | None = None) -> bytes:
        n = len(a) // 32
        out = ctypes.create_string_buffer(32)
        self._ck(self.lib.c12381_zp_inner_product(self.h, n, _p(a), _p(b), _p(out)))
        return out.raw

    def miller(self, g1: bytes, g2: bytes) -> bytes:
        n = len(g1) // 96
        out = ctypes.create_string_buffer(max(576 * n, 1))
        self._ck(self.lib.c12381_miller_batch(self.h, n, _p(g1), _p(g2), _p(out)))
        return out.raw[:576 * n]

    def fexp(self, f: bytes) -> bytes:
        n = len(f) // 576
        out = ctypes.create_string_buffer(max(576 * n, 1))
        self._ck(self.lib.c12381_fexp_batch(self.h, n, _p(f), _p(out)))
        return out.raw[:576 * n]

    GT_OPS = {"mul": 0, "conj": 1, "pow": 2, "fexp": 3}

    def gt_op(self, op: str, a: bytes, b: bytes | None = None) -> bytes:
        n = len(a) // 576
        out = ctypes.create_string_buffer(max(576 * n, 1))
        self._ck(self.lib.c12381_gt_op_batch(self.h, self.GT_OPS[op], n, _p(a), _p(b), _p(out)))
        return out.raw[:576 * n]

    def gt_is_unity(self, a: bytes) -> bytes:
        n = len(a) // 576
        out = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_gt_is_unity_batch(self.h, n, _p(a), _p(out)))
        return out.raw[:n]

    def bbs_plus_verify(self, g1: bytes, g2: bytes, h0: bytes, h: bytes, w: bytes, A: bytes, x: bytes, r: bytes, m: bytes,
                        strict: bool = True) -> bytes:
        """m is message-major: block i of signature j at m[32*(i*n + j)]."""
        n = len(A) // 96
        nmsg = len(h) // 96
        out = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_bbs_plus_verify_batch(self.h, n, nmsg, _p(g1), _p(g2), _p(h0), _p(h) if nmsg else None, _p(w), _p(A),
                                                       _p(x), _p(r), _p(m) if nmsg else None, _p(out)), allow_point=not strict)
        return out.raw[:n]

    def bbs_plus_verify_wire(self, g1_g2_h0: bytes, h49: bytes, pk97: bytes, sigs145: bytes, msgs: bytes, msg_len: int, strict: bool = True) -> bytes:
        """serialized public parameters / key / signatures (49 + 48 + 48 B) and raw messages in, one byte per signature out"""
        n, nh = len(sigs145) // 145, len(h49) // 49
        out = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_bbs_plus_verify_wire_batch(self.h, n, nh, msg_len, _p(g1_g2_h0), _p(h49) if nh else None, _p(pk97), _p(sigs145),
                                                            _p(msgs) if msg_len else None, _p(out)), allow_point=not strict)
        return out.raw[:n]

    def bbs_plus_verify_aggregate(self, g1: bytes, g2: bytes, h0: bytes, h: bytes, w: bytes, A: bytes, x: bytes, r: bytes, m: bytes,
                                  rho: bytes) -> bool:
        """ONE verdict for the batch by a random linear combination (rho: n x 32 B caller-drawn scalars).  True: every
        signature verifies (up to 2^-k for k-bit rho); False settles nothing — run bbs_plus_verify."""
        n = len(A) // 96
        nmsg = len(h) // 96
        out = ctypes.c_int(0)
        self._ck(self.lib.c12381_bbs_plus_verify_aggregate(self.h, n, nmsg, _p(g1), _p(g2), _p(h0), _p(h) if nmsg else None, _p(w),
                                                           _p(A) if n else None, _p(x) if n else None, _p(r) if n else None,
                                                           _p(m) if nmsg and n else None, _p(rho) if n else None, ctypes.byref(out)))
        return out.value == 1

    def bbs_plus_verify_aggregate_dev(self, n, nmsg, g1, g2, h0, h, w, A, x, r, m, rho, all_ok):
        self._ck(self.lib.c12381_bbs_plus_verify_aggregate_dev(self.h, n, nmsg, _p(g1), _p(g2), _p(h0), _p(h), _p(w), _p(A), _p(x), _p(r),
                                                               _p(m), _p(rho), _p(all_ok)))

    def bbs_plus_verify_dev(self, n, nmsg, g1, g2, h0, h, w, A, x, r, m, ok):
        self._ck(self.lib.c12381_bbs_plus_verify_batch_dev(self.h, n, nmsg, _p(g1), _p(g2), _p(h0), _p(h), _p(w), _p(A), _p(x), _p(r),
                                                           _p(m), _p(ok)))

    def sha3_512(self, msgs: bytes, n: int, length: int) -> bytes:
        """n messages of `length` bytes each, contiguous (length 0 allowed) -> n 64-byte SHA3-512 digests (hash_state's SHA3)"""
        out = ctypes.create_string_buffer(max(64 * n, 1))
        self._ck(self.lib.c12381_sha3_512_batch(self.h, n, length, _p(msgs) if length else None, _p(out)))
        return out.raw[:64 * n]

    def sha3_512_dev(self, n, length, msgs_ptr, out_ptr):
        self._ck(self.lib.c12381_sha3_512_batch_dev(self.h, n, length, _p(msgs_ptr), _p(out_ptr)))

    def bbs04_verify(self, gpk390: bytes, sigs435: bytes, msgs: bytes, msg_len: int, strict: bool = True) -> bytes:
        """bbs04 verify from the wire formats: gpk (390 B), signatures (435 B each), messages of msg_len bytes each.  One byte per
        signature: 1 / 0, or 0xff where the reference would terminate.  A gpk that does not decode is C12381_E_POINT (every byte
        0xff): raised when strict, returned as bytes otherwise."""
        n = len(sigs435) // 435
        out = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_bbs04_verify_batch(self.h, n, msg_len, _p(gpk390), _p(sigs435), _p(msgs) if msg_len else None, _p(out)),
                 allow_point=not strict)
        return out.raw[:n]

    def bbs04_verify_dev(self, n, msg_len, gpk_ptr, sig_ptr, msg_ptr, ok_ptr):
        self._ck(self.lib.c12381_bbs04_verify_batch_dev(self.h, n, msg_len, _p(gpk_ptr), _p(sig_ptr), _p(msg_ptr), _p(ok_ptr)))

    def bbs04_open(self, gmsk96: bytes, sigs435: bytes, strict: bool = True):
        """bbs04 open: (n x 49-byte points T3 / (T1^xi1 T2^xi2), n status bytes: 0, or 0xff where the reference would terminate).
        A gmsk scalar >= r is C12381_E_ARG (every status 0xff): raised when strict, returned otherwise."""
        n = len(sigs435) // 435
        out = ctypes.create_string_buffer(max(49 * n, 1))
        st = ctypes.create_string_buffer(max(n, 1))
        rc = self.lib.c12381_bbs04_open_batch(self.h, n, _p(gmsk96), _p(sigs435), _p(out), _p(st))
        if not (rc == E_ARG and not strict and len(gmsk96) == 96 and n):
            self._ck(rc)
        return out.raw[:49 * n], st.raw[:n]

    def bbs04_open_dev(self, n, gmsk_ptr, sig_ptr, out_ptr, status_ptr):
        self._ck(self.lib.c12381_bbs04_open_batch_dev(self.h, n, _p(gmsk_ptr), _p(sig_ptr), _p(out_ptr), _p(status_ptr)))

    def bbs04_sign(self, gpk390: bytes, gsk97: bytes, msgs: bytes, rnd224: bytes, msg_len: int, strict: bool = True):
        """bbs04 sign from the wire formats: gpk (390 B), member keys serialize(A, x) (97 B each), messages of msg_len bytes each and the
        caller's randomness (alpha, beta, r_alpha, r_beta, r_x, r_delta1, r_delta2: 7 x 32 B per signature) -> (n x 435-byte signatures,
        n status bytes: 0, or 0xff — and 435 bytes of 0xff — where the reference would terminate).  A gpk that does not decode is
        C12381_E_POINT (every byte 0xff): raised when strict, returned as bytes otherwise.  Not constant-time."""
        n = len(gsk97) // 97
        sig = ctypes.create_string_buffer(max(435 * n, 1))
        st = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_bbs04_sign_batch(self.h, n, msg_len, _p(gpk390), _p(gsk97), _p(msgs) if msg_len else None, _p(rnd224), _p(sig),
                                                  _p(st)), allow_point=not strict)
        return sig.raw[:435 * n], st.raw[:n]

    def bbs04_sign_dev(self, n, msg_len, gpk_ptr, gsk_ptr, msg_ptr, rnd_ptr, sig_ptr, status_ptr):
        self._ck(self.lib.c12381_bbs04_sign_batch_dev(self.h, n, msg_len, _p(gpk_ptr), _p(gsk_ptr), _p(msg_ptr), _p(rnd_ptr), _p(sig_ptr),
                                                      _p(status_ptr)))

    def bbs04_issue(self, gpk390: bytes, gamma32: bytes, x32: bytes, strict: bool = True) -> bytes:
        """bbs04 member keys as key_gen issues them: n x serialize(g1^inverse(gamma + x_i), x_i) (97 B each) for n 32-byte scalars x_i.
        A gpk that does not decode is C12381_E_POINT (every byte 0xff): raised when strict, returned as bytes otherwise."""
        n = len(x32) // 32
        out = ctypes.create_string_buffer(max(97 * n, 1))
        self._ck(self.lib.c12381_bbs04_issue_batch(self.h, n, _p(gpk390), _p(gamma32), _p(x32), _p(out)), allow_point=not strict)
        return out.raw[:97 * n]

    def bbs04_issue_dev(self, n, gpk_ptr, gamma_ptr, x_ptr, gsk_ptr):
        self._ck(self.lib.c12381_bbs04_issue_batch_dev(self.h, n, _p(gpk_ptr), _p(gamma_ptr), _p(x_ptr), _p(gsk_ptr)))

    @staticmethod
    def _idx(idx):
        """the disclosure set I as the host array of uint32_t the AC-bbs entries take"""
        idx = list(idx)
        return (ctypes.c_uint32 * max(len(idx), 1))(*idx), len(idx)

    def ac_bbs_verify(self, pk243: bytes, Y49: bytes, idx, pres243: bytes, u48: bytes, attr48: bytes, msgs: bytes, msg_len: int,
                      strict: bool = True) -> bytes:
        """AC-bbs verify from the wire formats (include/c12381_ac.h): pk.fixed_part (243 B), pk.Y (49 B each), the disclosure set idx,
        PresInfo.fixed_part (243 B each), PresInfo.u (nJ x 48 B each), the DISCLOSED attributes (nI x 48 B each, in the order of idx) and
        messages of msg_len bytes each.  One byte per presentation: 1 / 0, or 0xff where the reference would throw.  A pk that does not
        decode is C12381_E_POINT (every byte 0xff): raised when strict, returned as bytes otherwise."""
        n, nattr = len(pres243) // 243, len(Y49) // 49
        arr, nI = self._idx(idx)
        out = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_ac_bbs_verify_batch(self.h, n, nattr, nI, arr, msg_len, _p(pk243), _p(Y49), _p(pres243), _p(u48) if nattr > nI else None,
                                                     _p(attr48) if nI else None, _p(msgs) if msg_len else None, _p(out)), allow_point=not strict)
        return out.raw[:n]

    def ac_bbs_verify_dev(self, n, nattr, idx, msg_len, pk_ptr, Y_ptr, pres_ptr, u_ptr, attr_ptr, msg_ptr, ok_ptr):
        arr, nI = self._idx(idx)
        self._ck(self.lib.c12381_ac_bbs_verify_batch_dev(self.h, n, nattr, nI, arr, msg_len, _p(pk_ptr), _p(Y_ptr), _p(pres_ptr), _p(u_ptr), _p(attr_ptr),
                                                         _p(msg_ptr), _p(ok_ptr)))

    def ac_bbs_pres(self, pk243: bytes, Y49: bytes, idx, attr48: bytes, sigs97: bytes, msgs: bytes, rnd: bytes, msg_len: int, strict: bool = True):
        """AC-bbs pres from the wire formats: the holder's whole attribute spans (nattr x 48 B each), signatures serialize(A, w) (97 B each),
        messages and the caller's randomness (r, alpha, beta, delta_0 ..: (3 + nJ) x 32 B per presentation) -> (n x 243-byte
        PresInfo.fixed_part, n x nJ x 48-byte PresInfo.u, n status bytes: 0, or 0xff — and records of 0xff — where the reference would
        throw).  A pk that does not decode is C12381_E_POINT (every byte 0xff): raised when strict, returned as bytes otherwise.  Not
        constant-time."""
        n, nattr = len(sigs97) // 97, len(Y49) // 49
        arr, nI = self._idx(idx)
        nJ = max(nattr - nI, 0)
        pres = ctypes.create_string_buffer(max(243 * n, 1))
        u = ctypes.create_string_buffer(max(48 * nJ * n, 1))
        st = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_ac_bbs_pres_batch(self.h, n, nattr, nI, arr, msg_len, _p(pk243), _p(Y49), _p(attr48), _p(sigs97),
                                                   _p(msgs) if msg_len else None, _p(rnd), _p(pres), _p(u), _p(st)), allow_point=not strict)
        return pres.raw[:243 * n], u.raw[:48 * nJ * n], st.raw[:n]

    def ac_bbs_pres_dev(self, n, nattr, idx, msg_len, pk_ptr, Y_ptr, attr_ptr, sig_ptr, msg_ptr, rnd_ptr, pres_ptr, u_ptr, status_ptr):
        arr, nI = self._idx(idx)
        self._ck(self.lib.c12381_ac_bbs_pres_batch_dev(self.h, n, nattr, nI, arr, msg_len, _p(pk_ptr), _p(Y_ptr), _p(attr_ptr), _p(sig_ptr), _p(msg_ptr),
                                                       _p(rnd_ptr), _p(pres_ptr), _p(u_ptr), _p(status_ptr)))

    def ac_rbbs_verify(self, pk243: bytes, Y49: bytes, tY97: bytes, idx, pres341: bytes, attr48: bytes, msgs: bytes, msg_len: int,
                       strict: bool = True) -> bytes:
        """AC-rbbs verify from the wire formats (include/c12381_ac.h): pk.fixed_part (243 B), pk.Y (2 nattr x 49 B), pk.tilde_Y (nattr x 97 B),
        the disclosure set idx, PresInfo (341 B each), the DISCLOSED attributes (nI x 48 B each, in the order of idx) and messages of msg_len
        bytes each.  One byte per presentation: 1 / 0, or 0xff where the reference would throw.  A used key record that does not decode is
        C12381_E_POINT (every byte 0xff): raised when strict, returned as bytes otherwise."""
        n, nattr = len(pres341) // 341, len(tY97) // 97
        arr, nI = self._idx(idx)
        out = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_ac_rbbs_verify_batch(self.h, n, nattr, nI, arr, msg_len, _p(pk243), _p(Y49), _p(tY97), _p(pres341),
                                                      _p(attr48) if nI else None, _p(msgs) if msg_len else None, _p(out)), allow_point=not strict)
        return out.raw[:n]

    def ac_rbbs_verify_dev(self, n, nattr, idx, msg_len, pk_ptr, Y_ptr, tY_ptr, pres_ptr, attr_ptr, msg_ptr, ok_ptr):
        arr, nI = self._idx(idx)
        self._ck(self.lib.c12381_ac_rbbs_verify_batch_dev(self.h, n, nattr, nI, arr, msg_len, _p(pk_ptr), _p(Y_ptr), _p(tY_ptr), _p(pres_ptr), _p(attr_ptr),
                                                          _p(msg_ptr), _p(ok_ptr)))

    def ac_rbbs_pres(self, sigs97: bytes, cache196: bytes, msgs: bytes, rnd: bytes, msg_len: int):
        """AC-rbbs pres from the wire formats: signatures serialize(A, w) (97 B each), redact caches (196 B each), messages and the caller's
        randomness (r, alpha, beta: 3 x 32 B per presentation) -> (n x 341-byte PresInfo, n status bytes: 0, or 0xff — and a record of 0xff —
        where the reference would throw).  Not constant-time."""
        n = len(sigs97) // 97
        pres, st = ctypes.create_string_buffer(max(341 * n, 1)), ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_ac_rbbs_pres_batch(self.h, n, msg_len, _p(sigs97), _p(cache196), _p(msgs) if msg_len else None, _p(rnd), _p(pres), _p(st)))
        return pres.raw[:341 * n], st.raw[:n]

    def ac_rbbs_pres_dev(self, n, msg_len, sig_ptr, cache_ptr, msg_ptr, rnd_ptr, pres_ptr, status_ptr):
        self._ck(self.lib.c12381_ac_rbbs_pres_batch_dev(self.h, n, msg_len, _p(sig_ptr), _p(cache_ptr), _p(msg_ptr), _p(rnd_ptr), _p(pres_ptr), _p(status_ptr)))

    def ac_rbbs_redact(self, pk243: bytes, Y49: bytes, idx, attr48: bytes, sigs97: bytes, strict: bool = True):
        """AC-rbbs redact from the wire formats: pk.fixed_part, pk.Y (2 nattr x 49 B, nattr <= 16), the disclosure set idx, the holder's whole
        attribute spans (nattr x 48 B each) and signatures (97 B each) -> (n x 196-byte RedactCache, n status bytes: 0, or 0xff — and a record
        of 0xff — where the reference would throw).  A key that does not decode is C12381_E_POINT (every byte 0xff): raised when strict,
        returned as bytes otherwise.  Not constant-time."""
        n, nattr = len(sigs97) // 97, len(Y49) // 98
        arr, nI = self._idx(idx)
        cache, st = ctypes.create_string_buffer(max(196 * n, 1)), ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_ac_rbbs_redact_batch(self.h, n, nattr, nI, arr, _p(pk243), _p(Y49), _p(attr48), _p(sigs97), _p(cache), _p(st)),
                 allow_point=not strict)
        return cache.raw[:196 * n], st.raw[:n]

    def ac_rbbs_redact_dev(self, n, nattr, idx, pk_ptr, Y_ptr, attr_ptr, sig_ptr, cache_ptr, status_ptr):
        arr, nI = self._idx(idx)
        self._ck(self.lib.c12381_ac_rbbs_redact_batch_dev(self.h, n, nattr, nI, arr, _p(pk_ptr), _p(Y_ptr), _p(attr_ptr), _p(sig_ptr), _p(cache_ptr),
                                                          _p(status_ptr)))

    def ac_rps_verify(self, pk243: bytes, Y49: bytes, tY97: bytes, idx, pres389: bytes, attr48: bytes, strict: bool = True, dev: bool = False) -> bytes:
        """AC-rps verify from the wire formats (include/c12381_ac.h): pk.fixed_part (243 B), pk.Y ((2 nattr + 1) x 49 B), pk.tilde_Y
        ((nattr + 1) x 97 B), the disclosure set idx, PresInfo (389 B each) and the DISCLOSED attributes (nI x 48 B each, in the order of idx);
        there is no message.  One byte per presentation: 1 / 0, or 0xff where the reference would throw.  A used key record that does not
        decode is C12381_E_POINT (every byte 0xff): raised when strict, returned as bytes otherwise.  dev: through the _dev form on device
        copies of the buffers."""
        n, nattr = len(pres389) // 389, len(tY97) // 97 - 1
        arr, nI = self._idx(idx)
        if dev:
            return self._rps_dev(lambda p, o: self.lib.c12381_ac_rps_verify_batch_dev(self.h, n, nattr, nI, arr, *p, *o),
                                 [pk243, Y49, tY97, pres389, attr48 if nI else None], [n], strict)[0]
        out = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_ac_rps_verify_batch(self.h, n, nattr, nI, arr, _p(pk243), _p(Y49), _p(tY97), _p(pres389), _p(attr48) if nI else None,
                                                     _p(out)), allow_point=not strict)
        return out.raw[:n]

    def ac_rps_pres(self, pk243: bytes, Y49: bytes, idx, attr48: bytes, sigs195: bytes, cache97: bytes, usk48: bytes, rnd: bytes, strict: bool = True,
                    dev: bool = False):
        """AC-rps pres from the wire formats: pk.fixed_part, pk.Y, the disclosure set idx, the holder's whole attribute spans (nattr x 48 B each),
        signatures serialize(h, sigma, tilde_M) (195 B each), redact caches (97 B each), user secret keys (48 B each) and the caller's randomness
        (r, t, rho: 3 x 32 B per presentation) -> (n x 389-byte PresInfo, n status bytes: 0, or 0xff — and a record of 0xff — where the reference
        would throw).  A key that does not decode is C12381_E_POINT (every byte 0xff): raised when strict, returned as bytes otherwise.  Not
        constant-time."""
        n, nattr = len(sigs195) // 195, (len(Y49) // 49 - 1) // 2
        arr, nI = self._idx(idx)
        if dev:
            return tuple(self._rps_dev(lambda p, o: self.lib.c12381_ac_rps_pres_batch_dev(self.h, n, nattr, nI, arr, *p, *o),
                                       [pk243, Y49, attr48, sigs195, cache97, usk48, rnd], [389 * n, n], strict))
        pres, st = ctypes.create_string_buffer(max(389 * n, 1)), ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_ac_rps_pres_batch(self.h, n, nattr, nI, arr, _p(pk243), _p(Y49), _p(attr48), _p(sigs195), _p(cache97), _p(usk48), _p(rnd),
                                                   _p(pres), _p(st)), allow_point=not strict)
        return pres.raw[:389 * n], st.raw[:n]

    def ac_rps_redact(self, tY97: bytes, idx, attr48: bytes, sigs195: bytes, strict: bool = True, dev: bool = False):
        """AC-rps redact from the wire formats: pk.tilde_Y ((nattr + 1) x 97 B), the disclosure set idx, the holder's whole attribute spans and
        signatures (195 B each) -> (n x 97-byte RedactCache, n status bytes: 0, or 0xff — and a record of 0xff — where the reference would
        throw).  A used record of pk.tilde_Y that does not decode is C12381_E_POINT (every byte 0xff): raised when strict, returned as bytes
        otherwise.  Not constant-time."""
        n, nattr = len(sigs195) // 195, len(tY97) // 97 - 1
        arr, nI = self._idx(idx)
        if dev:
            return tuple(self._rps_dev(lambda p, o: self.lib.c12381_ac_rps_redact_batch_dev(self.h, n, nattr, nI, arr, *p, *o), [tY97, attr48, sigs195],
                                       [97 * n, n], strict))
        cache, st = ctypes.create_string_buffer(max(97 * n, 1)), ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_ac_rps_redact_batch(self.h, n, nattr, nI, arr, _p(tY97), _p(attr48), _p(sigs195), _p(cache), _p(st)), allow_point=not strict)
        return cache.raw[:97 * n], st.raw[:n]

    def mhac_bbs_verify(self, pp146: bytes, h49: bytes, pk97: bytes, prv, rev, crev49: bytes, fixed242: bytes, z48: bytes, zhp48: bytes, pub48: bytes,
                        strict: bool = True, dev: bool = False) -> bytes:
        """MHAC-bbs verify_pres from the wire formats (include/c12381_mhac.h): pp.g1_g2 (146 B), pp.h (m x 49 B), pk (97 B), the index sets prv (in
        the caller's order) and rev, then per presentation PresType.C_rev (49 B), Pres.fixed_part (242 B), Pres.z (nPrv x 48 B), Pres.z_hid_pub
        (nHidPub x 48 B) and the REVEALED public values (nRevPub x 48 B, ascending Pub position).  One byte per presentation: 1 / 0, or 0xff where
        the reference would throw.  A pp / used h / pk that does not decode is C12381_E_POINT (every byte 0xff): raised when strict, returned as
        bytes otherwise.  dev: through the _dev form on device copies of the buffers."""
        n, m = len(fixed242) // 242, len(h49) // 49
        (pa, nP), (ra, nR) = self._idx(prv), self._idx(rev)
        ins = [pp146, h49, pk97, crev49, fixed242, z48 or None, zhp48 or None, pub48 or None]
        if dev:
            return self._rps_dev(lambda p, o: self.lib.c12381_mhac_bbs_verify_batch_dev(self.h, n, m, nP, pa, nR, ra, *p, *o), ins, [n], strict)[0]
        out = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.c12381_mhac_bbs_verify_batch(self.h, n, m, nP, pa, nR, ra, *(_p(b) for b in ins), _p(out)), allow_point=not strict)
        return out.raw[:n]

    def mhac_bbs_pres(self, pp146: bytes, h49: bytes, prv, rev, t: int, A49: bytes, D49: bytes, lam48: bytes, eshare48: bytes, ashare48: bytes,
                      crev49: bytes, cpub49: bytes, pub48: bytes, rnd: bytes, strict: bool = True, dev: bool = False):
        """MHAC-bbs cred_pres from the wire formats for t parties: per presentation creds.A and group.D (49 B each), group.lambda and the parties'
        e_share (t x 48 B each), their a_share rows (t x nPrv x 48 B, party-major), PresType.C_rev / C_pub (49 B each), the WHOLE public span
        (nPub x 48 B) and the caller's randomness (r, alpha, beta_share, beta_share_j, gamma_share: (2 + (t - 1) nPrv + nHid + t) x 32 B) ->
        (n x 242-byte Pres.fixed_part, n x nPrv x 48-byte Pres.z, n x nHidPub x 48-byte Pres.z_hid_pub, n status bytes: 0, or 0xff — and records
        of 0xff — where the reference would throw).  A pp / used h that does not decode is C12381_E_POINT (every byte 0xff): raised when strict,
        returned as bytes otherwise.  Not constant-time."""
        n, m = len(A49) // 49, len(h49) // 49
        (pa, nP), (ra, nR) = self._idx(prv), self._idx(rev)
        nhp = max(m - nP - nR, 0)
        ins = [pp146, h49, A49, D49, lam48, eshare48, ashare48 or None, crev49, cpub49, pub48 or None, rnd]
        sizes = [242 * n, 48 * nP * n, 48 * nhp * n, n]
        if dev:
            return tuple(self._rps_dev(lambda p, o: self.lib.c12381_mhac_bbs_pres_batch_dev(self.h, n, m, t, nP, pa, nR, ra, *p, *o), ins, sizes, strict))
        outs = [ctypes.create_string_buffer(max(k, 1)) for k in sizes]
        self._ck(self.lib.c12381_mhac_bbs_pres_batch(self.h, n, m, t, nP, pa, nR, ra, *(_p(b) for b in ins), *(_p(o) for o in outs)), allow_point=not strict)
        return tuple(o.raw[:k] for o, k in zip(outs, sizes))

    def _mhac_call(self, name, head, ins, sizes, strict, dev, null_out=()):
        """one MHAC-bbs issuance entry in its host or its _dev form: head = the scalar arguments and index arrays, ins = the input buffers (None: a
        null pointer), sizes = the byte counts of the outputs; null_out: the positions of outputs passed as NULL (returned as b"")"""
        if dev:
            fn = getattr(self.lib, name + "_dev")
            got = self._rps_dev(lambda p, o: fn(self.h, *head, *p, *(None if i in null_out else x for i, x in enumerate(o))), ins, sizes, strict)
            return tuple(b"" if i in null_out else g for i, g in enumerate(got))
        outs = [ctypes.create_string_buffer(max(k, 1)) for k in sizes]
        self._ck(getattr(self.lib, name)(self.h, *head, *(_p(b) for b in ins), *(None if i in null_out else _p(o) for i, o in enumerate(outs))),
                 allow_point=not strict)
        return tuple(b"" if i in null_out else o.raw[:k] for i, (o, k) in enumerate(zip(outs, sizes)))

    def mhac_bbs_attr(self, pp146: bytes, h49: bytes, prv, t: int, nparties: int, rnd: bytes, strict: bool = True, dev: bool = False):
        """MHAC-bbs generate_attributes from the caller's randomness (include/c12381_mhac.h): per credential m + nPrv (t - 1) scalars of 32 B (the
        attributes, then the polynomial coefficients) -> (n x nPub x 48-byte public attributes, n x nparties x nPrv x 48-byte shares party-major,
        n x nparties x 49-byte commitments).  A pp / used h that does not decode is C12381_E_POINT (every byte 0xff): raised when strict."""
        m = len(h49) // 49
        pa, nP = self._idx(prv)
        n = len(rnd) // (32 * (m + nP * (t - 1)))
        return self._mhac_call("c12381_mhac_bbs_attr_batch", (n, m, t, nparties, nP, pa), [pp146, h49, rnd],
                               [48 * (m - nP) * n, 48 * nP * nparties * n, 49 * nparties * n], strict, dev)

    def mhac_bbs_iss(self, pp146: bytes, h49: bytes, sk48: bytes, pub_idx, t: int, nparties: int, C49: bytes, pub48: bytes, rnd: bytes,
                     strict: bool = True, dev: bool = False):
        """MHAC-bbs cred_iss from the wire formats: the issuer's key (48 B), public_indexes in the caller's order, per credential the nparties
        commitments (49 B each), the nPub public values (48 B each) and the randomness (e, then t - 1 coefficients: t x 32 B) -> (n x 49-byte A,
        n x nparties x 48-byte e_share, n x nparties x 49-byte D, n status bytes: 0, or 0xff — and records of 0xff — where the reference would
        throw).  sk >= r is C12381_E_ARG (every byte 0xff), a pp / used h that does not decode C12381_E_POINT.  Not constant-time."""
        m, n = len(h49) // 49, len(rnd) // (32 * t)
        ia, nPub = self._idx(pub_idx)
        return self._mhac_call("c12381_mhac_bbs_iss_batch", (n, m, t, nparties, nPub, ia), [pp146, h49, sk48, C49, pub48 or None, rnd],
                               [49 * n, 48 * nparties * n, 49 * nparties * n, n], strict, dev)

    def mhac_bbs_group(self, S, nparties: int, nPrv: int, D49: bytes, eshare48: bytes | None, ashare48: bytes | None, strict: bool = True,
                       dev: bool = False):
        """MHAC-bbs make_pres_group for the parties S (in the caller's order), with the gather of their rows: per credential the nparties D records,
        and optionally the nparties e_share fields and the nparties x nPrv a_share fields -> (n x t x 48-byte lambda, n x 49-byte D, the rows of S
        of e_share (n x t x 48 B) and of a_share (n x t x nPrv x 48 B) — b"" where the input was None —, n status bytes: 0, or 0xff where a D
        record of S does not decode)."""
        n = len(D49) // (49 * nparties)
        sa, t = self._idx(S)
        null = tuple(i for i, b in ((2, eshare48), (3, ashare48 if nPrv else None)) if b is None)
        return self._mhac_call("c12381_mhac_bbs_group_batch", (n, nparties, t, sa, nPrv), [D49, eshare48, ashare48 if nPrv else None],
                               [48 * t * n, 49 * n, 48 * t * n, 48 * t * nPrv * n, n], strict, dev, null)

    def mhac_bbs_type(self, pp146: bytes, h49: bytes, prv, rev, pub48: bytes, n: int | None = None, strict: bool = True, dev: bool = False):
        """MHAC-bbs make_pres_type from the wire formats: the index sets of verify and pres and per presentation the WHOLE public span (nPub x 48 B)
        -> (n x 49-byte C_rev, n x 49-byte C_pub, n status bytes: 0, or 0xff — and records of 0xff — where a public value is >= r).  n: the
        number of presentations, taken from pub48 when not given (nPub = 0 needs it)."""
        m = len(h49) // 49
        (pa, nP), (ra, nR) = self._idx(prv), self._idx(rev)
        n = len(pub48) // (48 * (m - nP)) if n is None else n
        return self._mhac_call("c12381_mhac_bbs_type_batch", (n, m, nP, pa, nR, ra), [pp146, h49, pub48 or None], [49 * n, 49 * n, n], strict, dev)

    def ac_bbs_issue(self, sk48: bytes, pk243: bytes, Y49: bytes, attr48: bytes, rnd32: bytes, strict: bool = True, dev: bool = False):
        """AC-bbs issue from the wire formats (include/c12381_ac_issue.h): the issuer's key serialize(x) (48 B), pk.fixed_part (243 B), pk.Y (nattr x
        49 B), the holders' whole attribute spans (nattr x 48 B each) and the caller's randomness (w: 32 B per credential) -> (n x 97-byte
        Signature serialize(A, w), n status bytes: 0, or 0xff — and a record of 0xff — where an attribute is >= r).  x >= r is C12381_E_ARG, a
        key that does not decode C12381_E_POINT (every byte 0xff): the latter raised when strict, returned as bytes otherwise.  Not constant-time."""
        n, nattr = len(rnd32) // 32, len(Y49) // 49
        return self._mhac_call("c12381_ac_bbs_issue_batch", (n, nattr), [sk48, pk243, Y49, attr48, rnd32], [97 * n, n], strict, dev)

    def ac_rbbs_issue(self, sk96: bytes, pk243: bytes, Y49: bytes, attr48: bytes, rnd32: bytes, strict: bool = True, dev: bool = False):
        """AC-rbbs issue: as ac_bbs_issue with the key serialize(x, y) (96 B, both fields range-checked) and the 2 nattr records of pk.Y, of
        which the first nattr are read."""
        n, nattr = len(rnd32) // 32, len(Y49) // 49 // 2
        return self._mhac_call("c12381_ac_rbbs_issue_batch", (n, nattr), [sk96, pk243, Y49, attr48, rnd32], [97 * n, n], strict, dev)

    def ac_rps_user_keygen(self, pk243: bytes, rnd32: bytes, strict: bool = True, dev: bool = False):
        """AC-rps user_keygen: pk.fixed_part (243 B) and the caller's randomness (usk: 32 B per key pair, reduced mod r) -> (n x 48-byte
        UserSecretKey, n x 49-byte UserPublicKey g^usk).  A pk that does not decode is C12381_E_POINT (every byte 0xff): raised when strict,
        returned as bytes otherwise.  Not constant-time."""
        n = len(rnd32) // 32
        return self._mhac_call("c12381_ac_rps_user_keygen_batch", (n,), [pk243, rnd32], [48 * n, 49 * n], strict, dev)

    def ac_rps_issue(self, sk96: bytes, pk243: bytes, tY97: bytes, upk49: bytes, attr48: bytes, rnd32: bytes, strict: bool = True, dev: bool = False):
        """AC-rps issue from the wire formats: the issuer's key serialize(x, y) (96 B), pk.fixed_part, pk.tilde_Y ((nattr + 1) x 97 B), one
        UserPublicKey per credential (49 B each), the holders' whole attribute spans and the caller's randomness (alpha: 32 B per credential)
        -> (n x 195-byte Signature serialize(h, sigma, tilde_M), n status bytes: 0, or 0xff — and a record of 0xff — where an attribute is >= r
        or upk does not decode).  x or y >= r is C12381_E_ARG, a key that does not decode C12381_E_POINT (every byte 0xff): the latter raised
        when strict, returned as bytes otherwise.  Not constant-time."""
        n, nattr = len(rnd32) // 32, len(tY97) // 97 - 1
        return self._mhac_call("c12381_ac_rps_issue_batch", (n, nattr), [sk96, pk243, tY97, upk49, attr48, rnd32], [195 * n, n], strict, dev)

    def _rps_dev(self, call, ins, out_sizes, strict):
        """the _dev form of an AC-rps entry on device copies of `ins` (bytes, or None for a null pointer): call(input pointers, output pointers), sync,
        the outputs as bytes.  The outputs start as 0x07 bytes, so a byte the entry does not write shows."""
        import torch
        dev = [None if b is None else torch.frombuffer(bytearray(b) or bytearray(1), dtype=torch.uint8).to("cuda") for b in ins]
        outs = [torch.full((max(k, 1),), 7, dtype=torch.uint8, device="cuda") for k in out_sizes]
        torch.cuda.synchronize()
        self._ck(call([None if t is None else _p(t.data_ptr()) for t in dev], [_p(t.data_ptr()) for t in outs]))
        rc = self.lib.c12381_sync(self.h)
        got = [bytes(t.cpu().numpy().tobytes())[:k] for t, k in zip(outs, out_sizes)]
        self._ck(rc, allow_point=not strict)
        return got

    # ---- device-pointer entry points (ints = device addresses, e.g. torch tensor.data_ptr())
    def bbs_plus_sign(self, g1, h0, h, gamma32, x, r, m) -> bytes:
        n = len(x) // 32
        nmsg = len(h) // 96
        out = ctypes.create_string_buffer(max(96 * n, 1))
        self._ck(self.lib.c12381_bbs_plus_sign_batch(self.h, n, nmsg, _p(g1), _p(h0), _p(h), _p(gamma32), _p(x), _p(r), _p(m), _p(out)))
        return out.raw[:96 * n]

    def miller_dev(self, n, g1_ptr, g2_ptr, out_ptr):
        self._ck(self.lib.c12381_miller_batch_dev(self.h, n, _p(g1_ptr), _p(g2_ptr), _p(out_ptr)))

    def gt_op_dev(self, op, n, a_ptr, b_ptr, out_ptr):
        self._ck(self.lib.c12381_gt_op_batch_dev(self.h, self.GT_OPS[op], n, _p(a_ptr), _p(b_ptr), _p(out_ptr)))

    def gt_is_unity_dev(self, n, a_ptr, out_ptr):
        self._ck(self.lib.c12381_gt_is_unity_batch_dev(self.h, n, _p(a_ptr), _p(out_ptr)))

    def g1_decompress_dev(self, n, in_ptr, out_ptr, status_ptr):
        self._ck(self.lib.c12381_g1_decompress_batch_dev(self.h, n, _p(in_ptr), _p(out_ptr), _p(status_ptr)))

    def g2_decompress_dev(self, n, in_ptr, out_ptr, status_ptr):
        self._ck(self.lib.c12381_g2_decompress_batch_dev(self.h, n, _p(in_ptr), _p(out_ptr), _p(status_ptr)))

    def bbs_plus_verify_wire_dev(self, n, nh, msg_len, pub_ptr, h_ptr, pk_ptr, sig_ptr, msg_ptr, ok_ptr):
        self._ck(self.lib.c12381_bbs_plus_verify_wire_batch_dev(self.h, n, nh, msg_len, _p(pub_ptr), _p(h_ptr), _p(pk_ptr), _p(sig_ptr), _p(msg_ptr), _p(ok_ptr)))

    def g1_from_hash_dev(self, n, digests_ptr, out_ptr, fmt=96):
        self._ck(self.lib.c12381_g1_from_hash_batch_dev(self.h, n, _p(digests_ptr), _p(out_ptr), fmt))

    def zp_op_dev(self, op, n, a_ptr, b_ptr, out_ptr):
        self._ck(self.lib.c12381_zp_op_batch_dev(self.h, self.ZP_OPS[op], n, _p(a_ptr), _p(b_ptr), _p(out_ptr)))

    def zp_inner_product_dev(self, n, a_ptr, b_ptr, out_ptr):
        self._ck(self.lib.c12381_zp_inner_product_dev(self.h, n, _p(a_ptr), _p(b_ptr), _p(out_ptr)))

    def g2_mul_dev(self, n, pts_ptr, sc_ptr, out_ptr, fmt=97):
        self._ck(self.lib.c12381_g2_mul_batch_dev(self.h, n, _p(pts_ptr), _p(sc_ptr), _p(out_ptr), fmt))

    def pair_dev(self, n, g1_ptr, g2_ptr, gt_ptr):
        self._ck(self.lib.c12381_pair_batch_dev(self.h, n, _p(g1_ptr), _p(g2_ptr), _p(gt_ptr)))

    def pair_eq_dev(self, n, a1, a2, b1, b2, ok_ptr):
        self._ck(self.lib.c12381_pair_eq_batch_dev(self.h, n, _p(a1), _p(a2), _p(b1), _p(b2), _p(ok_ptr)))

    def fp_mulchain_dev(self, n, iters, a_ptr, b_ptr, out_ptr):
        self._ck(self.lib.c12381_fp_mulchain_dev(self.h, n, iters, _p(a_ptr), _p(b_ptr), _p(out_ptr)))

    def fp_op_dev(self, op, n, a_ptr, b_ptr, out_ptr):
        self._ck(self.lib.c12381_fp_op_batch_dev(self.h, self.FP_OPS[op], n, _p(a_ptr), _p(b_ptr), _p(out_ptr)))

    def exp_fp_raw(self, op: int, n: int, arity: int, outputs: int, limbs: bytes, k: bytes) -> bytes:
        """Experiments library only: the raw-limb test kernel (n x arity x 14 int32 in, n x 4 int32 multipliers, n x outputs x 14 int32 out)."""
        if not hasattr(self.lib, "c12381_exp_fp_raw_batch"):
            raise RuntimeError("c12381_exp_fp_raw_batch: only the experiments library exports the raw-limb test entry")
        out = ctypes.create_string_buffer(max(56 * outputs * n, 1))
        self._ck(self.lib.c12381_exp_fp_raw_batch(self.h, op, n, arity, outputs, _p(limbs), _p(k), _p(out)))
        return out.raw[:56 * outputs * n]

    def g1_mul_dev(self, n, pts_ptr, sc_ptr, out_ptr, fmt=49):
        self._ck(self.lib.c12381_g1_mul_batch_dev(self.h, n, _p(pts_ptr), _p(sc_ptr), _p(out_ptr), fmt))

    def g1_msm_dev(self, n, pts_ptr, sc_ptr, out_ptr, fmt=49):
        self._ck(self.lib.c12381_g1_msm_dev(self.h, n, _p(pts_ptr), _p(sc_ptr), _p(out_ptr), fmt))


def g1_msm_multi(contexts, pts: bytes, scalars: bytes, fmt: int = 49) -> bytes:
    """c12381_g1_msm_multi: one host process, one Context per GPU."""
    lib = contexts[0].lib
    n = len(pts) // 96
    arr = (ctypes.c_void_p * len(contexts))(*[c.h for c in contexts])
    out = ctypes.create_string_buffer(fmt)
    rc = lib.c12381_g1_msm_multi(arr, len(contexts), n, _p(pts), _p(scalars), _p(out), fmt)
    if rc != 0:
        raise C12381Error(rc, "c12381_g1_msm_multi")
    return out.raw[:fmt]
