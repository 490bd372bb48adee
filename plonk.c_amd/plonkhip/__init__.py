"""Python plumbing over libplonkhip.so -- the C ABI declared in include/plonkhip.h.

The product boundary is the C ABI (and the drop-in C headers in include/ that the
reference's plonk.h compiles against).  This module only loads that library with ctypes
for the tests, bench.py and the multi-GPU driver; it never computes anything itself and
there is no fallback: if libplonkhip.so is missing or no GPU is usable, every call raises.

Host-buffer functions mirror the reference hot path (src/srs.h:53-68, src/poly.h:106-122):
    msm_g1(points, scalars) -> 3 bytes {x, y, infinite}        (srs_eval_at_s)
    poly_mul(a, b)          -> trimmed coefficient bytes         (poly_mul)
    srs_eval_at_s(g1s, coeffs) -- with the reference's degree check
Device functions take torch CUDA tensors (or raw ints) and an optional stream.
"""
import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("PLK_LIB") or os.path.join(PKG_DIR, "libplonkhip.so")   # PLK_LIB: tuning builds only
HEADER_PATH = os.path.join(REPO_DIR, "include", "plonkhip.h")

PLK_OK, PLK_ERR_HIP, PLK_ERR_ARG, PLK_ERR_RANGE, PLK_ERR_NODEV, PLK_ERR_NOMEM = range(6)
MSM_RESULT_BYTES = 2176
MSM_LOG_OFFSET, MSM_IRREGULAR_OFFSET, MSM_G1_OFFSET = 8, 12, 16

_u8p = C.POINTER(C.c_uint8)
_vp = C.c_void_p
_sz = C.c_size_t

# every exported entry point with its ctypes signature (restype, argtypes)
SIGNATURES = {
    "plk_init": (C.c_int, [C.c_int]),
    "plk_shutdown": (None, []),
    "plk_last_error": (C.c_char_p, []),
    "plk_device_count": (C.c_int, []),
    "plk_version": (C.c_char_p, []),
    "plk_msm_g1": (C.c_int, [_u8p, _u8p, _sz, _u8p]),
    "plk_poly_mul": (C.c_int, [_u8p, _sz, _u8p, _sz, _u8p, C.POINTER(_sz)]),
    "plk_msm_result_init": (C.c_int, [_vp, _vp]),
    "plk_msm_g1_dev": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    "plk_msm_g1_batch_dev": (C.c_int, [_vp, _sz, _vp, _sz, _sz, C.c_int, _vp, _vp]),
    "plk_msm_plan": (C.c_int, [_sz, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "plk_msm_g1_serial_dev": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    "plk_msm_combine_dev": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "plk_msm_finalize_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "plk_dlog_generator": (C.c_int, [_u8p]),
    "plk_msm_g1_segments_plan": (C.c_int, [_sz, _sz, _sz, C.c_int, C.POINTER(C.c_int64)]),
    "plk_msm_g1_segments_workspace": (_sz, [_sz, _sz, _sz, C.c_int]),
    "plk_msm_g1_segments_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp]),
    "plk_msm_g1_segments": (C.c_int, [_u8p, _u8p, _sz, C.POINTER(C.c_uint32), _sz, _sz, _u8p]),
    "plk_poly_mul_workspace": (_sz, [_sz, _sz]),
    "plk_poly_mul_dev": (C.c_int, [_vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp]),
    "plk_poly_mul_batch_workspace": (_sz, [_vp, C.c_int]),
    "plk_poly_mul_batch_dev": (C.c_int, [_vp, C.c_int, _vp, _sz, _vp]),
    "plk_ntt_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "plk_ntt_batch_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp]),
    "plk_ntt29_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "plk_ntt29_batch_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp]),
    "plk_poly_eval": (C.c_int, [_u8p, _sz, C.c_uint8, _u8p]),
    "plk_poly_eval_batch": (C.c_int, [C.POINTER(_u8p), C.POINTER(_sz), _u8p, C.c_int, _u8p]),
    "plk_poly_eval_workspace": (_sz, [C.c_int]),
    "plk_poly_eval_batch_dev": (C.c_int, [C.POINTER(_vp), C.POINTER(_sz), _u8p, C.c_int, _vp, _vp, _vp]),
    "plk_poly_divide": (C.c_int, [_u8p, _sz, _u8p, _sz, _u8p, C.POINTER(_sz), _u8p, C.POINTER(_sz)]),
    "plk_poly_divide_workspace": (_sz, [_sz, _sz]),
    "plk_poly_divide_path": (C.c_int, [_u8p, _sz, _sz]),
    "plk_poly_divide_dev": (C.c_int, [_vp, _sz, _u8p, _sz, _vp, _vp, _vp, _vp, _vp]),
    "plk_matrix_mul": (C.c_int, [_u8p, _sz, _sz, _u8p, _sz, _u8p]),
    "plk_matrix_inv": (C.c_int, [_u8p, _sz, _u8p]),
    "plk_interpolate": (C.c_int, [_u8p, _u8p, _sz, _u8p, C.POINTER(_sz)]),
    "plk_prover_create": (C.c_int, [_vp, C.POINTER(_vp)]),
    "plk_prover_destroy": (None, [_vp]),
    "plk_prover_device_bytes": (_sz, [_vp]),
    "plk_prover_prove": (C.c_int, [_vp, _vp, _u8p, _u8p, _u8p]),
    "plk_prover_rounds_dev": (C.c_int, [_vp, C.POINTER(_vp), _u8p, _u8p, C.c_int, _u8p]),
    "plk_prover_profile_dev": (C.c_int, [_vp, C.POINTER(_vp), _u8p, _u8p, C.c_int, _u8p, C.POINTER(C.c_double)]),
    "plk_prover_launches": (C.c_int, [_vp, C.POINTER(_vp), _u8p, _u8p, C.c_int, C.POINTER(C.c_int),
                                      C.POINTER(C.c_int)]),
    "plk_prove_exit_message": (C.c_int, [C.c_uint32, C.c_char_p, _sz]),
    "plk_prover_batch_path": (C.c_int, [_vp, C.c_int]),
    "plk_prover_prove_batch": (C.c_int, [_vp, _u8p, _u8p, _u8p, C.c_int, _u8p, C.POINTER(C.c_uint32)]),
    "plk_prover_rounds_batch": (C.c_int, [_vp, _u8p, _u8p, _u8p, C.c_int, C.c_int, _u8p, C.POINTER(C.c_uint32)]),
    "plk_prover_prove_batch_dev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp]),
    "plk_prover_rounds_batch_dev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "plk_prover_alg_bytes": (C.c_uint64, [_vp]),
    "plk_prover_preprocess": (C.c_int, [_vp, C.POINTER(_vp)]),
    "plk_prover_chain_bytes": (_sz, [_vp, C.c_int]),
    "plk_prover_chains_dev": (C.c_int, [_vp, C.POINTER(_vp), _u8p, _u8p, C.c_int, _vp, _vp, _vp]),
    "plk_prover_rounds_ext_dev": (C.c_int, [_vp, C.POINTER(_vp), _u8p, _u8p, C.c_int, C.c_int, _vp, _vp, _vp,
                                            _u8p]),
    "plk_set_option": (C.c_int, [C.c_int, C.c_int64]),
    "plk_init_devices": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "plk_devices": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "plk_get_option": (C.c_int64, [C.c_int]),
    "plk_prover_attach_helpers": (C.c_int, [_vp, C.c_int]),
    "plk_prover_helpers": (C.c_int, [_vp]),
    "plk_prover_rounds_multi_dev": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, _u8p, _u8p, C.c_int, _u8p]),
    "plk_ntt_launch_log": (C.c_int, [C.POINTER(C.c_int32), C.c_int]),
    "plk_srs_create": (C.c_int, [_u8p, _sz, C.POINTER(_vp)]),
    "plk_srs_destroy": (None, [_vp]),
    "plk_srs_len": (_sz, [_vp]),
    "plk_srs_irregular": (C.c_int, [_vp]),
    "plk_kzg_commit_batch": (C.c_int, [_vp, C.POINTER(_u8p), C.POINTER(_sz), C.c_int, _u8p]),
    "plk_kzg_open_batch": (C.c_int, [_vp, C.POINTER(_u8p), C.POINTER(_sz), _u8p, C.c_int, _u8p, _u8p]),
    "plk_kzg_workspace": (_sz, [C.POINTER(_sz), C.c_int]),
    "plk_kzg_commit_batch_dev": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_sz), C.c_int, _vp, _vp]),
    "plk_kzg_open_batch_dev": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_sz), _u8p, C.c_int, _vp, _vp,
                                         C.POINTER(_vp), _vp, _vp]),
    "plk_pairing_batch": (C.c_int, [_u8p, _u8p, _sz, _u8p]),
    "plk_pairing_batch_dev": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    "plk_kzg_verify_batch": (C.c_int, [_vp, _u8p, _u8p, _u8p, _u8p, _sz, _u8p]),
    "plk_kzg_verify_batch_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "plk_kzg_fold_workspace": (_sz, [C.POINTER(_sz), C.POINTER(C.c_int), C.c_int]),
    "plk_kzg_open_fold_batch": (C.c_int, [_vp, C.POINTER(_u8p), C.POINTER(_sz), _u8p, C.POINTER(C.c_int), _u8p,
                                          C.c_int, _u8p, _u8p]),
    "plk_kzg_open_fold_batch_dev": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_sz), _u8p, C.POINTER(C.c_int), _u8p,
                                              C.c_int, _vp, _vp, C.POINTER(_vp), _vp, _vp]),
    "plk_kzg_verify_fold_batch": (C.c_int, [_vp, C.c_int, _u8p, _u8p, _u8p, _u8p, _u8p, _sz, _u8p]),
    "plk_kzg_verify_fold_batch_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "plk_kzg_multi_coeffs": (C.c_int, [C.POINTER(C.c_uint32), _u8p, C.c_int, C.c_uint8, _u8p]),
    "plk_kzg_multi_workspace": (_sz, [C.POINTER(_sz), C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.c_int]),
    "plk_kzg_open_multi_batch": (C.c_int, [_vp, C.POINTER(_u8p), C.POINTER(_sz), C.POINTER(C.c_uint32), _u8p,
                                           C.POINTER(C.c_int), _u8p, C.c_int, _u8p, _u8p]),
    "plk_kzg_open_multi_batch_dev": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_sz), C.POINTER(C.c_uint32), _u8p,
                                               C.POINTER(C.c_int), _u8p, C.c_int, _vp, _vp, C.POINTER(_vp), _vp, _vp]),
    "plk_kzg_verify_multi_batch": (C.c_int, [_vp, C.c_int, _u8p, C.POINTER(C.c_uint32), _u8p, _u8p, _u8p, _u8p, _sz,
                                             _u8p]),
    "plk_kzg_verify_multi_batch_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "plk_kzg_verify_agg_plan": (C.c_int, [_sz, _sz, C.POINTER(C.c_int64)]),
    "plk_kzg_verify_agg_workspace": (_sz, [_sz, _sz]),
    "plk_kzg_verify_agg_batch": (C.c_int, [_vp, _sz, _u8p, _u8p, _u8p, _u8p, _u8p, _sz, _u8p]),
    "plk_kzg_verify_agg_batch_dev": (C.c_int, [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "plk_kzg_points_count": (_sz, [C.POINTER(C.c_uint32), C.c_int]),
    "plk_kzg_points_workspace": (_sz, [C.POINTER(_sz), C.POINTER(C.c_uint32), C.c_int]),
    "plk_kzg_open_points_batch": (C.c_int, [_vp, C.POINTER(_u8p), C.POINTER(_sz), C.POINTER(C.c_uint32), C.c_int,
                                            _u8p, _u8p, _u8p]),
    "plk_kzg_open_points_batch_dev": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_sz), C.POINTER(C.c_uint32), C.c_int,
                                                _vp, _vp, _vp, _vp, _vp, _vp]),
    "plk_kzg_flat_plan": (C.c_int, [_sz, _sz, C.c_int, C.POINTER(C.c_int64)]),
    "plk_kzg_commit_flat_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp]),
    "plk_kzg_open_flat_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "plk_kzg_commit_flat": (C.c_int, [_vp, _u8p, _sz, C.POINTER(C.c_uint32), _sz, _sz, _u8p]),
    "plk_kzg_open_flat": (C.c_int, [_vp, _u8p, _sz, C.POINTER(C.c_uint32), _sz, _sz, _u8p, _u8p, _u8p, _u8p]),
    "plk_kzg_fold_flat_plan": (C.c_int, [_sz, _sz, _sz, C.c_int, C.POINTER(C.c_int64)]),
    "plk_kzg_open_fold_flat_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "plk_kzg_open_fold_flat": (C.c_int, [_vp, _u8p, _sz, C.POINTER(C.c_uint32), _sz, _sz, _sz, _u8p, _u8p, _u8p, _u8p,
                                         _u8p]),
    "plk_kzg_multi_flat_plan": (C.c_int, [_sz, _sz, _sz, C.c_int, C.POINTER(C.c_int64)]),
    "plk_kzg_open_multi_flat_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "plk_kzg_open_multi_flat": (C.c_int, [_vp, _u8p, _sz, C.POINTER(C.c_uint32), _sz, _sz, _sz, C.POINTER(C.c_uint32), _u8p,
                                          _u8p, _u8p, _u8p, _u8p]),
    "plk_poly_lincomb_len": (_sz, [_vp]),
    "plk_poly_lincomb": (C.c_int, [_vp, C.POINTER(_sz)]),
    "plk_poly_lincomb_batch_dev": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "plk_poly_divide_short_workspace": (_sz, [_vp, C.c_int]),
    "plk_poly_divide_short_plan": (C.c_int, [_sz, _sz, C.POINTER(C.c_int)]),
    "plk_poly_divide_short_batch_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    "plk_poly_divide_short_batch": (C.c_int, [_vp, C.c_int, C.POINTER(_sz), C.POINTER(_sz)]),
    "plk_poly_from_roots": (C.c_int, [_u8p, C.c_int, _u8p]),
    "plk_poly_mul_short_plan": (C.c_int, [_sz, _sz, _sz, C.POINTER(C.c_int64)]),
    "plk_poly_mul_short_batch_dev": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "plk_poly_mul_short_batch": (C.c_int, [_vp, C.c_int, C.POINTER(_sz)]),
}

# PLK_OPT_* (include/plonkhip.h), by the name without the prefix
OPTIONS = {"TINY_CALLS": 1, "PROVE_SYNC": 2, "POLY_BLOCK_L": 3, "POLY_BLOCK_S": 4, "NTT_F29": 5, "NTT_SHARE": 6,
           "NTT_SHARED_FIX": 7, "NTT_T13_MIN_K": 8, "NTT_CENTER_BLOCKS": 9, "MSM_THREADS": 10,
           "MSM_MAX_BLOCKS": 11, "MSM_GROUPS": 12, "MSM_COPIES": 13, "MSM_HALF": 14, "MSM_SHARD_MIN": 15,
           "NTT_CENTER_SUM": 16, "MSM_HOST_LANES": 17,
           "PROVE_DERIVE_T2A": 18, "NTT_TABLE_SHARE": 19, "NTT_LAUNCH_LOG": 20,
           "PROVE_SRS_LOGS": 22, "PROVE_PACK_FUSE": 23, "PROVE_EARLY_COMMITS": 24,
           "PROVE_HELPER_COPY": 25,   # (21, 26, 27: retired)
           "DROPIN_HOST_WORK": 28, "DIVIDE_FAST_MIN": 29}

PLK_PROVE_STRICT = 1
PLK_PROVE_PREPROCESSED = 2
PLK_CHAIN_T2 = 1   # t_2 = (A2 B2)(C2 z_x), src/plonk.h:432-434
PLK_CHAIN_T3 = 2   # t_3 = (A3 B3)(C3 z_x(omega x)), src/plonk.h:471-473


class PlonkDesc(C.Structure):
    """plk_plonk_desc_t"""
    _fields_ = [("n", _sz), ("h", _u8p), ("k1_h", _u8p), ("k2_h", _u8p), ("h_pows_inv", _u8p),
                ("z_h", _u8p), ("z_h_len", _sz), ("srs_g1", _u8p), ("srs_len", _sz)]


class Circuit(C.Structure):
    """plk_circuit_t"""
    _fields_ = [(k, _u8p) for k in ("q_m", "q_l", "q_r", "q_o", "q_c", "copy_a", "copy_b",
                                    "copy_c", "a", "b", "c")]


class PlonkHipError(RuntimeError):
    def __init__(self, fn, code, msg):
        super().__init__("%s failed (code %d): %s" % (fn, code, msg))
        self.code = code


_lib = None


def lib():
    """Load libplonkhip.so (raises if it was never built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError("libplonkhip.so not built (run `make -C plonk.c_amd` or "
                                    "__graft_entry__.build()): %s" % LIB_PATH)
        # torch-ROCm ships its own libamdhip64 (soname libamdhip64.so.7) and asks for it by a
        # different file name, so loading ours first would put TWO HIP runtimes in the
        # process.  Load torch first: our NEEDED libamdhip64.so.7 then binds to torch's copy
        # and the process has one runtime, one device context, shared streams.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def last_error():
    return lib().plk_last_error().decode(errors="replace")


def _check(fn, rc):
    if rc != PLK_OK:
        raise PlonkHipError(fn, rc, last_error())


def _u8(a):
    return np.ascontiguousarray(np.frombuffer(a, np.uint8) if isinstance(a, (bytes, bytearray))
                                else np.asarray(a, dtype=np.uint8))


def _p(a):
    return a.ctypes.data_as(_u8p)


def init(device=-1):
    _check("plk_init", lib().plk_init(int(device)))


def init_devices(ids):
    """plk_init_devices: ids[0] is the primary device; plk_msm_g1 point-range shards over the
    list (repeats allowed: several shards on one GPU)"""
    ids = [int(i) for i in ids]
    arr = (C.c_int * max(1, len(ids)))(*ids)
    _check("plk_init_devices", lib().plk_init_devices(arr, len(ids)))


def devices():
    arr = (C.c_int * 16)()
    n = int(lib().plk_devices(arr, 16))
    return [arr[i] for i in range(min(n, 16))]


def ntt_launch_log(cap=4096):
    """plk_ntt_launch_log: the recorded NTT pass launches (PLK_OPT_NTT_LAUNCH_LOG = 1) as dicts, log cleared"""
    buf = (C.c_int32 * (8 * cap))()
    n = int(lib().plk_ntt_launch_log(buf, cap))
    keys = ("kind", "tb", "m", "k", "n", "per_block", "units", "field")
    return [dict(zip(keys, buf[8 * i:8 * i + 8])) for i in range(n)]


def _opt_id(name):
    return OPTIONS[name.upper()] if isinstance(name, str) else int(name)


def set_option(name, value):
    """plk_set_option: name = "NTT_F29", ... (PLK_OPT_ without the prefix) or the number"""
    _check("plk_set_option", lib().plk_set_option(_opt_id(name), int(value)))


def get_option(name):
    return int(lib().plk_get_option(_opt_id(name)))


class options:
    """with options(NTT_F29=0, ...): set for the block, the previous values restored after"""

    def __init__(self, **kw):
        self.kw = kw
        self.old = {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = get_option(k)
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            set_option(k, v)
        return False


def tune_from_env():
    """bench / tools only (never called by the library or the tests' product path): apply
    $PLK_TUNE = "NAME=value,NAME=value" through plk_set_option, for A/B runs of one build.
    Returns the dict applied."""
    spec = os.environ.get("PLK_TUNE", "")
    done = {}
    for item in filter(None, (t.strip() for t in spec.split(","))):
        k, v = item.split("=")
        set_option(k.strip(), int(v))
        done[k.strip().upper()] = int(v)
    return done


def device_count():
    return int(lib().plk_device_count())


def dlog_generator():
    out = np.zeros(3, np.uint8)
    _check("plk_dlog_generator", lib().plk_dlog_generator(_p(out)))
    return bytes(out)


# ---------------------------------------------------------------- host-buffer entry points
def msm_g1(points, scalars):
    """sum_i scalars[i] * points[i] as the reference's serial fold would return it."""
    pts = _u8(points).reshape(-1)
    sc = _u8(scalars).reshape(-1)
    if pts.size != 3 * sc.size:
        raise ValueError("points must be n x 3 bytes for n scalars")
    out = np.zeros(3, np.uint8)
    _check("plk_msm_g1", lib().plk_msm_g1(_p(pts), _p(sc), sc.size, _p(out)))
    return bytes(out)


def srs_eval_at_s(g1s, coeffs):
    """srs_eval_at_s(srs, vs) (src/srs.h:53-68): the reference exits when the polynomial is
    longer than the SRS; this mirror raises ValueError instead of exiting the interpreter."""
    pts = _u8(g1s).reshape(-1)
    sc = _u8(coeffs).reshape(-1)
    if sc.size > pts.size // 3:
        raise ValueError("Poynomial degree exceeds SRS size: POLY degree: %d, SRS supports up "
                         "to degree: %d" % (sc.size, sc.size))
    return msm_g1(pts[:3 * sc.size], sc)


def poly_mul(a, b):
    """GF(17) product, trimmed exactly like the reference's poly_new."""
    a = _u8(a).reshape(-1)
    b = _u8(b).reshape(-1)
    rl = max(a.size + b.size - 1, 1)
    out = np.zeros(rl, np.uint8)
    n = _sz(0)
    _check("plk_poly_mul", lib().plk_poly_mul(_p(a), a.size, _p(b), b.size, _p(out), C.byref(n)))
    return bytes(out[:n.value])


def poly_eval(p, x):
    """Horner at x exactly as src/poly.h:265-272 (raw HF bytes included)."""
    p = _u8(p).reshape(-1)
    y = np.zeros(1, np.uint8)
    _check("plk_poly_eval", lib().plk_poly_eval(_p(p), p.size, int(x) & 0xFF, _p(y)))
    return int(y[0])


def poly_eval_batch(polys, xs):
    arrs = [_u8(p).reshape(-1) for p in polys]
    n = len(arrs)
    ptrs = (_u8p * n)(*[_p(a) for a in arrs])
    lens = (_sz * n)(*[a.size for a in arrs])
    xa = _u8(xs).reshape(-1)
    ys = np.zeros(n, np.uint8)
    _check("plk_poly_eval_batch", lib().plk_poly_eval_batch(ptrs, lens, _p(xa), n, _p(ys)))
    return [int(v) for v in ys]


def poly_divide(num, den):
    """(quot, rem) bytes, trimmed as src/poly.h:124-177 returns them."""
    num = _u8(num).reshape(-1)
    den = _u8(den).reshape(-1)
    q = np.zeros(max(num.size, 1), np.uint8)
    r = np.zeros(max(num.size, 1), np.uint8)
    ql, rl = _sz(0), _sz(0)
    _check("plk_poly_divide", lib().plk_poly_divide(_p(num), num.size, _p(den), den.size, _p(q), C.byref(ql),
                                                    _p(r), C.byref(rl)))
    return bytes(q[:ql.value]), bytes(r[:rl.value])


def matrix_mul(a, m, k, b, n):
    a = _u8(a).reshape(-1)
    b = _u8(b).reshape(-1)
    out = np.zeros(max(m * n, 1), np.uint8)
    _check("plk_matrix_mul", lib().plk_matrix_mul(_p(a), m, k, _p(b), n, _p(out)))
    return bytes(out[:m * n])


def matrix_inv(mat, n):
    mat = _u8(mat).reshape(-1)
    out = np.zeros(max(n * n, 1), np.uint8)
    _check("plk_matrix_inv", lib().plk_matrix_inv(_p(mat), n, _p(out)))
    return bytes(out[:n * n])


def interpolate(h_pows_inv, values):
    v = _u8(values).reshape(-1)
    m = _u8(h_pows_inv).reshape(-1)
    out = np.zeros(max(v.size, 1), np.uint8)
    ol = _sz(0)
    _check("plk_interpolate", lib().plk_interpolate(_p(m), _p(v), v.size, _p(out), C.byref(ol)))
    return bytes(out[:ol.value])


# ---------------------------------------------------------------- device entry points
def _ptr(t):
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


def _stream(s):
    if s is None:
        return None
    if isinstance(s, int):
        return s
    return s.cuda_stream


def msm_result_init(res, stream=None):
    _check("plk_msm_result_init", lib().plk_msm_result_init(_ptr(res), _stream(stream)))


def msm_g1_dev(points, scalars, n, res, stream=None):
    _check("plk_msm_g1_dev", lib().plk_msm_g1_dev(_ptr(points), _ptr(scalars), int(n), _ptr(res),
                                                  _stream(stream)))


def msm_g1_batch_dev(points, points_stride, scalars, scalars_stride, n, batch, res, stream=None):
    _check("plk_msm_g1_batch_dev", lib().plk_msm_g1_batch_dev(
        _ptr(points), int(points_stride), _ptr(scalars), int(scalars_stride), int(n), int(batch),
        _ptr(res), _stream(stream)))


def msm_plan(n, batch, aligned=True):
    """plk_msm_plan: the launch plan of msm_g1_dev (batch = 1) / msm_g1_batch_dev for batch MSMs of n
    points under the current options (aligned=False: the byte-wise form).  No device needed."""
    out = (C.c_int * 5)()
    _check("plk_msm_plan", lib().plk_msm_plan(int(n), int(batch), 1 if aligned else 0, out))
    return dict(zip(("threads", "blocks", "groups", "copies", "half"), list(out)))


def msm_g1_serial_dev(points, scalars, n, res, stream=None):
    _check("plk_msm_g1_serial_dev", lib().plk_msm_g1_serial_dev(_ptr(points), _ptr(scalars), int(n),
                                                                _ptr(res), _stream(stream)))


def msm_combine_dev(logs, count, out3, stream=None):
    _check("plk_msm_combine_dev", lib().plk_msm_combine_dev(_ptr(logs), int(count), _ptr(out3),
                                                            _stream(stream)))


def msm_finalize_dev(logs, batch, stride, out4, stream=None):
    _check("plk_msm_finalize_dev", lib().plk_msm_finalize_dev(_ptr(logs), int(batch), int(stride),
                                                              _ptr(out4), _stream(stream)))


def poly_mul_workspace(la, lb):
    return int(lib().plk_poly_mul_workspace(int(la), int(lb)))


def poly_mul_dev(a, la, b, lb, out, nz, work, stream=None):
    _check("plk_poly_mul_dev", lib().plk_poly_mul_dev(_ptr(a), int(la), _ptr(b), int(lb), _ptr(out),
                                                      _ptr(nz), _ptr(work), _stream(stream)))


class PolyMulJob(C.Structure):
    """plk_polymul_job_t (include/plonkhip.h)"""
    _fields_ = [("a", C.c_void_p), ("la", C.c_size_t), ("b", C.c_void_p), ("lb", C.c_size_t),
                ("out", C.c_void_p), ("acc", C.c_int)]


def _jobs(jobs):
    arr = (PolyMulJob * len(jobs))()
    for i, (a, la, b, lb, out, acc) in enumerate(jobs):
        arr[i] = PolyMulJob(_ptr(a), int(la), _ptr(b), int(lb), _ptr(out), int(acc))
    return arr


def poly_mul_batch_workspace(jobs):
    """jobs: (a, la, b, lb, out, acc) tuples of device tensors / pointers"""
    arr = _jobs(jobs)
    return int(lib().plk_poly_mul_batch_workspace(arr, len(jobs)))


def poly_mul_batch_dev(jobs, work, work_bytes, stream=None):
    arr = _jobs(jobs)
    _check("plk_poly_mul_batch_dev", lib().plk_poly_mul_batch_dev(arr, len(jobs), _ptr(work), int(work_bytes),
                                                                  _stream(stream)))


def poly_eval_workspace(n):
    return int(lib().plk_poly_eval_workspace(int(n)))


def poly_eval_batch_dev(polys, lens, xs, ys, tick, stream=None):
    """polys: device tensors (or raw pointers); tick: zeroed device workspace."""
    n = len(polys)
    ptrs = (_vp * n)(*[_ptr(p) for p in polys])
    ls = (_sz * n)(*[int(v) for v in lens])
    xa = _u8(xs).reshape(-1)
    _check("plk_poly_eval_batch_dev", lib().plk_poly_eval_batch_dev(ptrs, ls, _p(xa), n, _ptr(ys), _ptr(tick),
                                                                    _stream(stream)))


def poly_divide_workspace(nl, dl):
    return int(lib().plk_poly_divide_workspace(int(nl), int(dl)))


def poly_divide_path(den, nl):
    """plk_poly_divide_path: 0 trivial, 1 constant, 2 binomial scan, 3 serial loop, 4 Newton under the
    current options; a negated PLK_ERR_* for a zero divisor / a lead byte >= 17.  No device needed."""
    d = _u8(den).reshape(-1)
    return int(lib().plk_poly_divide_path(_p(d), d.size, int(nl)))


def poly_divide_dev(num, nl, den, quot, rem, lens, work, stream=None):
    """den: HOST bytes (classified on the host)."""
    d = _u8(den).reshape(-1)
    _check("plk_poly_divide_dev", lib().plk_poly_divide_dev(_ptr(num), int(nl), _p(d), d.size, _ptr(quot),
                                                            _ptr(rem), _ptr(lens), _ptr(work), _stream(stream)))


def ntt_dev(data, log_n, inverse=False, stream=None):
    _check("plk_ntt_dev", lib().plk_ntt_dev(_ptr(data), int(log_n), 1 if inverse else 0,
                                            _stream(stream)))


def ntt_batch_dev(data, log_n, batch, inverse=False, stream=None):
    _check("plk_ntt_batch_dev", lib().plk_ntt_batch_dev(_ptr(data), int(log_n), int(batch), 1 if inverse else 0,
                                                        _stream(stream)))


def ntt29_dev(data, log_n, inverse=False, stream=None):
    """plk_ntt29_dev: the same transform over F29 (p = 7 2^26 + 1), log_n 13..26."""
    _check("plk_ntt29_dev", lib().plk_ntt29_dev(_ptr(data), int(log_n), 1 if inverse else 0, _stream(stream)))


def ntt29_batch_dev(data, log_n, batch, inverse=False, stream=None):
    _check("plk_ntt29_batch_dev", lib().plk_ntt29_batch_dev(_ptr(data), int(log_n), int(batch),
                                                            1 if inverse else 0, _stream(stream)))


def parse_result(res_bytes):
    """Decode a plk_msm_result_t (MSM_RESULT_BYTES) copied to the host."""
    b = bytes(res_bytes)
    return {"log": int.from_bytes(b[MSM_LOG_OFFSET:MSM_LOG_OFFSET + 4], "little"),
            "irregular": int.from_bytes(b[MSM_IRREGULAR_OFFSET:MSM_IRREGULAR_OFFSET + 4], "little"),
            "g1": b[MSM_G1_OFFSET:MSM_G1_OFFSET + 3]}


# ---------------------------------------------------------------- KZG over a resident SRS
class Srs:
    """plk_srs_t: an SRS resident on the device (G1 form and log form); `with Srs(g1s) as s: ...`"""

    def __init__(self, g1s):
        pts = _u8(g1s).reshape(-1)
        if pts.size % 3:
            raise ValueError("an SRS is n x 3 bytes")
        self._h = _vp()
        _check("plk_srs_create", lib().plk_srs_create(_p(pts), pts.size // 3, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().plk_srs_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __len__(self):
        return int(lib().plk_srs_len(self._h))

    @property
    def irregular(self):
        return bool(lib().plk_srs_irregular(self._h))


def _srs_h(srs):
    return srs._h if isinstance(srs, Srs) else srs


def _host_polys(polys):
    arrs = [_u8(p).reshape(-1) for p in polys]
    n = len(arrs)
    ptrs = (_u8p * max(n, 1))(*[_p(a) for a in arrs])
    lens = (_sz * max(n, 1))(*[a.size for a in arrs])
    return arrs, ptrs, lens, n


def kzg_commit(srs, polys):
    """plk_kzg_commit_batch: [3 bytes] per polynomial, = msm_g1(srs[:len(p)], p)"""
    arrs, ptrs, lens, n = _host_polys(polys)
    out = np.zeros(3 * max(n, 1), np.uint8)
    _check("plk_kzg_commit_batch", lib().plk_kzg_commit_batch(_srs_h(srs), ptrs, lens, n, _p(out)))
    return [bytes(out[3 * i:3 * i + 3]) for i in range(n)]


def kzg_open(srs, polys, zs):
    """plk_kzg_open_batch: ([y], [proof 3 bytes]) -- y = p(z) and the commitment of (p - y) / (x - z)"""
    arrs, ptrs, lens, n = _host_polys(polys)
    za = _u8(zs).reshape(-1)
    if za.size != n:
        raise ValueError("one z per polynomial")
    ys = np.zeros(max(n, 1), np.uint8)
    out = np.zeros(3 * max(n, 1), np.uint8)
    _check("plk_kzg_open_batch", lib().plk_kzg_open_batch(_srs_h(srs), ptrs, lens, _p(za), n, _p(ys), _p(out)))
    return [int(v) for v in ys[:n]], [bytes(out[3 * i:3 * i + 3]) for i in range(n)]


def kzg_workspace(lens):
    """plk_kzg_workspace: bytes of d_work for kzg_open_dev over these lengths.  No device needed."""
    n = len(lens)
    ls = (_sz * max(n, 1))(*[int(v) for v in lens])
    return int(lib().plk_kzg_workspace(ls, n))


def kzg_commit_dev(srs, polys, lens, res, stream=None):
    """polys: device tensors (or raw pointers); res: n zeroed plk_msm_result_t records."""
    n = len(polys)
    ptrs = (_vp * max(n, 1))(*[_ptr(p) for p in polys])
    ls = (_sz * max(n, 1))(*[int(v) for v in lens])
    _check("plk_kzg_commit_batch_dev", lib().plk_kzg_commit_batch_dev(_srs_h(srs), ptrs, ls, n, _ptr(res),
                                                                      _stream(stream)))


def kzg_open_dev(srs, polys, lens, zs, ys, res, quots=None, work=None, stream=None):
    """polys / quots: device tensors (or raw pointers; quots None, or None per job); ys: n device
    bytes; res: n zeroed records; work: kzg_workspace(lens) device bytes."""
    n = len(polys)
    ptrs = (_vp * max(n, 1))(*[_ptr(p) for p in polys])
    ls = (_sz * max(n, 1))(*[int(v) for v in lens])
    za = _u8(zs).reshape(-1)
    qs = None if quots is None else (_vp * max(n, 1))(*[_ptr(q) for q in quots])
    _check("plk_kzg_open_batch_dev", lib().plk_kzg_open_batch_dev(_srs_h(srs), ptrs, ls, _p(za), n, _ptr(ys),
                                                                  _ptr(res), qs, _ptr(work), _stream(stream)))


# ---------------------------------------------------------------- pairings and KZG verification
class KzgVk(C.Structure):
    """plk_kzg_vk_t: [1]_1 (3 bytes), [1]_2 and [s]_2 (2 bytes each); KzgVk((1, 2, 0), (36, 31), (90, 82))"""
    _fields_ = [("g1", C.c_uint8 * 3), ("g2_1", C.c_uint8 * 2), ("g2_s", C.c_uint8 * 2), ("pad", C.c_uint8)]

    def __init__(self, g1, g2_1, g2_s):
        super().__init__((C.c_uint8 * 3)(*bytes(g1)), (C.c_uint8 * 2)(*bytes(g2_1)), (C.c_uint8 * 2)(*bytes(g2_s)), 0)


def pairing(g1s, g2s):
    """plk_pairing_batch: n x 2 GT bytes {a, b} of pairing(g1s[i], g2s[i]); FF FF for an invalid encoding"""
    p, q = _u8(g1s).reshape(-1), _u8(g2s).reshape(-1)
    if p.size % 3 or q.size % 2 or p.size // 3 != q.size // 2:
        raise ValueError("n x 3 bytes of G1 and n x 2 bytes of G2")
    n = p.size // 3
    out = np.zeros(2 * max(n, 1), np.uint8)
    _check("plk_pairing_batch", lib().plk_pairing_batch(_p(p), _p(q), n, _p(out)))
    return out[:2 * n].reshape(n, 2)


def pairing_dev(g1s, g2s, n, out, stream=None):
    """g1s (3 n), g2s (2 n), out (2 n): device tensors (or raw pointers) of any alignment"""
    _check("plk_pairing_batch_dev", lib().plk_pairing_batch_dev(_ptr(g1s), _ptr(g2s), int(n), _ptr(out),
                                                                _stream(stream)))


def kzg_verify(vk, commits, zs, ys, proofs):
    """plk_kzg_verify_batch: n bytes, 1 accept / 0 reject / 2 an invalid byte in the job"""
    c, w = _u8(commits).reshape(-1), _u8(proofs).reshape(-1)
    za, ya = _u8(zs).reshape(-1), _u8(ys).reshape(-1)
    n = za.size
    if c.size != 3 * n or w.size != 3 * n or ya.size != n:
        raise ValueError("n commitments and proofs of 3 bytes, n bytes of z and of y")
    ok = np.zeros(max(n, 1), np.uint8)
    _check("plk_kzg_verify_batch", lib().plk_kzg_verify_batch(C.byref(vk), _p(c), _p(za), _p(ya), _p(w), n, _p(ok)))
    return ok[:n]


def kzg_verify_dev(vk, commits, zs, ys, proofs, n, ok, stream=None):
    """vk: a KzgVk on the host; the rest device tensors (or raw pointers) of any alignment; ok: n bytes"""
    _check("plk_kzg_verify_batch_dev", lib().plk_kzg_verify_batch_dev(
        C.byref(vk), _ptr(commits), _ptr(zs), _ptr(ys), _ptr(proofs), int(n), _ptr(ok), _stream(stream)))


# ---------------------------------------------------------------- KZG folded openings
def _fold_start(counts):
    start = [0]
    for k in counts:
        start.append(start[-1] + int(k))
    return (C.c_int * len(start))(*start)


def kzg_fold_workspace(lens, start):
    """plk_kzg_fold_workspace: bytes of d_work for kzg_open_fold_dev; start: the ngroups + 1 group
    boundaries in the flat arrays.  No device needed; 0 for bad arguments."""
    ng = len(start) - 1
    ls = (_sz * max(len(lens), 1))(*[int(v) for v in lens])
    st = (C.c_int * max(len(start), 1))(*[int(v) for v in start])
    return int(lib().plk_kzg_fold_workspace(ls, st, ng))


def kzg_open_fold(srs, groups, weights, zs):
    """plk_kzg_open_fold_batch: groups = [[polynomial, ...], ...] (1 .. 16 each), weights the same shape,
    one z per group -> ([[y, ...], ...], [proof 3 bytes per group]): every y_i = p_i(z) and the commitment
    of (sum_i w_i (p_i - y_i)) / (x - z)"""
    if len(weights) != len(groups) or any(len(w) != len(g) for w, g in zip(weights, groups)):
        raise ValueError("one weight per polynomial")
    arrs, ptrs, lens, n = _host_polys([p for g in groups for p in g])
    wa = _u8([w for g in weights for w in g]).reshape(-1)
    za = _u8(zs).reshape(-1)
    ng = len(groups)
    if za.size != ng:
        raise ValueError("one z per group")
    start = _fold_start(len(g) for g in groups)
    ys = np.zeros(max(n, 1), np.uint8)
    out = np.zeros(3 * max(ng, 1), np.uint8)
    _check("plk_kzg_open_fold_batch", lib().plk_kzg_open_fold_batch(_srs_h(srs), ptrs, lens, _p(wa), start, _p(za), ng,
                                                                    _p(ys), _p(out)))
    return ([[int(v) for v in ys[start[g]:start[g + 1]]] for g in range(ng)],
            [bytes(out[3 * g:3 * g + 3]) for g in range(ng)])


def kzg_open_fold_dev(srs, polys, lens, weights, start, zs, ys, res, quots=None, work=None, stream=None):
    """polys: the flat list of device tensors (or raw pointers), group g = [start[g], start[g + 1]); lens,
    weights, start, zs: host values; ys: len(polys) device bytes; res: one zeroed record per group;
    quots: None, or per group None / max(L - 1, 1) device bytes; work: kzg_fold_workspace(lens, start)
    device bytes."""
    n = len(polys)
    ng = len(start) - 1
    ptrs = (_vp * max(n, 1))(*[_ptr(p) for p in polys])
    ls = (_sz * max(n, 1))(*[int(v) for v in lens])
    st = (C.c_int * max(len(start), 1))(*[int(v) for v in start])
    wa = _u8(weights).reshape(-1)
    za = _u8(zs).reshape(-1)
    qs = None if quots is None else (_vp * max(ng, 1))(*[_ptr(q) for q in quots])
    _check("plk_kzg_open_fold_batch_dev", lib().plk_kzg_open_fold_batch_dev(
        _srs_h(srs), ptrs, ls, _p(wa), st, _p(za), ng, _ptr(ys), _ptr(res), qs, _ptr(work), _stream(stream)))


def kzg_verify_fold(vk, k, commits, weights, ys, zs, proofs):
    """plk_kzg_verify_fold_batch: job b owns entries [k b, k (b + 1)) of commits (3 bytes each), weights
    and ys; one z and one proof per job -> n bytes, 1 accept / 0 reject / 2 an invalid byte in the job"""
    c, w = _u8(commits).reshape(-1), _u8(proofs).reshape(-1)
    wa, ya, za = _u8(weights).reshape(-1), _u8(ys).reshape(-1), _u8(zs).reshape(-1)
    n = za.size
    e = n * int(k)
    if c.size != 3 * e or wa.size != e or ya.size != e or w.size != 3 * n:
        raise ValueError("n k commitments, weights and ys; n zs and proofs")
    ok = np.zeros(max(n, 1), np.uint8)
    _check("plk_kzg_verify_fold_batch", lib().plk_kzg_verify_fold_batch(C.byref(vk), int(k), _p(c), _p(wa), _p(ya),
                                                                        _p(za), _p(w), n, _p(ok)))
    return ok[:n]


def kzg_verify_fold_dev(vk, k, commits, weights, ys, zs, proofs, n, ok, stream=None):
    """vk: a KzgVk on the host; the rest device tensors (or raw pointers) of any alignment; ok: n bytes"""
    _check("plk_kzg_verify_fold_batch_dev", lib().plk_kzg_verify_fold_batch_dev(
        C.byref(vk), int(k), _ptr(commits), _ptr(weights), _ptr(ys), _ptr(zs), _ptr(proofs), int(n), _ptr(ok),
        _stream(stream)))


# ---------------------------------------------------------------- KZG multi-point openings
PLK_KZG_MULTI_MAX = 15
PLK_KZG_MULTI_POINTS = 16


def _u32s(a):
    v = [int(x) for x in a]
    return (C.c_uint32 * max(len(v), 1))(*v)


def kzg_multi_coeffs(sets, weights, u):
    """plk_kzg_multi_coeffs: sets = one mask per polynomial (bit a set: the point a) -> the k + 1 weights of the
    second proof's fold, c_i = w_i prod_{a in T \\ S_i} (u - a) and (17 - c_T) % 17.  No device needed."""
    k = len(sets)
    wa = _u8(weights).reshape(-1)
    if wa.size != k:
        raise ValueError("one weight per set")
    out = np.zeros(k + 1, np.uint8)
    _check("plk_kzg_multi_coeffs", lib().plk_kzg_multi_coeffs(_u32s(sets), _p(wa), k, int(u), _p(out)))
    return [int(v) for v in out]


def kzg_multi_workspace(lens, sets, start):
    """plk_kzg_multi_workspace: bytes of d_work for kzg_open_multi_dev; start: the ngroups + 1 group
    boundaries in the flat arrays.  No device needed; 0 for bad arguments."""
    ng = len(start) - 1
    ls = (_sz * max(len(lens), 1))(*[int(v) for v in lens])
    st = (C.c_int * max(len(start), 1))(*[int(v) for v in start])
    return int(lib().plk_kzg_multi_workspace(ls, _u32s(sets), st, ng))


def kzg_open_multi(srs, groups, sets, weights, us):
    """plk_kzg_open_multi_batch: groups = [[polynomial, ...], ...] (1 .. 15 each), sets (masks) and weights the
    same shape, one u per group -> ([[17-byte row per polynomial, ...], ...], [6 proof bytes W, W' per group]);
    row[a] = p_i(a) for a in S_i, 0xFF elsewhere"""
    if any(len(x) != len(groups) for x in (sets, weights)) or \
            any(len(w) != len(g) or len(m) != len(g) for w, m, g in zip(weights, sets, groups)):
        raise ValueError("one set and one weight per polynomial")
    arrs, ptrs, lens, n = _host_polys([p for g in groups for p in g])
    wa = _u8([w for g in weights for w in g]).reshape(-1)
    ua = _u8(us).reshape(-1)
    ng = len(groups)
    if ua.size != ng:
        raise ValueError("one u per group")
    start = _fold_start(len(g) for g in groups)
    ys = np.zeros(17 * max(n, 1), np.uint8)
    out = np.zeros(6 * max(ng, 1), np.uint8)
    _check("plk_kzg_open_multi_batch", lib().plk_kzg_open_multi_batch(
        _srs_h(srs), ptrs, lens, _u32s([m for g in sets for m in g]), _p(wa), start, _p(ua), ng, _p(ys), _p(out)))
    return ([[bytes(ys[17 * i:17 * i + 17]) for i in range(start[g], start[g + 1])] for g in range(ng)],
            [bytes(out[6 * g:6 * g + 6]) for g in range(ng)])


def kzg_open_multi_dev(srs, polys, lens, sets, weights, start, us, ys, res, hs=None, work=None, stream=None):
    """polys: the flat list of device tensors (or raw pointers), group g = [start[g], start[g + 1]); lens, sets,
    weights, start, us: host values; ys: 17 len(polys) device bytes; res: two zeroed records per group (W at
    2 g, W' at 2 g + 1); hs: None, or per group None / Lh device bytes; work: kzg_multi_workspace(lens, sets,
    start) device bytes."""
    n = len(polys)
    ng = len(start) - 1
    ptrs = (_vp * max(n, 1))(*[_ptr(p) for p in polys])
    ls = (_sz * max(n, 1))(*[int(v) for v in lens])
    st = (C.c_int * max(len(start), 1))(*[int(v) for v in start])
    wa = _u8(weights).reshape(-1)
    ua = _u8(us).reshape(-1)
    hp = None if hs is None else (_vp * max(ng, 1))(*[_ptr(h) for h in hs])
    _check("plk_kzg_open_multi_batch_dev", lib().plk_kzg_open_multi_batch_dev(
        _srs_h(srs), ptrs, ls, _u32s(sets), _p(wa), st, _p(ua), ng, _ptr(ys), _ptr(res), hp, _ptr(work), _stream(stream)))


def kzg_verify_multi(vk, k, commits, sets, weights, ys, us, proofs):
    """plk_kzg_verify_multi_batch: job b owns entries [k b, k (b + 1)) of commits (3 bytes each), sets (masks),
    weights and ys (17-byte rows); one u and six proof bytes W, W' per job -> n bytes, 1 accept / 0 reject /
    2 an invalid byte in the job"""
    c, w = _u8(commits).reshape(-1), _u8(proofs).reshape(-1)
    wa, ya, ua = _u8(weights).reshape(-1), _u8(ys).reshape(-1), _u8(us).reshape(-1)
    sa = np.ascontiguousarray(np.asarray(sets, dtype=np.uint32).reshape(-1))
    n = ua.size
    e = n * int(k)
    if c.size != 3 * e or wa.size != e or sa.size != e or ya.size != 17 * e or w.size != 6 * n:
        raise ValueError("n k commitments, sets, weights and 17-byte rows of ys; n us and 6-byte proofs")
    ok = np.zeros(max(n, 1), np.uint8)
    _check("plk_kzg_verify_multi_batch", lib().plk_kzg_verify_multi_batch(
        C.byref(vk), int(k), _p(c), sa.ctypes.data_as(C.POINTER(C.c_uint32)), _p(wa), _p(ya), _p(ua), _p(w), n, _p(ok)))
    return ok[:n]


def kzg_verify_multi_dev(vk, k, commits, sets, weights, ys, us, proofs, n, ok, stream=None):
    """vk: a KzgVk on the host; the rest device tensors (or raw pointers) of any alignment, the masks
    (4 bytes each) 4-byte aligned; ok: n bytes"""
    _check("plk_kzg_verify_multi_batch_dev", lib().plk_kzg_verify_multi_batch_dev(
        C.byref(vk), int(k), _ptr(commits), _ptr(sets), _ptr(weights), _ptr(ys), _ptr(us), _ptr(proofs), int(n), _ptr(ok),
        _stream(stream)))


# ---------------------------------------------------------------- KZG aggregate verification
PLK_KZG_AGG_UNDECIDED = 3
KZG_AGG_PLAN_FIELDS = ("path", "slices", "blocks", "launches")


def kzg_verify_agg_plan(m, n):
    """plk_kzg_verify_agg_plan: the geometry of kzg_verify_agg_dev for n groups of m jobs -- path (0 one lane
    per group, 1 one wave per group, 2 `slices` blocks per group), slices (records per group in the
    workspace), blocks of the first launch, launches.  No device needed."""
    out = (C.c_int64 * 4)()
    _check("plk_kzg_verify_agg_plan", lib().plk_kzg_verify_agg_plan(int(m), int(n), out))
    return dict(zip(KZG_AGG_PLAN_FIELDS, (int(v) for v in out)))


def kzg_verify_agg_workspace(m, n):
    """plk_kzg_verify_agg_workspace: bytes of d_work for kzg_verify_agg_dev; 0 where the plan says one launch
    and for bad arguments.  No device needed."""
    return int(lib().plk_kzg_verify_agg_workspace(int(m), int(n)))


def kzg_verify_agg(vk, m, commits, zs, ys, proofs, rs):
    """plk_kzg_verify_agg_batch: n groups of m consecutive jobs (as kzg_verify's, plus a weight byte r per
    job) -> n bytes, 1 the group's weighted sum accepts / 0 rejects / 2 an invalid byte in the group.  An
    accept is a statement about the weighted sum, not about each job."""
    c, w = _u8(commits).reshape(-1), _u8(proofs).reshape(-1)
    za, ya, ra = _u8(zs).reshape(-1), _u8(ys).reshape(-1), _u8(rs).reshape(-1)
    m = int(m)
    e = za.size
    if m <= 0 or e % m or c.size != 3 * e or w.size != 3 * e or ya.size != e or ra.size != e:
        raise ValueError("n m commitments and proofs of 3 bytes, n m bytes of z, of y and of r")
    n = e // m
    ok = np.zeros(max(n, 1), np.uint8)
    _check("plk_kzg_verify_agg_batch", lib().plk_kzg_verify_agg_batch(C.byref(vk), m, _p(c), _p(za), _p(ya), _p(w),
                                                                      _p(ra), n, _p(ok)))
    return ok[:n]


def kzg_verify_agg_dev(vk, m, commits, zs, ys, proofs, rs, n, ok, work=None, stream=None):
    """vk: a KzgVk on the host; the rest device tensors (or raw pointers) of any alignment; ok: n bytes, 3
    (PLK_KZG_AGG_UNDECIDED) for a valid group that is not canonical; work: kzg_verify_agg_workspace(m, n)
    device bytes, None where that is 0"""
    _check("plk_kzg_verify_agg_batch_dev", lib().plk_kzg_verify_agg_batch_dev(
        C.byref(vk), int(m), _ptr(commits), _ptr(zs), _ptr(ys), _ptr(proofs), _ptr(rs), int(n), _ptr(ok), _ptr(work),
        _stream(stream)))


# ---------------------------------------------------------------- segmented MSM
PLK_MSM_SEG_IRREGULAR = 1
PLK_MSM_SEG_BAD = 2
MSM_SEGMENTS_PLAN_FIELDS = ("path", "tile", "launches", "blocks")


def msm_g1_segments_plan(total, m, nseg, ragged):
    """plk_msm_g1_segments_plan: the geometry of msm_g1_segments_dev -- path (0 one lane per segment: uniform
    m <= 32; 1 prefix: everything else), tile (points per block of the first launch), launches, blocks of the
    first launch.  No device needed."""
    out = (C.c_int64 * 4)()
    _check("plk_msm_g1_segments_plan", lib().plk_msm_g1_segments_plan(int(total), int(m), int(nseg), int(bool(ragged)), out))
    return dict(zip(MSM_SEGMENTS_PLAN_FIELDS, (int(v) for v in out)))


def msm_g1_segments_workspace(total, m, nseg, ragged):
    """plk_msm_g1_segments_workspace: bytes of d_work for msm_g1_segments_dev; 0 where the plan says one launch
    and for bad arguments.  No device needed."""
    return int(lib().plk_msm_g1_segments_workspace(int(total), int(m), int(nseg), int(bool(ragged))))


def msm_g1_segments(points, scalars, offsets=None, m=None):
    """plk_msm_g1_segments: segment g = points and scalars [offsets[g], offsets[g + 1]) (ragged), or
    [g m, (g + 1) m) with offsets None (uniform) -> an (nseg, 3) array, row g the bytes msm_g1 returns for
    that segment, for every input byte."""
    pts, sc = _u8(points).reshape(-1), _u8(scalars).reshape(-1)
    total = sc.size
    if pts.size != 3 * total:
        raise ValueError("points must be n x 3 bytes for n scalars")
    if offsets is None:
        if m is None or int(m) <= 0 or total % int(m):
            raise ValueError("uniform segments: m > 0 dividing the number of points")
        m, nseg, off = int(m), total // int(m), None
    else:
        ov = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint32).reshape(-1))
        m, nseg, off = 0, ov.size - 1, ov.ctypes.data_as(C.POINTER(C.c_uint32))
    out = np.zeros((max(nseg, 1), 3), np.uint8)
    _check("plk_msm_g1_segments", lib().plk_msm_g1_segments(_p(pts), _p(sc), total, off, m, max(nseg, 0), _p(out)))
    return out[:max(nseg, 0)]


def msm_g1_segments_dev(points, scalars, total, offsets, m, nseg, out4, work=None, stream=None):
    """device tensors (or raw pointers) of any alignment; offsets: nseg + 1 uint32 words on the device, or None
    for uniform segments of m points; out4: 4 nseg bytes {x, y, infinite, status}; work:
    msm_g1_segments_workspace device bytes, None where that is 0"""
    _check("plk_msm_g1_segments_dev", lib().plk_msm_g1_segments_dev(
        _ptr(points), _ptr(scalars), int(total), _ptr(offsets), int(m), int(nseg), _ptr(out4), _ptr(work),
        _stream(stream)))


# ---------------------------------------------------------------- KZG per-point openings
PLK_KZG_POINTS_LAUNCH_POLYS = 64


def kzg_points_count(sets):
    """plk_kzg_points_count: J = the jobs of these sets (masks, bit a set: the point a; all 17 bits allowed);
    0 for an invalid mask.  No device needed."""
    return int(lib().plk_kzg_points_count(_u32s(sets), len(sets)))


def kzg_points_workspace(lens, sets):
    """plk_kzg_points_workspace: bytes of d_work for kzg_open_points_dev; 0 when every polynomial fits one
    chunk and for bad arguments.  No device needed."""
    n = len(lens)
    if len(sets) != n:
        raise ValueError("one set per polynomial")
    ls = (_sz * max(n, 1))(*[int(v) for v in lens])
    return int(lib().plk_kzg_points_workspace(ls, _u32s(sets), n))


def kzg_open_points(srs, polys, sets):
    """plk_kzg_open_points_batch: one set (mask) per polynomial -> ([z], [y], [proof 3 bytes]) flat in job
    order (polynomials in order, within one its points ascending): what kzg_open returns on the expanded list"""
    arrs, ptrs, lens, n = _host_polys(polys)
    if len(sets) != n:
        raise ValueError("one set per polynomial")
    j = kzg_points_count(sets) if n else 0
    zs = np.zeros(max(j, 1), np.uint8)
    ys = np.zeros(max(j, 1), np.uint8)
    out = np.zeros(3 * max(j, 1), np.uint8)
    _check("plk_kzg_open_points_batch", lib().plk_kzg_open_points_batch(_srs_h(srs), ptrs, lens, _u32s(sets), n, _p(zs),
                                                                        _p(ys), _p(out)))
    return ([int(v) for v in zs[:j]], [int(v) for v in ys[:j]], [bytes(out[3 * i:3 * i + 3]) for i in range(j)])


def kzg_open_points_dev(srs, d_polys, lens, sets, zs, ys, proofs3, status, work=None, stream=None):
    """d_polys: device tensors (or raw pointers); lens, sets: host values; zs (or None), ys, status: J device
    bytes, proofs3: 3 J, J = kzg_points_count(sets); work: kzg_points_workspace(lens, sets) device bytes, None
    where that is 0."""
    n = len(d_polys)
    ptrs = (_vp * max(n, 1))(*[_ptr(p) for p in d_polys])
    ls = (_sz * max(n, 1))(*[int(v) for v in lens])
    _check("plk_kzg_open_points_batch_dev", lib().plk_kzg_open_points_batch_dev(
        _srs_h(srs), ptrs, ls, _u32s(sets), n, _ptr(zs), _ptr(ys), _ptr(proofs3), _ptr(status), _ptr(work),
        _stream(stream)))


# ---------------------------------------------------------------- KZG flat batches
PLK_KZG_FLAT_MAX = 4096
PLK_KZG_FLAT_IRREGULAR = 1
PLK_KZG_FLAT_BAD = 2
KZG_FLAT_PLAN_FIELDS = ("path", "per_block", "blocks", "launches")


def kzg_flat_plan(m, npoly, ragged=False):
    """plk_kzg_flat_plan: the geometry of the flat calls -- path (0 one lane per polynomial: m <= 32; 1 one wave:
    m <= 1024; 2 one block: m <= 4096), polynomials per block, blocks, launches (1).  No device needed."""
    out = (C.c_int64 * 4)()
    _check("plk_kzg_flat_plan", lib().plk_kzg_flat_plan(int(m), int(npoly), int(bool(ragged)), out))
    return dict(zip(KZG_FLAT_PLAN_FIELDS, (int(v) for v in out)))


def _flat_host(coeffs, offsets, m):
    co = _u8(coeffs).reshape(-1)
    if offsets is None:
        if m is None or int(m) <= 0 or co.size % int(m):
            raise ValueError("uniform polynomials: m > 0 dividing the number of coefficients")
        return co, None, None, int(m), co.size // int(m)
    ov = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint32).reshape(-1))
    if m is None:
        m = int(np.diff(ov.astype(np.int64)).max()) if ov.size > 1 else 1
    return co, ov, ov.ctypes.data_as(C.POINTER(C.c_uint32)), int(m), ov.size - 1


def kzg_commit_flat(srs, coeffs, offsets=None, m=None):
    """plk_kzg_commit_flat: polynomial g = coeffs[offsets[g]:offsets[g + 1]] (ragged; m the length bound, by
    default the longest), or coeffs[g m:(g + 1) m] with offsets None -> an (npoly, 3) array, row g what
    kzg_commit returns for that polynomial, for every input byte."""
    co, keep, off, m, npoly = _flat_host(coeffs, offsets, m)
    out = np.zeros((max(npoly, 1), 3), np.uint8)
    _check("plk_kzg_commit_flat", lib().plk_kzg_commit_flat(_srs_h(srs), _p(co), co.size, off, m, max(npoly, 0), _p(out)))
    return out[:max(npoly, 0)]


def kzg_open_flat(srs, coeffs, zs, offsets=None, m=None, commits=False):
    """plk_kzg_open_flat: the polynomials of kzg_commit_flat, polynomial g opened at zs[g] -> (ys, proofs) or
    (ys, proofs, commitments): npoly bytes and (npoly, 3) arrays, what kzg_open / kzg_commit return on the
    expanded list, for every input byte."""
    co, keep, off, m, npoly = _flat_host(coeffs, offsets, m)
    za = _u8(zs).reshape(-1)
    if za.size != npoly:
        raise ValueError("one z per polynomial")
    ys = np.zeros(max(npoly, 1), np.uint8)
    pr = np.zeros((max(npoly, 1), 3), np.uint8)
    cm = np.zeros((max(npoly, 1), 3), np.uint8) if commits else None
    _check("plk_kzg_open_flat", lib().plk_kzg_open_flat(_srs_h(srs), _p(co), co.size, off, m, max(npoly, 0), _p(za), _p(ys),
                                                        _p(pr), _p(cm) if commits else None))
    n = max(npoly, 0)
    return (ys[:n], pr[:n], cm[:n]) if commits else (ys[:n], pr[:n])


def kzg_commit_flat_dev(srs, coeffs, total, offsets, m, npoly, commits3, status, stream=None):
    """device tensors (or raw pointers) of any alignment; offsets: npoly + 1 uint32 words on the device, or None
    for uniform polynomials of m coefficients; commits3: 3 npoly bytes; status: npoly bytes"""
    _check("plk_kzg_commit_flat_dev", lib().plk_kzg_commit_flat_dev(
        _srs_h(srs), _ptr(coeffs), int(total), _ptr(offsets), int(m), int(npoly), _ptr(commits3), _ptr(status),
        _stream(stream)))


def kzg_open_flat_dev(srs, coeffs, total, offsets, m, npoly, zs, ys, proofs3, commits3, status, stream=None):
    """as kzg_commit_flat_dev; zs, ys, status: npoly device bytes; proofs3: 3 npoly; commits3: 3 npoly or None.
    (commits3, zs, ys, proofs3) are the arguments of kzg_verify_dev / kzg_verify_agg_dev as they stand."""
    _check("plk_kzg_open_flat_dev", lib().plk_kzg_open_flat_dev(
        _srs_h(srs), _ptr(coeffs), int(total), _ptr(offsets), int(m), int(npoly), _ptr(zs), _ptr(ys), _ptr(proofs3),
        _ptr(commits3), _ptr(status), _stream(stream)))


# ---------------------------------------------------------------- KZG flat folded openings
def kzg_fold_flat_plan(m, k, ngroups, ragged=False):
    """plk_kzg_fold_flat_plan: the geometry of the flat folded calls -- path (0 one lane per group: m <= 32; 1 one
    wave: m <= 1024; 2 one block: m <= 4096), groups per block, blocks, launches (1).  No device needed."""
    out = (C.c_int64 * 4)()
    _check("plk_kzg_fold_flat_plan", lib().plk_kzg_fold_flat_plan(int(m), int(k), int(ngroups), int(bool(ragged)), out))
    return dict(zip(KZG_FLAT_PLAN_FIELDS, (int(v) for v in out)))


def kzg_open_fold_flat(srs, coeffs, k, weights, zs, offsets=None, m=None, commits=False):
    """plk_kzg_open_fold_flat: the polynomials of kzg_commit_flat in groups of k, group g = polynomials and weights
    [k g, k (g + 1)) opened at zs[g] with one proof -> (ys, proofs) or (ys, proofs, commitments): npoly bytes,
    (ngroups, 3) and (npoly, 3) arrays, what kzg_open_fold / kzg_commit return on the expanded groups, for every
    input byte."""
    co, keep, off, m, npoly = _flat_host(coeffs, offsets, m)
    k = int(k)
    if k <= 0 or npoly % k:
        raise ValueError("k > 0 dividing the number of polynomials")
    ng = npoly // k
    wa, za = _u8(weights).reshape(-1), _u8(zs).reshape(-1)
    if wa.size != npoly or za.size != ng:
        raise ValueError("one weight per polynomial and one z per group")
    ys = np.zeros(max(npoly, 1), np.uint8)
    pr = np.zeros((max(ng, 1), 3), np.uint8)
    cm = np.zeros((max(npoly, 1), 3), np.uint8) if commits else None
    _check("plk_kzg_open_fold_flat", lib().plk_kzg_open_fold_flat(_srs_h(srs), _p(co), co.size, off, m, k, max(ng, 0), _p(wa),
                                                                  _p(za), _p(ys), _p(pr), _p(cm) if commits else None))
    n, g = max(npoly, 0), max(ng, 0)
    return (ys[:n], pr[:g], cm[:n]) if commits else (ys[:n], pr[:g])


def kzg_open_fold_flat_dev(srs, coeffs, total, offsets, m, k, ngroups, weights, zs, ys, proofs3, commits3, status,
                           stream=None):
    """device tensors (or raw pointers) of any alignment; offsets: k ngroups + 1 uint32 words on the device, or None
    for uniform polynomials of m coefficients; weights, ys: k ngroups device bytes; zs, status: ngroups; proofs3:
    3 ngroups; commits3: 3 k ngroups or None.  (commits3, weights, ys, zs, proofs3) are the arguments of
    kzg_verify_fold_dev(vk, k, ..., n=ngroups) as they stand."""
    _check("plk_kzg_open_fold_flat_dev", lib().plk_kzg_open_fold_flat_dev(
        _srs_h(srs), _ptr(coeffs), int(total), _ptr(offsets), int(m), int(k), int(ngroups), _ptr(weights), _ptr(zs),
        _ptr(ys), _ptr(proofs3), _ptr(commits3), _ptr(status), _stream(stream)))


# ---------------------------------------------------------------- KZG flat multi-point openings
def kzg_multi_flat_plan(m, k, ngroups, ragged=False):
    """plk_kzg_multi_flat_plan: the geometry of the flat multi-point calls -- path (0 one lane per group: m <= 32;
    1 one wave: m <= 1024; 2 one block: m <= 4096), groups per block, blocks, launches (1).  No device needed."""
    out = (C.c_int64 * 4)()
    _check("plk_kzg_multi_flat_plan", lib().plk_kzg_multi_flat_plan(int(m), int(k), int(ngroups), int(bool(ragged)), out))
    return dict(zip(KZG_FLAT_PLAN_FIELDS, (int(v) for v in out)))


def kzg_open_multi_flat(srs, coeffs, k, sets, weights, us, offsets=None, m=None, commits=False):
    """plk_kzg_open_multi_flat: the polynomials of kzg_commit_flat in groups of k, group g = polynomials, sets
    (masks) and weights [k g, k (g + 1)) under the challenge us[g] -> (ys, proofs) or (ys, proofs, commitments):
    (npoly, 17), (ngroups, 6) and (npoly, 3) arrays, what kzg_open_multi / kzg_commit return on the expanded
    groups, for every input byte."""
    co, keep, off, m, npoly = _flat_host(coeffs, offsets, m)
    k = int(k)
    if k <= 0 or npoly % k:
        raise ValueError("k > 0 dividing the number of polynomials")
    ng = npoly // k
    sa = np.ascontiguousarray(np.asarray(sets, dtype=np.uint32).reshape(-1))
    wa, ua = _u8(weights).reshape(-1), _u8(us).reshape(-1)
    if sa.size != npoly or wa.size != npoly or ua.size != ng:
        raise ValueError("one set and one weight per polynomial and one u per group")
    ys = np.zeros((max(npoly, 1), 17), np.uint8)
    pr = np.zeros((max(ng, 1), 6), np.uint8)
    cm = np.zeros((max(npoly, 1), 3), np.uint8) if commits else None
    _check("plk_kzg_open_multi_flat", lib().plk_kzg_open_multi_flat(
        _srs_h(srs), _p(co), co.size, off, m, k, max(ng, 0), sa.ctypes.data_as(C.POINTER(C.c_uint32)), _p(wa), _p(ua),
        _p(ys), _p(pr), _p(cm) if commits else None))
    n, g = max(npoly, 0), max(ng, 0)
    return (ys[:n], pr[:g], cm[:n]) if commits else (ys[:n], pr[:g])


def kzg_open_multi_flat_dev(srs, coeffs, total, offsets, m, k, ngroups, sets, weights, us, ys, proofs6, commits3, status,
                            stream=None):
    """device tensors (or raw pointers) of any alignment, offsets and sets 4-byte aligned; offsets: k ngroups + 1
    uint32 words on the device, or None for uniform polynomials of m coefficients; sets: k ngroups uint32 masks;
    weights: k ngroups device bytes; ys: 17 k ngroups; us, status: ngroups; proofs6: 6 ngroups; commits3:
    3 k ngroups or None.  (commits3, sets, weights, ys, us, proofs6) are the arguments of
    kzg_verify_multi_dev(vk, k, ..., n=ngroups) as they stand."""
    _check("plk_kzg_open_multi_flat_dev", lib().plk_kzg_open_multi_flat_dev(
        _srs_h(srs), _ptr(coeffs), int(total), _ptr(offsets), int(m), int(k), int(ngroups), _ptr(sets), _ptr(weights),
        _ptr(us), _ptr(ys), _ptr(proofs6), _ptr(commits3), _ptr(status), _stream(stream)))


# ---------------------------------------------------------------- poly linear combinations
PLK_LC_MAX_TERMS = 16
PLK_LC_RAW = 0xFF


class LcTerm(C.Structure):
    """plk_lc_term_t"""
    _fields_ = [("p", C.c_void_p), ("len", _sz), ("shift", _sz), ("sub", C.c_uint8), ("scale", C.c_uint8),
                ("neg", C.c_uint8), ("twist", C.c_uint8)]


class LcJob(C.Structure):
    """plk_lc_job_t"""
    _fields_ = [("terms", C.POINTER(LcTerm)), ("nterms", C.c_int), ("add_hf", C.c_int), ("out", C.c_void_p)]


def lc_term(p, len=None, shift=0, sub=0, scale=PLK_LC_RAW, neg=0, twist=0):
    """one term of a linear combination as a dict; p: bytes / array (host form) or a device tensor / raw
    pointer (_dev form, len then required unless p is a tensor)"""
    return {"p": p, "len": len, "shift": shift, "sub": sub, "scale": scale, "neg": neg, "twist": twist}


def _lc_job(terms, add_hf, out, keep, host):
    arr = (LcTerm * max(len(terms), 1))()
    for i, t in enumerate(terms):
        p, ln = t["p"], t.get("len")
        if host:
            a = _u8(p).reshape(-1)
            keep.append(a)
            ptr, ln = a.ctypes.data, a.size if ln is None else ln
        else:
            ptr, ln = _ptr(p), p.numel() if ln is None else ln
        arr[i] = LcTerm(ptr, int(ln), int(t.get("shift", 0)), int(t.get("sub", 0)), int(t.get("scale", PLK_LC_RAW)),
                        int(t.get("neg", 0)), int(t.get("twist", 0)))
    keep.append(arr)
    return LcJob(arr, len(terms), -1 if add_hf is None else int(add_hf), out)


def poly_lincomb_len(terms, add_hf=None):
    """plk_poly_lincomb_len: L = max(len + shift) over lc_term dicts whose p may be None; 0 for bad
    arguments.  No device needed."""
    arr = (LcTerm * max(len(terms), 1))()
    for i, t in enumerate(terms):
        arr[i] = LcTerm(1, int(t["len"]), int(t.get("shift", 0)), int(t.get("sub", 0)),
                        int(t.get("scale", PLK_LC_RAW)), int(t.get("neg", 0)), int(t.get("twist", 0)))
    job = LcJob(arr, len(terms), -1 if add_hf is None else int(add_hf), None)
    return int(lib().plk_poly_lincomb_len(C.byref(job)))


def poly_lincomb(job):
    """plk_poly_lincomb on host bytes: job = (terms, add_hf) with terms a list of lc_term(bytes, ...);
    returns (the L untrimmed result bytes, the trimmed length)"""
    terms, add_hf = job
    keep = []
    L = max(int(np.size(_u8(t["p"])) if t.get("len") is None else t["len"]) + int(t.get("shift", 0)) for t in terms)
    out = np.zeros(max(L, 1), np.uint8)
    j = _lc_job(terms, add_hf, out.ctypes.data, keep, True)
    n = _sz(0)
    _check("plk_poly_lincomb", lib().plk_poly_lincomb(C.byref(j), C.byref(n)))
    return bytes(out[:L]), int(n.value)


def poly_lincomb_batch_dev(jobs, nz=None, stream=None):
    """plk_poly_lincomb_batch_dev: jobs = [(terms, add_hf, out), ...] with device tensors / raw pointers
    in the lc_term dicts and as out; nz: len(jobs) device uint32 words or None"""
    keep = []
    arr = (LcJob * max(len(jobs), 1))()
    for i, (terms, add_hf, out) in enumerate(jobs):
        arr[i] = _lc_job(terms, add_hf, _ptr(out), keep, False)
    _check("plk_poly_lincomb_batch_dev", lib().plk_poly_lincomb_batch_dev(arr, len(jobs), _ptr(nz), _stream(stream)))


# ---------------------------------------------------------------- division by short divisors
PLK_DIV_SHORT_MAX = 17
PLK_DIV_SHORT_LAUNCH_JOBS = 32


class DivShortJob(C.Structure):
    """plk_divshort_job_t"""
    _fields_ = [("num", C.c_void_p), ("nl", _sz), ("den", C.c_void_p), ("dl", _sz), ("quot", C.c_void_p),
                ("rem", C.c_void_p)]


def _divshort_jobs(jobs, keep):
    """jobs: (num, nl, den, quot, rem) with num / quot / rem device tensors or raw pointers, den HOST bytes"""
    arr = (DivShortJob * max(len(jobs), 1))()
    for i, (num, nl, den, quot, rem) in enumerate(jobs):
        d = _u8(den).reshape(-1)
        keep.append(d)
        arr[i] = DivShortJob(_ptr(num), int(nl), d.ctypes.data, d.size, _ptr(quot), _ptr(rem))
    return arr


def poly_divide_short_workspace(shapes):
    """plk_poly_divide_short_workspace for [(nl, dl), ...]: bytes of d_work; 0 for bad arguments.  No device
    needed."""
    arr = (DivShortJob * max(len(shapes), 1))(*[DivShortJob(1, int(nl), 1, int(dl), 1, 1) for nl, dl in shapes])
    return int(lib().plk_poly_divide_short_workspace(arr, len(shapes)))


def poly_divide_short_plan(nl, dl):
    """plk_poly_divide_short_plan: one job of shape (nl, dl) run alone.  No device needed."""
    out = (C.c_int * 4)()
    _check("plk_poly_divide_short_plan", lib().plk_poly_divide_short_plan(int(nl), int(dl), out))
    return dict(zip(("kernels", "per_thread", "per_block", "one_kernel_max"), list(out)))


def poly_divide_short_batch(nums, dens):
    """plk_poly_divide_short_batch on host bytes: [(quot, rem)] trimmed as poly_divide returns them"""
    keep, n = [], len(nums)
    arr = (DivShortJob * max(n, 1))()
    outs = []
    for i, (num, den) in enumerate(zip(nums, dens)):
        a, d = _u8(num).reshape(-1), _u8(den).reshape(-1)
        q, r = np.zeros(max(a.size, 1), np.uint8), np.zeros(max(a.size, 1), np.uint8)
        keep += [a, d]
        outs.append((q, r))
        arr[i] = DivShortJob(a.ctypes.data, a.size, d.ctypes.data, d.size, q.ctypes.data, r.ctypes.data)
    ql, rl = (_sz * max(n, 1))(), (_sz * max(n, 1))()
    _check("plk_poly_divide_short_batch", lib().plk_poly_divide_short_batch(arr, n, ql, rl))
    return [(bytes(q[:ql[i]]), bytes(r[:rl[i]])) for i, (q, r) in enumerate(outs)]


def poly_divide_short_batch_dev(jobs, lens, work, stream=None):
    """plk_poly_divide_short_batch_dev: jobs = [(num, nl, den, quot, rem), ...] (device tensors / raw
    pointers, den HOST bytes); lens: 3 len(jobs) device uint32 words; work: poly_divide_short_workspace bytes"""
    keep = []
    arr = _divshort_jobs(jobs, keep)
    _check("plk_poly_divide_short_batch_dev",
           lib().plk_poly_divide_short_batch_dev(arr, len(jobs), _ptr(lens), _ptr(work), _stream(stream)))


def poly_from_roots(roots):
    """plk_poly_from_roots: the coefficients of prod (x - r), low degree first.  No device needed."""
    r = _u8(roots).reshape(-1)
    out = np.zeros(r.size + 1, np.uint8)
    _check("plk_poly_from_roots", lib().plk_poly_from_roots(_p(r), r.size, _p(out)))
    return bytes(out)


# ---------------------------------------------------------------- products by short operands
PLK_MUL_SHORT_MAX = 1024
PLK_MUL_SHORT_LAUNCH_RUNS = 32


class MulShortRun(C.Structure):
    """plk_mulshort_run_t"""
    _fields_ = [("a", C.c_void_p), ("la", _sz), ("a_stride", _sz), ("b", C.c_void_p), ("lb", _sz), ("b_stride", _sz),
                ("out", C.c_void_p), ("out_stride", _sz), ("count", _sz)]


def mul_short_run(a, la, b, lb, out, count=1, a_stride=0, b_stride=0, out_stride=0):
    """a MulShortRun from device tensors / raw pointers: count products of la x lb coefficients, product i at
    a + i a_stride, b + i b_stride, out + i out_stride"""
    return MulShortRun(_ptr(a), int(la), int(a_stride), _ptr(b), int(lb), int(b_stride), _ptr(out), int(out_stride),
                       int(count))


def poly_mul_short_plan(la, lb, count=1):
    """plk_poly_mul_short_plan: one run of count products of shape (la, lb) alone.  No device needed."""
    out = (C.c_int64 * 4)()
    _check("plk_poly_mul_short_plan", lib().plk_poly_mul_short_plan(int(la), int(lb), int(count), out))
    return dict(zip(("per_unit", "units_per_product", "units_per_block", "blocks"), [int(v) for v in out]))


def poly_mul_short_batch(runs):
    """plk_poly_mul_short_batch on host bytes.  A run is (a, b) -- one product -- or (a, la, a_stride, b, lb,
    b_stride, count) over host arrays that hold every operand of the run.  Returns the products in run order,
    trimmed as poly_mul returns them."""
    keep, outs = [], []
    arr = (MulShortRun * max(len(runs), 1))()
    for i, run in enumerate(runs):
        if len(run) == 2:
            a, b = _u8(run[0]).reshape(-1), _u8(run[1]).reshape(-1)
            la, sa, lb, sb, count = a.size, 0, b.size, 0, 1
        else:
            a, la, sa, b, lb, sb, count = run
            a, b = _u8(a).reshape(-1), _u8(b).reshape(-1)
            if count < 1 or la < 1 or lb < 1 or (count - 1) * sa + la > a.size or (count - 1) * sb + lb > b.size:
                raise ValueError("run %d: the arrays do not hold count operands at these strides" % i)
        lo = max(int(la) + int(lb) - 1, 1)
        out = np.zeros(max(int(count), 1) * lo, np.uint8)
        keep += [a, b]
        outs.append((out, lo, int(count)))
        arr[i] = MulShortRun(a.ctypes.data, int(la), int(sa), b.ctypes.data, int(lb), int(sb), out.ctypes.data, lo,
                             int(count))
    total = sum(c for _, _, c in outs)
    lens = (_sz * max(total, 1))()
    _check("plk_poly_mul_short_batch", lib().plk_poly_mul_short_batch(arr, len(runs), lens))
    res, k = [], 0
    for out, lo, count in outs:
        for i in range(count):
            res.append(bytes(out[i * lo:i * lo + lens[k]]))
            k += 1
    return res


def poly_mul_short_batch_dev(runs, nz=None, stream=None):
    """plk_poly_mul_short_batch_dev: runs = MulShortRun structures (mul_short_run) or (a, la, a_stride, b, lb,
    b_stride, out, out_stride, count) tuples over device tensors / raw pointers; nz: one device uint32 word per
    product in run order, or None"""
    arr = (MulShortRun * max(len(runs), 1))()
    for i, r in enumerate(runs):
        if isinstance(r, MulShortRun):
            arr[i] = r
        else:
            a, la, sa, b, lb, sb, out, so, count = r
            arr[i] = MulShortRun(_ptr(a), int(la), int(sa), _ptr(b), int(lb), int(sb), _ptr(out), int(so), int(count))
    _check("plk_poly_mul_short_batch_dev",
           lib().plk_poly_mul_short_batch_dev(arr, len(runs), _ptr(nz), _stream(stream)))


# ---------------------------------------------------------------- device prover
def prove_exit_message(status):
    """the text of a batch entry's status word: what plk_last_error() holds after the single call
    that takes the same exit ('' for 0)"""
    buf = C.create_string_buffer(96)
    rc = lib().plk_prove_exit_message(int(status), buf, len(buf))
    if rc < 0:
        raise ValueError("prove_exit_message: unknown exit in status word 0x%x" % int(status))
    return buf.value.decode()


class Prover:
    """plk_prover_t: plonk_new's setup on the device (SRS + Z_H [+ circuit tables]),
    plonk_prove as `prove` (circuit) or `rounds_dev` (device-resident interpolated polys)."""

    def __init__(self, n, z_h, srs_g1, h=None, k1_h=None, k2_h=None, h_pows_inv=None):
        self._keep = [_u8(x) if x is not None else None for x in (h, k1_h, k2_h, h_pows_inv, z_h, srs_g1)]
        hh, k1, k2, hi, zh, srs = self._keep
        d = PlonkDesc(n, *(None if x is None else _p(x) for x in (hh, k1, k2, hi)), _p(zh), zh.size,
                      _p(srs), srs.size // 3)
        self._h = _vp()
        _check("plk_prover_create", lib().plk_prover_create(C.byref(d), C.byref(self._h)))
        self.n = n

    def close(self):
        if self._h:
            lib().plk_prover_destroy(self._h)
            self._h = _vp()
        self._fixed = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_bytes(self):
        return int(lib().plk_prover_device_bytes(self._h))

    def prove(self, q_m, q_l, q_r, q_o, q_c, copy_a, copy_b, copy_c, a, b, c, chal, rand):
        """copy_*: n (type, index) pairs, flattened or not."""
        arrs = [_u8(x).reshape(-1) for x in (q_m, q_l, q_r, q_o, q_c, copy_a, copy_b, copy_c, a, b, c)]
        cir = Circuit(*(_p(x) for x in arrs))
        ch, rd = _u8(chal), _u8(rand)
        out = np.zeros(34, np.uint8)
        _check("plk_prover_prove", lib().plk_prover_prove(self._h, C.byref(cir), _p(ch), _p(rd), _p(out)))
        return bytes(out)

    # -- many whole proofs per call (plk_prover_prove_batch / plk_prover_rounds_batch)
    def batch_path(self, circuit=True):
        """1: the fused kernel (one launch for the whole batch), 0: one single call per entry"""
        rc = lib().plk_prover_batch_path(self._h, 1 if circuit else 0)
        if rc < 0:
            raise PlonkHipError("plk_prover_batch_path", -rc, last_error())
        return rc

    def _batch_host(self, fn, what, each, data, chals, rands):
        d, ch, rd = _u8(data).reshape(-1), _u8(chals).reshape(-1), _u8(rands).reshape(-1)
        batch = ch.size // 5
        if batch == 0 or ch.size != 5 * batch:
            raise ValueError("%s: chals must hold 5 values per entry (got %d)" % (fn, ch.size))
        if rd.size != 9 * batch:
            raise ValueError("%s: rands must hold 9 values per entry (%d entries, got %d)" % (fn, batch, rd.size))
        if d.size != each * batch:
            raise ValueError("%s: %s must hold %d bytes per entry (%d entries, got %d)" % (fn, what, each, batch, d.size))
        return d, ch, rd, batch, np.zeros(34 * batch, np.uint8), np.zeros(batch, np.uint32)

    def prove_batch(self, circuits, chals, rands):
        """circuits: batch x 14n bytes (q_m q_l q_r q_o q_c | copy_a copy_b copy_c | a b c per entry);
        returns (34 * batch proof bytes, uint32 status per entry: 0 or prove_exit_message's word)"""
        d, ch, rd, batch, out, st = self._batch_host("prove_batch", "circuits", 14 * self.n, circuits, chals, rands)
        _check("plk_prover_prove_batch", lib().plk_prover_prove_batch(
            self._h, _p(d), _p(ch), _p(rd), batch, _p(out), st.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out.tobytes(), st

    def rounds_batch(self, polys, chals, rands, strict=False):
        """polys: batch x 13 x n bytes (rounds_dev's order, zero padded to n); returns as prove_batch"""
        d, ch, rd, batch, out, st = self._batch_host("rounds_batch", "polys", 13 * self.n, polys, chals, rands)
        _check("plk_prover_rounds_batch", lib().plk_prover_rounds_batch(
            self._h, _p(d), _p(ch), _p(rd), PLK_PROVE_STRICT if strict else 0, batch, _p(out),
            st.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out.tobytes(), st

    def _batch_dev(self, fn, batch, sizes):
        if batch <= 0:
            raise ValueError("%s: batch = %d" % (fn, batch))
        for (name, t, per) in sizes:
            if hasattr(t, "numel") and t.numel() * t.element_size() < per * batch:
                raise ValueError("%s: %s holds %d bytes, %d entries need %d" % (fn, name, t.numel() * t.element_size(),
                                                                             batch, per * batch))

    def prove_batch_dev(self, circuits, chals, rands, batch, proofs, status, stream=None):
        """device tensors / pointers: circuits 14n, chals 5, rands 9, proofs 34 bytes per entry, status one
        uint32 each; asynchronous on `stream`, the fused path only"""
        self._batch_dev("prove_batch_dev", batch, (("circuits", circuits, 14 * self.n), ("chals", chals, 5),
                                                               ("rands", rands, 9), ("proofs", proofs, 34),
                                                               ("status", status, 4)))
        _check("plk_prover_prove_batch_dev", lib().plk_prover_prove_batch_dev(
            self._h, _ptr(circuits), _ptr(chals), _ptr(rands), batch, _ptr(proofs), _ptr(status), _stream(stream)))

    def rounds_batch_dev(self, polys, chals, rands, batch, proofs, status, strict=False, stream=None):
        self._batch_dev("rounds_batch_dev", batch, (("polys", polys, 13 * self.n), ("chals", chals, 5),
                                                                ("rands", rands, 9), ("proofs", proofs, 34),
                                                                ("status", status, 4)))
        _check("plk_prover_rounds_batch_dev", lib().plk_prover_rounds_batch_dev(
            self._h, _ptr(polys), _ptr(chals), _ptr(rands), PLK_PROVE_STRICT if strict else 0, batch, _ptr(proofs),
            _ptr(status), _stream(stream)))

    def _args(self, polys, chal, rand):
        """ctypes argument blocks of (polys, chal, rand), cached by value"""
        cache = self.__dict__.setdefault("_argcache", {})
        ch, rd = _u8(chal).reshape(-1), _u8(rand).reshape(-1)
        if ch.size != 5 or rd.size != 9:
            raise ValueError("rounds_dev: chal must hold 5 values and rand 9 (got %d, %d)" % (ch.size, rd.size))
        if len(polys) != 13:
            raise ValueError("rounds_dev: 13 polynomials, got %d" % len(polys))
        key = (tuple(p if isinstance(p, int) else p.data_ptr() for p in polys), ch.tobytes(), rd.tobytes())
        args = cache.get(key)
        if args is None:
            if len(cache) > 64:
                cache.clear()
            args = ((_vp * 13)(*key[0]), (C.c_uint8 * 5).from_buffer_copy(key[1]),
                    (C.c_uint8 * 9).from_buffer_copy(key[2]))
            cache[key] = args
        return args

    def rounds_dev(self, polys, chal, rand, strict=False, preprocessed=False):
        """polys: 13 device tensors / pointers (n bytes each).  preprocessed: use the fixed
        polynomials' transforms from `preprocess` (same addresses, unchanged bytes).  The ctypes
        argument blocks are cached by value (a 2^20-gate proof is ~0.5 ms: building them anew
        each call was ~5 % of it)."""
        args = self._args(polys, chal, rand)
        out = self.__dict__.setdefault("_out", (C.c_uint8 * 34)())
        flags = (PLK_PROVE_STRICT if strict else 0) | (PLK_PROVE_PREPROCESSED if preprocessed else 0)
        _check("plk_prover_rounds_dev", lib().plk_prover_rounds_dev(self._h, args[0], args[1], args[2], flags, out))
        return bytes(out)

    def profile_dev(self, polys, chal, rand, preprocessed=False):
        """plk_prover_profile_dev: (proof bytes, {span_ms, ntt_ms, batch1_ms, batch2_ms}) -- the proof's
        launch sequence and its two product batches (all its NTT pass kernels) timed by hipEvents on the
        prover's stream"""
        args = self._args(polys, chal, rand)
        out = (C.c_uint8 * 34)()
        ms = (C.c_double * 4)()
        flags = PLK_PROVE_PREPROCESSED if preprocessed else 0
        _check("plk_prover_profile_dev",
               lib().plk_prover_profile_dev(self._h, args[0], args[1], args[2], flags, out, ms))
        return bytes(out), dict(zip(("span_ms", "ntt_ms", "batch1_ms", "batch2_ms"), list(ms)))

    def launches(self, polys, chal, rand, preprocessed=False):
        """plk_prover_launches: (kernel launches, other graph nodes) of one proof, counted from a
        captured (never launched) HIP graph of the call"""
        args = self._args(polys, chal, rand)
        k, o = C.c_int(), C.c_int()
        flags = PLK_PROVE_PREPROCESSED if preprocessed else 0
        _check("plk_prover_launches",
               lib().plk_prover_launches(self._h, args[0], args[1], args[2], flags, C.byref(k), C.byref(o)))
        return k.value, o.value

    def alg_bytes(self):
        """plk_prover_alg_bytes: the proof's algorithmic bytes in SURVEY 8(d) terms"""
        return int(lib().plk_prover_alg_bytes(self._h))

    # ---- strong-scaled proof (plk_prover_chains_dev / plk_prover_rounds_ext_dev)
    def chain_bytes(self, chain):
        """buffer size for one chain's product (PLK_CHAIN_T2 or PLK_CHAIN_T3)"""
        return int(lib().plk_prover_chain_bytes(self._h, int(chain)))

    def _check_chain_bufs(self, which, t2, t3):
        """a chain buffer in `which` must be a device tensor of at least chain_bytes on this
        prover's device (an undersized one would be written / read past its end on the GPU);
        raw integer pointers are passed through unchecked"""
        for chain, t in ((PLK_CHAIN_T2, t2), (PLK_CHAIN_T3, t3)):
            if not (int(which) & chain) or t is None or isinstance(t, int):
                continue
            need = self.chain_bytes(chain)
            have = t.numel() * t.element_size()
            if have < need:
                raise ValueError("chain %d buffer holds %d bytes, chain_bytes is %d" % (chain, have, need))
            if not t.is_cuda:
                raise ValueError("chain %d buffer is not a device tensor" % chain)
            dev = getattr(self, "device", None)
            if dev is not None and t.device.index != dev:
                raise ValueError("chain %d buffer is on device %s, the prover on %d" % (chain, t.device, dev))

    def chains_dev(self, polys, chal, rand, which, t2=None, t3=None, done=None):
        """Helper GPU: enqueue the preparation and the chains in `which` (PLK_CHAIN_* mask) into
        the device buffers t2 / t3 (chain_bytes each); stream `done` (None: the null stream,
        torch's default) waits for them."""
        self._check_chain_bufs(which, t2, t3)
        args = self._args(polys, chal, rand)
        _check("plk_prover_chains_dev", lib().plk_prover_chains_dev(
            self._h, args[0], args[1], args[2], int(which), _ptr(t2) if t2 is not None else None,
            _ptr(t3) if t3 is not None else None, _stream(done)))

    def rounds_ext_dev(self, polys, chal, rand, which, t2=None, t3=None, ready=None, strict=False,
                       preprocessed=False):
        """rounds_dev with the chains in `which` read from t2 / t3 (computed by chains_dev on
        another GPU from the same inputs) once everything enqueued on stream `ready` (None: the
        null stream) so far has run.  Same 34 bytes as rounds_dev."""
        self._check_chain_bufs(which, t2, t3)
        args = self._args(polys, chal, rand)
        out = (C.c_uint8 * 34)()
        flags = (PLK_PROVE_STRICT if strict else 0) | (PLK_PROVE_PREPROCESSED if preprocessed else 0)
        _check("plk_prover_rounds_ext_dev", lib().plk_prover_rounds_ext_dev(
            self._h, args[0], args[1], args[2], flags, int(which), _ptr(t2) if t2 is not None else None,
            _ptr(t3) if t3 is not None else None, _stream(ready), out))
        return bytes(out)

    # ---- the same split from C over the plk_init_devices list (plk_prover_attach_helpers)
    def attach_helpers(self, k):
        """k helper provers on entries 1..k of the plk_init_devices list (0 detaches); from then on
        rounds_dev / prove run split (the chains on the helpers, products peer-copied back)"""
        _check("plk_prover_attach_helpers", lib().plk_prover_attach_helpers(self._h, int(k)))

    def helpers(self):
        return int(lib().plk_prover_helpers(self._h))

    def rounds_multi_dev(self, poly_sets, chal, rand, strict=False, preprocessed=False):
        """poly_sets: 1 + helpers() lists of 13 device tensors, set h on helper h's device"""
        ch, rd = _u8(chal).reshape(-1), _u8(rand).reshape(-1)
        if ch.size != 5 or rd.size != 9:
            raise ValueError("rounds_multi_dev: chal must hold 5 values and rand 9")
        flat = [p for ps in poly_sets for p in ps]
        if any(len(ps) != 13 for ps in poly_sets):
            raise ValueError("rounds_multi_dev: 13 polynomials per set")
        arr = (_vp * len(flat))(*[_ptr(p) for p in flat])
        out = (C.c_uint8 * 34)()
        flags = (PLK_PROVE_STRICT if strict else 0) | (PLK_PROVE_PREPROCESSED if preprocessed else 0)
        _check("plk_prover_rounds_multi_dev", lib().plk_prover_rounds_multi_dev(
            self._h, arr, len(poly_sets), _p(ch), _p(rd), flags, out))
        return bytes(out)

    def preprocess(self, polys):
        """plk_prover_preprocess: the round-3 transforms of q_o q_m q_l q_r s_sigma_3 l_1_x
        (entries 3 4 5 6 10 12 of the 13 device polys); None drops them."""
        arr = None if polys is None else (_vp * 13)(*[_ptr(p) for p in polys])
        # the transforms are bound to these device addresses: hold the tensors so the caching
        # allocator cannot hand the same addresses to another circuit's polynomials
        self._fixed = None
        _check("plk_prover_preprocess", lib().plk_prover_preprocess(self._h, arr))
        self._fixed = None if polys is None else list(polys)
