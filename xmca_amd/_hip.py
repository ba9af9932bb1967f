"""ctypes binding of libxmca_hip.so (C ABI: include/xmca_hip.h).

The product path has no CPU fallback: importing this module without the built
library, or creating a handle without a visible MI355X, raises.
"""
import ctypes
import weakref
import ctypes.util
import os

import numpy as np

from . import build as _build

XMCA_F32, XMCA_F64 = 0, 1
HOST, DEVICE = 0, 1

ERR_INVALID, ERR_HIP, ERR_NOT_CONVERGED, ERR_STATE, ERR_UNSUPPORTED, ERR_NUMERIC = -1, -2, -3, -4, -5, -6

_c_i64 = ctypes.c_int64
_c_int = ctypes.c_int
_c_dbl = ctypes.c_double
_vp = ctypes.c_void_p
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)

# name -> (restype, argtypes); the ABI test checks every one of these is exported
SIGNATURES = {
    "xmca_version": (ctypes.c_char_p, []),
    "xmca_abi_version": (_c_int, []),
    "xmca_device_count": (_c_int, []),
    "xmca_create": (_c_int, [_c_int, ctypes.POINTER(_vp)]),
    "xmca_destroy": (None, [_vp]),
    "xmca_last_error": (ctypes.c_char_p, [_vp]),
    "xmca_set_field": (_c_int, [_vp, _c_int, _vp, _vp, _c_i64, _c_i64, _c_int, _c_int]),
    "xmca_set_field_strided": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int]),
    "xmca_ingest_regime": (_c_int, [_c_i64, _c_i64, _c_i64, _c_i64]),
    "xmca_complexify": (_c_int, [_vp, _vp]),
    "xmca_complexify_extended": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_int]),
    "xmca_complexify_theta": (_c_int, [_vp, _vp, _vp, _vp, _c_int]),
    "xmca_theta_fit": (_c_int, [_vp, _c_int, _c_int, _vp]),
    "xmca_get_field_imag": (_c_int, [_vp, _c_int, _vp]),
    "xmca_solve": (_c_int, [_vp, _c_int, _c_i64, ctypes.POINTER(_c_i64)]),
    "xmca_get_singular_values": (_c_int, [_vp, _vp, _c_i64]),
    "xmca_get_vectors": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_int]),
    "xmca_get_eofs": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_i64, _c_int, _vp, _c_int]),
    "xmca_get_maps": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_i64, _c_int, _vp, _c_int, _vp, _c_i64, _c_int, _c_int, _vp, _c_int, _vp]),
    "xmca_get_maps_to": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_i64, _c_int, _vp, _c_int, _vp, _c_i64, _c_int, _c_int, _vp, _c_int, _vp,
                                  _c_int]),
    "xmca_center_field": (_c_int, [_vp, _c_int, _vp, _vp, ctypes.POINTER(_c_i64)]),
    "xmca_compact_field": (_c_int, [_vp, _c_int, _vp, ctypes.POINTER(_c_i64)]),
    "xmca_scale_field": (_c_int, [_vp, _c_int, _vp, _c_int]),
    "xmca_get_field": (_c_int, [_vp, _c_int, _vp]),
    "xmca_bootstrap_begin": (_c_int, [_vp, _c_int]),
    "xmca_bootstrap_runs": (_c_int, [_vp, _vp, _vp, _vp, _c_i64, _c_int, _c_int, _c_int, _c_dbl, _vp, _vp, _c_i64]),
    "xmca_bootstrap_runs_extended": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_int, _vp, _vp, _c_i64, _c_int, _c_int, _c_int, _c_dbl, _vp, _vp,
                                              _c_i64]),
    "xmca_bootstrap_runs_columns": (_c_int, [_vp, _vp, _vp, _vp, _c_i64, _c_int, _c_int, _c_int, _c_dbl, _vp, _vp, _c_i64]),
    "xmca_bootstrap_runs_columns_extended": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_int, _vp, _vp, _c_i64, _c_int, _c_int, _c_int, _c_dbl,
                                                      _vp, _vp, _c_i64]),
    "xmca_bootstrap_runs_theta": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _vp, _vp, _c_i64, _c_int, _c_int, _c_int, _c_dbl, _vp, _vp, _c_i64]),
    "xmca_bootstrap_runs_columns_theta": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _vp, _vp, _c_i64, _c_int, _c_int, _c_int, _c_dbl, _vp, _vp,
                                                   _c_i64]),
    "xmca_bootstrap_patterns": (_c_int, [_vp, _vp, _vp, _c_i64, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "xmca_pattern_stats": (_c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _c_int, _c_i64, _c_i64, _c_int, _c_int, _c_int,
                                    _vp, _vp, _vp, _vp, _vp]),
    "xmca_pattern_tile": (_c_int, []),
    "xmca_extended_eofs": (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _c_i64, _vp, _vp, _vp]),
    "xmca_lag_gram": (_c_int, [_vp, _vp, _c_i64, _c_int, _c_int, _c_int, _vp]),
    "xmca_lag_gram_tile": (_c_int, []),
    "xmca_extended_reconstruct": (_c_int, [_vp, _c_int, _c_int, _vp, _c_int, _c_int, _vp, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _c_int]),
    "xmca_lag_expand": (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp]),
    "xmca_lag_window_means": (_c_int, [_vp, _c_int, _c_int, _vp]),
    "xmca_extended_rule_n": (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _c_i64, _c_i64, ctypes.c_uint64, _vp, _vp, _vp]),
    "xmca_extended_project": (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _c_int, _vp]),
    "xmca_lag_project": (_c_int, [_vp, _vp, _c_i64, _c_int, _c_int, _c_int, _vp]),
    "xmca_lag_project_tile": (_c_int, [_ip, _ip]),
    "xmca_fill_gaps": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_int, _vp, _c_i64, _c_int, _c_int, _c_dbl, _vp, _vp, _ip, _dp, _vp]),
    "xmca_gap_center": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_int, _vp, _vp, _vp, _dp]),
    "xmca_gap_fill_step": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_i64, _c_i64, _c_int, _c_int, _vp, _dp]),
    "xmca_gap_fill_tile": (_c_int, [_ip, _ip]),
    "xmca_fill_gaps_lagged": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_int, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_dbl, _vp, _vp, _ip,
                                       _dp, _vp]),
    "xmca_gap_lag_fill_step": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_int, _vp, _dp]),
    "xmca_column_regress": (_c_int, [_vp, _vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _vp, _c_int, _vp, _c_int, _vp, _vp]),
    "xmca_column_residual": (_c_int, [_vp, _vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _vp, _c_int, _vp, _vp, _c_int]),
    "xmca_reg_mask": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_int, _vp, _vp, ctypes.POINTER(_c_i64)]),
    "xmca_reg_solve": (_c_int, [_vp, _vp, _c_int, _vp, _c_i64, _c_int, _vp, _vp]),
    "xmca_reg_residual_tile": (_c_int, [_ip, _ip]),
    "xmca_time_filter": (_c_int, [_vp, _vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _vp, _c_int, _c_int, _c_int, _c_dbl, _c_int, _vp,
                                  _c_int]),
    "xmca_time_filter_tile": (_c_int, [_ip, _ip, _ip]),
    "xmca_lead_lag_maps": (_c_int, [_vp, _vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _vp, _c_int, _vp, _c_int, _c_int, _c_int, _vp, _vp,
                                    _vp, _vp, _vp, _vp, _vp, _c_int]),
    "xmca_lead_lag_tile": (_c_int, [_ip, _ip, _ip]),
    "xmca_spectral_maps": (_c_int, [_vp, _vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _vp, _c_int, _c_int, _c_int, _vp, _c_int, _vp, _c_int,
                                    _c_dbl, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int]),
    "xmca_spectral_tile": (_c_int, [_ip, _ip, _ip]),
    "xmca_correlate": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_i64, _vp]),
    "xmca_pearson_pvalues": (_c_int, [_vp, _vp, _c_i64, _c_i64, _vp]),
    "xmca_pvalue_log_norm": (_c_int, [_c_i64, _dp]),
    "xmca_correlation_maps": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_i64, _vp, _c_i64, _c_int, _vp, _vp]),
    "xmca_correlation_maps_to": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_i64, _vp, _c_i64, _c_int, _vp, _vp, _c_int]),
    "xmca_project": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_i64, _c_int, _vp, ctypes.POINTER(_c_int)]),
    "xmca_predict": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_i64, _c_int, _vp, _c_i64, _vp, _vp, _vp, _c_int, _vp, _c_i64, _c_i64, _c_int,
                              _vp, ctypes.POINTER(_c_int)]),
    "xmca_reconstruct": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_i64, _c_int, _vp, _c_int, _vp, _c_i64, _c_i64, _vp, _vp, _vp]),
    "xmca_predict_weighted": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_i64, _c_int, _vp, _c_i64, _vp, _vp, _vp, _c_int, _vp, _c_i64, _c_i64,
                                       _c_int, _vp, ctypes.POINTER(_c_int), _vp]),
    "xmca_reconstruct_weighted": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_i64, _c_int, _vp, _c_int, _vp, _c_i64, _c_i64, _vp, _vp, _vp, _vp]),
    "xmca_predict_strided": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _vp, _c_i64, _vp, _vp, _vp, _c_int,
                                      _vp, _c_i64, _c_i64, _c_int, _vp, ctypes.POINTER(_c_int), _vp]),
    "xmca_reconstruct_to": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_i64, _c_int, _vp, _c_int, _vp, _c_i64, _c_i64, _vp, _vp, _vp, _vp,
                                     _c_int]),
    "xmca_is_complex": (_c_int, [_vp]),
    "xmca_vectors_are_f32": (_c_int, [_vp, _c_int]),
    "xmca_persistent_giveups": (ctypes.c_longlong, []),
    "xmca_get_solve_info": (_c_int, [_vp, _vp, _c_int]),
    "xmca_rotate_loadings": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_dbl, _c_int, _c_int, _c_dbl,
                                      _vp, _vp, _vp, _vp, _vp, _ip]),
    "xmca_rotate_solved": (_c_int, [_vp, _c_int, _c_int, _c_dbl, _c_int, _vp, _vp, _vp, _vp, _ip]),
    "xmca_rule_n": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _c_int, _vp, _c_int, _c_int, _c_int, _c_dbl, _c_i64, _c_i64,
                             ctypes.c_uint64, _c_int, _vp, _vp, _c_i64]),
    "xmca_comm_unique_id": (_c_int, [_vp]),
    "xmca_comm_create": (_c_int, [_vp, _vp, _c_int, _c_int, ctypes.POINTER(_vp)]),
    "xmca_comm_destroy": (None, [_vp]),
    "xmca_comm_last_error": (ctypes.c_char_p, [_vp]),
    "xmca_comm_allgather": (_c_int, [_vp, _vp, _vp, _c_i64]),
    "xmca_comm_broadcast": (_c_int, [_vp, _vp, _c_i64, _c_int]),
    "xmca_comm_info": (_c_int, [_vp, _ip, _ip, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64)]),
    "xmca_rule_n_sharded": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _vp, _c_int, _c_int, _c_int, _c_dbl,
                                     ctypes.c_uint64, _c_int, _vp, _vp, _c_i64]),
    "xmca_surrogate": (_c_int, [_vp, _c_i64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp]),
    "xmca_lag1_autocorrelation": (_c_int, [_vp, _c_int, _vp]),
    "xmca_rule_n_ar1": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _c_int, _vp, _c_int, _c_int, _c_int, _c_dbl, _c_i64, _c_i64,
                                 ctypes.c_uint64, _c_int, _vp, _vp, _c_i64, _vp, _vp]),
    "xmca_rule_n_ar1_sharded": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _vp, _c_int, _c_int, _c_int, _c_dbl,
                                         ctypes.c_uint64, _c_int, _vp, _vp, _c_i64, _vp, _vp]),
    "xmca_surrogate_ar1": (_c_int, [_vp, _c_i64, _c_i64, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _c_int, _vp]),
    "xmca_ar1_segments": (_c_int, [_c_i64, _c_i64, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64)]),
    "xmca_get_timings": (_c_int, [_vp, ctypes.c_char_p, _c_int, _vp, _c_int]),
    "xmca_get_reduction_info": (_c_int, [_vp, ctypes.c_char_p, _c_int]),
    "xmca_reset_timings": (_c_int, [_vp]),
    "xmca_fft": (_c_int, [_vp, _vp, _vp, _c_int, _c_int, _c_int, _vp, _vp]),
    "xmca_pool_bytes": (_c_int, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    "xmca_trim_pool": (_c_int, [_vp]),
    "xmca_gemm": (_c_int, [_vp, _vp, _c_i64, _c_int, _vp, _c_i64, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_dbl,
                           _c_int, _c_int, _c_int]),
    "xmca_gemm_ex": (_c_int, [_vp, _vp, _c_i64, _c_int, _vp, _c_i64, _c_int, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int,
                              _c_dbl, _c_dbl, _vp, _vp, _c_int, _c_int, _c_int]),
    "xmca_eigh": (_c_int, [_vp, _vp, _c_int, _c_int, _vp, _vp, _vp]),
    "xmca_eigh_lead": (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _vp, _vp, _vp]),
    "xmca_partial_count": (_c_int, [_vp, _c_int, _c_int, _vp]),
    "xmca_cholesky": (_c_int, [_vp, _vp, _c_int, _c_int, _c_dbl, _vp, ctypes.POINTER(_c_int)]),
    "xmca_cholesky_ex": (_c_int, [_vp, _vp, _c_int, _c_i64, _c_int, _c_int, _c_dbl, _vp, ctypes.POINTER(_c_int)]),
    "xmca_lead_rows": (_c_int, [_vp, _vp, _c_i64, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _c_i64, ctypes.POINTER(_c_int)]),
    "xmca_fft_ex": (_c_int, [_vp, _vp, _vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _vp, _c_int, _c_int, _c_int, _vp, _vp, _c_i64,
                             _c_i64, _c_i64, _c_int, _vp, _vp, _c_dbl]),
    "xmca_tridiag_eigenvalues": (_c_int, [_vp, _vp, _vp, _c_int, _vp]),
    "xmca_tridiag_vectors": (_c_int, [_vp, _vp, _vp, _c_int, _vp, _c_int, _vp, _c_i64]),
    "xmca_bench_gram": (_c_int, [_vp, _c_int, _c_int, _dp, _dp, _dp]),
    "xmca_bench_gemm": (_c_int, [_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _dp]),
}

_lib = None


def library_path():
    return _build.LIB


MAP_EOF, MAP_AMPLITUDE, MAP_PHASE = 0, 1, 2          # `kind` of xmca_get_maps
SCALE_NONE, SCALE_MAX, SCALE_STD = 0, 1, 2           # ... and its `scaling`
INGEST_ROWS, INGEST_TRANSPOSE, INGEST_GATHER = 0, 1, 2   # regimes of xmca_set_field_strided (xmca_ingest_regime)
DOF_N, DOF_BRETHERTON = 0, 1                         # `dof_mode` of xmca_lead_lag_maps
DETREND_NONE, DETREND_MEAN = 0, 1                    # `detrend` of xmca_spectral_maps
PVALUE_MAX_OBS = 1000000    # largest n_obs of xmca_pearson_pvalues / xmca_correlation_maps (csrc/kernels.h)
ABI_VERSION = 16        # bumped whenever a signature of include/xmca_hip.h changes; checked against xmca_abi_version()


def load_library():
    """Loads libxmca_hip.so and binds every symbol of include/xmca_hip.h.  The library is never built implicitly
    (`python -m xmca_amd.build` / `__graft_entry__.build()` do that); a missing library, a missing symbol or a library
    built from an older header (ABI number) raises ImportError - there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            "xmca_amd: %s is missing. Build it with `python -m xmca_amd.build` (needs hipcc, "
            "--offload-arch=gfx950). There is no CPU fallback." % path)
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as err:
            raise ImportError("xmca_amd: %s does not export %s - rebuild it with `python -m xmca_amd.build --force`"
                              % (path, name)) from err
        fn.restype = res
        fn.argtypes = args
    have = lib.xmca_abi_version()
    if have != ABI_VERSION:
        raise ImportError("xmca_amd: %s was built for ABI %d, this package binds ABI %d - rebuild it with "
                          "`python -m xmca_amd.build --force`" % (path, have, ABI_VERSION))
    _lib = lib
    return lib


def pvalue_log_norm(n_obs):
    """-ln a - ln B(a, a) for a = n_obs / 2 - 1: the per-call constant of the p-value kernel (xmca_pvalue_log_norm; no device)."""
    out = _c_dbl(0)
    rc = load_library().xmca_pvalue_log_norm(int(n_obs), ctypes.byref(out))
    if rc != 0:
        raise ValueError("pvalue_log_norm: n_obs must be between 3 and 1 000 000")
    return out.value


def partial_count(lam_desc, n_lead):
    """(k', repeated): the number of eigenvectors the partial route of the eigensolver forms for `n_lead` wanted ones, given all
    eigenvalues in descending order (n: all of them), and whether bit-equal leading values send the solve to the Jacobi sweeps
    (xmca_partial_count; no device)."""
    lam = np.ascontiguousarray(lam_desc, dtype=np.float64)
    rep = _c_int(0)
    kp = load_library().xmca_partial_count(_ptr(lam), int(lam.size), int(n_lead), ctypes.byref(rep))
    if kp < 0:
        raise ValueError("partial_count: at least one eigenvalue is needed")
    return kp, bool(rep.value)


def ingest_regime(T, N, stride_t, stride_n):
    """The copy kernel `xmca_set_field_strided` takes for a T x N view with these element strides: INGEST_ROWS (contiguous rows),
    INGEST_TRANSPOSE (time is the fast axis) or INGEST_GATHER (xmca_ingest_regime; no device)."""
    rc = load_library().xmca_ingest_regime(int(T), int(N), int(stride_t), int(stride_n))
    if rc < 0:
        raise ValueError("ingest_regime: a non-empty view with strides >= 0 is needed")
    return rc


def ar1_segments(T, N):
    """The time segments [(begin, end), ...] of the AR(1) filter of a T x N surrogate (xmca_ar1_segments; no device): a function of
    the shape alone, so the red-noise surrogates do not depend on lanes, ranks or the load of the device."""
    count, length = _c_i64(0), _c_i64(0)
    rc = load_library().xmca_ar1_segments(int(T), int(N), ctypes.byref(count), ctypes.byref(length))
    if rc != 0:
        raise ValueError("ar1_segments: T and N must be >= 1")
    return [(k * length.value, min(int(T), (k + 1) * length.value)) for k in range(count.value)]


def pattern_tile():
    """Columns per partial sum of the alignment of `bootstrap_patterns` (xmca_pattern_tile; no device): a constant of the build."""
    return int(load_library().xmca_pattern_tile())


def lag_gram_tile():
    """Output tile edge of the lag-sum kernel of `extended_eofs` (xmca_lag_gram_tile; no device): a constant of the build."""
    return int(load_library().xmca_lag_gram_tile())


def lag_project_tile():
    """(rows, columns) of Q one workgroup of the projection kernels of `extended_rule_n` handles (xmca_lag_project_tile; no
    device): constants of the build."""
    rows, cols = _c_int(0), _c_int(0)
    load_library().xmca_lag_project_tile(ctypes.byref(rows), ctypes.byref(cols))
    return int(rows.value), int(cols.value)


def gap_fill_tile():
    """(rows, columns) of a tile of the fill kernel of `fill_gaps` (xmca_gap_fill_tile; no device): constants of the build."""
    rows, cols = _c_int(0), _c_int(0)
    load_library().xmca_gap_fill_tile(ctypes.byref(rows), ctypes.byref(cols))
    return int(rows.value), int(cols.value)


def reg_residual_tile():
    """(rows, columns) of a tile of the residual kernel of `anomalies` (xmca_reg_residual_tile; no device): constants of the build."""
    rows, cols = _c_int(0), _c_int(0)
    load_library().xmca_reg_residual_tile(ctypes.byref(rows), ctypes.byref(cols))
    return int(rows.value), int(cols.value)


def time_filter_tile():
    """(rows, columns, most weights): the output rows and columns of a workgroup's tile of the filter kernel of `time_filter` and the
    longest filter it takes (xmca_time_filter_tile; no device): constants of the build."""
    rows, cols, most = _c_int(0), _c_int(0), _c_int(0)
    load_library().xmca_time_filter_tile(ctypes.byref(rows), ctypes.byref(cols), ctypes.byref(most))
    return int(rows.value), int(cols.value), int(most.value)


def lead_lag_tile():
    """(columns, rows, groups): the columns of a workgroup of the moment kernel of `lead_lag_maps`, the rows of a piece a lane loads
    together, and groups[q - 1], q = 1 .. 8, the lags of a workgroup's group with q index series (xmca_lead_lag_tile; no device)."""
    cols, rows = _c_int(0), _c_int(0)
    groups = (_c_int * 8)()
    load_library().xmca_lead_lag_tile(ctypes.byref(cols), ctypes.byref(rows), groups)
    return int(cols.value), int(rows.value), tuple(int(g) for g in groups)


def spectral_tile():
    """(columns, rows, groups): the columns of a workgroup of the segment kernel of `spectral_maps`, the rows of a piece a lane loads
    together, and groups[q], q = 0 .. 4, the bins of a workgroup's group with q index series (xmca_spectral_tile; no device)."""
    cols, rows = _c_int(0), _c_int(0)
    groups = (_c_int * 5)()
    load_library().xmca_spectral_tile(ctypes.byref(cols), ctypes.byref(rows), groups)
    return int(cols.value), int(rows.value), tuple(int(g) for g in groups)


def _gap_plane(what, X):
    """A field with gaps as a contiguous 2-D float32 / float64 array."""
    X = np.asarray(X)
    if X.ndim != 2 or X.dtype not in (np.float32, np.float64):
        raise ValueError("%s: need a T x N float32 or float64 array, got %s of shape %s" % (what, X.dtype, X.shape))
    return np.ascontiguousarray(X)


def _mode_major_planes(what, V, k, cplx):
    """The vectors of one field, N x k (or None), as the contiguous float64 planes k x N the pattern entries read: (re, im or None, N)."""
    if V is None:
        return None, None, 0
    V = np.asarray(V)
    if V.ndim != 2 or V.shape[1] != k or V.shape[0] < 1:
        raise ValueError("%s: the vectors of a field must be N x %d, got shape %s" % (what, k, V.shape))
    if np.iscomplexobj(V) and not cplx:
        raise ValueError("%s: complex vectors for a real model" % what)
    re = np.ascontiguousarray(V.real.T, dtype=np.float64)
    im = np.ascontiguousarray(V.imag.T, dtype=np.float64) if cplx else None
    return re, im, V.shape[0]


def _phi_array(what, phi, N):
    """The lag-1 autocorrelations of N columns as contiguous float64: finite, |phi| < 1 (checked here, before any device call)."""
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    if phi.shape != (int(N),):
        raise ValueError("%s: phi must hold one value per column (%d), got shape %s" % (what, N, phi.shape))
    if not np.all(np.abs(phi) < 1.0):                   # (False for NaN)
        raise ValueError("%s: every phi must be finite with |phi| < 1" % what)
    return phi


def _phi_pair(what, ar1, Nx, Ny, n_fields):
    """`ar1 = (phi_left, phi_right or None)` of rule_n / rule_n_sharded as two checked arrays (the right one None for one field)."""
    try:
        left, right = ar1
    except (TypeError, ValueError):
        raise ValueError("%s: ar1 must be the pair (phi_left, phi_right or None)" % what)
    if (right is not None) != (n_fields == 2):
        raise ValueError("%s: ar1 needs a phi for each of the %d field(s), and none for a field the model lacks" % (what, n_fields))
    return _phi_array(what, left, Nx), None if right is None else _phi_array(what, right, Ny)


class DeviceView:
    """A real T x N view of memory on a handle's GPU: element (t, n) at `ptr` + (t * stride_t + n * stride_n) elements of `dtype`
    (float32 / float64).  `owner` keeps the memory alive (a tensor); the library only ever reads it."""

    def __init__(self, ptr, T, N, stride_t, stride_n, dtype, owner=None):
        self.ptr, self.T, self.N = int(ptr), int(T), int(N)
        self.stride_t, self.stride_n = int(stride_t), int(stride_n)
        self.dtype = np.dtype(dtype)
        self.owner = owner
        self.shape = (self.T, self.N)
        if self.dtype not in (np.float32, np.float64):
            raise TypeError("DeviceView: float32 / float64 only, got %s" % self.dtype)
        if self.stride_t < 0 or self.stride_n < 0:
            raise ValueError("DeviceView: negative strides are not supported")


class HipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(message)
        self.code = code


def _raise(code, message):
    if code == ERR_INVALID:
        raise ValueError(message)
    if code == ERR_NOT_CONVERGED:
        raise RuntimeError(message)
    if code == ERR_UNSUPPORTED:
        raise NotImplementedError(message)
    if code == ERR_NUMERIC:
        raise np.linalg.LinAlgError(message)
    raise HipError(code, message)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _np_dtype_code(dt):
    dt = np.dtype(dt)
    if dt in (np.float32, np.complex64):
        return XMCA_F32
    if dt in (np.float64, np.complex128):
        return XMCA_F64
    raise TypeError("unsupported dtype %s (float32 / float64 / complex64 / complex128 only)" % dt)


def _real_np(code):
    return np.float32 if code == XMCA_F32 else np.float64


def _cplx_np(code):
    return np.complex64 if code == XMCA_F32 else np.complex128


def _host_vectors(V):
    """A maybe-complex host array as contiguous float64 / complex128 -> (array or None, is complex)."""
    if V is None:
        return None, False
    V = np.asarray(V)
    cplx = np.iscomplexobj(V)
    return np.ascontiguousarray(V, dtype=np.complex128 if cplx else np.float64), cplx


def _column_weights(what, w, N):
    """Per-column weights of the weighted transforms as N contiguous float64 values (the device reads exactly N)."""
    w = np.asarray(w)
    if np.iscomplexobj(w) or w.shape != (N,):
        raise ValueError("%s: the weights must be %d real values, one per kept column, got shape %s" % (what, N, w.shape))
    return np.ascontiguousarray(w, dtype=np.float64)


def _kept_index(what, keep_idx, N=None):
    """The kept columns as contiguous int64 indices (None: all are kept); `N`: how many there must be, where the caller knows."""
    idx = None if keep_idx is None else np.ascontiguousarray(keep_idx, dtype=np.int64)
    if idx is not None and N is not None and idx.shape != (int(N),):
        raise ValueError("%s: keep_idx must hold one index per kept point (%d), got shape %s" % (what, N, idx.shape))
    return idx


def _output(alloc, shape, dtype):
    """(array, pointer argument, XMCA_HOST / XMCA_DEVICE) of a result: a new host array, or what `alloc(shape, dtype)` made on the
    handle's GPU - `(array, device address)`."""
    if alloc is None:
        out = np.empty(shape, dtype=dtype)
        return out, _ptr(out), HOST
    out, address = alloc(shape, np.dtype(dtype))
    return out, _vp(int(address)), DEVICE


def _unpack(out, rows, cols, is_complex):
    """The (rows, cols) result written into the complex128 buffer `out`: as it is, or its leading float64 values."""
    if is_complex:
        return out
    return out.view(np.float64).reshape(-1)[:rows * cols].reshape(rows, cols).copy()


def hilbert_imag_column(T):
    """First column of the imaginary part of the analytic-signal operator of scipy.signal.hilbert (axis 0).

    hilbert(x) = ifft(fft(x) * h) with h = [1, 2, ..., 2, (1), 0, ...]; its imaginary part acts on a real x as the
    real circulant matrix Ht[t, s] = col[(t - s) mod T] with col = imag(ifft(h)).
    """
    h = np.zeros(T)
    if T % 2 == 0:
        h[0] = h[T // 2] = 1.0
        h[1:T // 2] = 2.0
    else:
        h[0] = 1.0
        h[1:(T + 1) // 2] = 2.0
    return np.ascontiguousarray(np.fft.ifft(h).imag)


def hilbert_imag_operator(T):
    """The full T x T operator (tests / documentation)."""
    col = hilbert_imag_column(T)
    idx = (np.arange(T)[:, None] - np.arange(T)[None, :]) % T
    return np.ascontiguousarray(col[idx])


def extended_imag_parts(T, period):
    """O(T) parts of the imaginary operator G of the fore/back-cast analytic signal (extend='exp', xmca/array.py:378-472).

    For `extend='exp'` the reference's `_complexify` is linear in the column and the same for every column: `_get_reg_coefs`
    divides by the constant `mean(x)`, so the forecast of a series y is y[T-1] e + ymean (1 - e) + s (t + tc - tc e) with
    e_t = exp(-(t + 1) / period), tc = (T - 1) / 2 and s = sum (t - tc) y_t / (T tc^2); the backcast is the same map of the
    reversed series.  After `hilbert` of the 3T-long series, the trim to [T, 2T) and `remove_mean`, a centered field X becomes
    X + i G X with

        G = P (H3[T:2T, T:2T] + U W^T),   P = I - 1 1^T / T,

    H3 the circulant imaginary operator of `hilbert` at length 3T and U W^T of rank 4: the extensions see a column only through
    W^T y = (mean, s, y_0, y_{T-1}).  Returned (float64, nothing of size T x T):

      col3   (3T,)   first column of H3: H3[T + t, T + s] = col3[(t - s) mod 3T]
      hbar   (T,)    column means of the middle block, hbar[s] = mean_t col3[(t - s) mod 3T]
      U      (T, 4)  P applied to the four images H3[T:2T, :] [backcast; 0; forecast] of the functionals
      W      (T, 4)  the functionals

    so that G[t, s] = col3[(t - s) mod 3T] - hbar[s] + sum_k U[t, k] W[s, k]."""
    T = int(T)
    if T < 2:
        raise ValueError("extend='exp' needs at least 2 time steps")
    period = float(period)
    t = np.arange(T, dtype=np.float64)
    tc = (T - 1) / 2.0
    e = np.exp(-(t + 1.0) / period)
    W = np.empty((T, 4))
    W[:, 0] = 1.0 / T                               # ymean
    W[:, 1] = (t - tc) / (T * tc * tc)              # slope s
    W[:, 2] = 0.0
    W[0, 2] = 1.0                                   # y_0 (last point of the reversed series)
    W[:, 3] = 0.0
    W[T - 1, 3] = 1.0                               # y_{T-1}
    # coefficients of the four functionals in the forecast `post` (rows t) and the backcast `pre` (pre[t] = f_rev[T-1-t])
    post = np.stack([1.0 - e, t + tc - tc * e, np.zeros(T), e], axis=1)
    pre = np.stack([1.0 - e, -(t + tc - tc * e), e, np.zeros(T)], axis=1)[::-1]
    col3 = hilbert_imag_column(3 * T)
    h3 = np.zeros(3 * T)
    if T % 2 == 0:                                  # 3T even
        h3[0] = h3[3 * T // 2] = 1.0
        h3[1:3 * T // 2] = 2.0
    else:
        h3[0] = 1.0
        h3[1:(3 * T + 1) // 2] = 2.0
    ext = np.zeros((3 * T, 4))
    ext[:T] = pre
    ext[2 * T:] = post
    U = np.fft.ifft(np.fft.fft(ext, axis=0) * h3[:, None], axis=0).imag[T:2 * T]
    U = np.ascontiguousarray(U - U.mean(axis=0))
    # hbar[s] = (1/T) sum_{d = -s}^{T-1-s} col3[d mod 3T]: a sliding window over col3[-(T-1):] ++ col3[:T]
    win = np.concatenate([col3[2 * T + 1:], col3[:T]])
    cs = np.concatenate([[0.0], np.cumsum(win)])
    s = np.arange(T)
    hbar = (cs[2 * T - 1 - s] - cs[T - 1 - s]) / T
    return np.ascontiguousarray(col3), np.ascontiguousarray(hbar), U, np.ascontiguousarray(W)


def _hilbert_weights(n):
    """The frequency weights of scipy.signal.hilbert at length n."""
    h = np.zeros(n)
    if n % 2 == 0:
        h[0] = h[n // 2] = 1.0
        h[1:n // 2] = 2.0
    else:
        h[0] = 1.0
        h[1:(n + 1) // 2] = 2.0
    return h


def theta_forecast_basis(T, period):
    """(T, 2 + period) basis F of the Theta forecast of a column of length T: the columns 1, h and the indicators of
    (T + h) mod period == p, so that the forecast is F c with c = (level + 0.95 b0 (1 - (1 - alpha)^T) / alpha, 0.95 b0, s_0 ..)."""
    h = np.arange(T)
    F = np.zeros((T, 2 + period))
    F[:, 0] = 1.0
    F[:, 1] = h
    F[h, 2 + (T + h) % period] = 1.0
    return F


def theta_imag_parts(T, period):
    """O(T period) parts of the imaginary planes of the Theta fore/back-cast analytic signal (extend='theta', xmca/array.py:367-376,
    :429-472).  The forecast of a column is not linear in it, but it is F c with the 2 + period fitted coefficients c of the column
    (`theta_forecast_basis`), and the backcast F[::-1] c' with those of the reversed column.  After `hilbert` at length 3T, the trim to
    [T, 2T) and `remove_mean` a centered field X becomes X + i (G0 X + B C) with

      col3, hbar  the operator G0[t, s] = col3[(t - s) mod 3T] - hbar[s] of `extended_imag_parts` at rank 0
      B  (T, 2 (2 + period))   the centered images H3[T:2T, 2T:3T] F of the forecast basis, then H3[T:2T, 0:T] F[::-1] of the backcast's

    and C (2 (2 + period), N) the coefficients of every column, fitted on the device (xmca_complexify_theta)."""
    T, period = int(T), int(period)
    if period < 1 or T < 2 * period:
        raise ValueError("extend='theta' needs period >= 1 and at least 2 * period time steps")
    col3, hbar, _, _ = extended_imag_parts(T, 1.0)           # (col3 and hbar do not depend on the period of 'exp')
    kc = 2 + period
    F = theta_forecast_basis(T, period)
    ext = np.zeros((3 * T, 2 * kc))
    ext[2 * T:, :kc] = F
    ext[:T, kc:] = F[::-1]
    B = np.fft.ifft(np.fft.fft(ext, axis=0) * _hilbert_weights(3 * T)[:, None], axis=0).imag[T:2 * T]
    B = np.ascontiguousarray(B - B.mean(axis=0))
    return col3, hbar, B


class Handle:
    """One device + stream + workspace.  Not thread-safe."""

    def __init__(self, device=0):
        self._lib = load_library()
        self._h = _vp()
        n = self._lib.xmca_device_count()
        if n <= 0:
            raise HipError(ERR_HIP, "xmca_amd: no HIP device visible (MI355X / gfx950 required; there is no CPU fallback)")
        rc = self._lib.xmca_create(int(device), ctypes.byref(self._h))
        if rc != 0:
            raise HipError(rc, "xmca_create(device=%d) failed" % device)
        self.device = device
        self.field_dtype = None      # real dtype of the resident fields (float64 after complexify_extended of float32 fields)
        self._keep = []      # host / device buffers that must outlive the handle's use of them

    def close(self):
        if getattr(self, "_h", None):
            self._lib.xmca_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.xmca_last_error(self._h)
            _raise(rc, msg.decode("utf-8", "replace") if msg else "xmca error %d" % rc)

    # ---- result ownership -------------------------------------------------------------------
    def hold_result(self, holder):
        """`holder` (anything with `_materialize_vectors()`) still reads the vectors of the last solve from the device
        on demand; it is asked to fetch them before anything invalidates that result."""
        self._result_holder = weakref.ref(holder)

    def release_result(self):
        ref, self._result_holder = getattr(self, "_result_holder", None), None
        holder = ref() if ref is not None else None
        if holder is not None:
            holder._materialize_vectors()

    # ---- fields -------------------------------------------------------------------------------
    def set_field(self, side, field):
        """field: T x N numpy array (real or complex, float32/float64 based)."""
        self.release_result()
        self.fields_owner = None            # whoever uploads claims the resident fields afterwards (MCA._upload_fields)
        field = np.asarray(field)
        if field.ndim != 2:
            raise ValueError("field must be 2-D (time x space)")
        code = _np_dtype_code(field.dtype)
        T, N = field.shape
        if np.iscomplexobj(field):
            re = np.ascontiguousarray(field.real)
            im = np.ascontiguousarray(field.imag)
        else:
            re = np.ascontiguousarray(field)
            im = None
        self._check(self._lib.xmca_set_field(self._h, side, _ptr(re), _ptr(im), T, N, code, HOST))
        self.field_dtype = np.dtype(_real_np(code))

    def set_field_device(self, side, re_ptr, im_ptr, T, N, dtype):
        """Adopt device pointers (e.g. torch tensors' data_ptr()); the caller keeps them alive."""
        self.release_result()
        self.fields_owner = None
        self._check(self._lib.xmca_set_field(self._h, side, _vp(re_ptr), _vp(im_ptr) if im_ptr else None, T, N,
                                             _np_dtype_code(dtype), DEVICE))
        self.field_dtype = np.dtype(_real_np(_np_dtype_code(dtype)))

    def set_field_strided(self, side, view):
        """The field of `side` from a `DeviceView`: copied on the device into the library's own contiguous buffer
        (xmca_set_field_strided), whatever its two strides; afterwards as after `set_field`.  The view's memory is not written and
        not referenced once this returns; the caller has ordered its own work on it (a stream synchronisation) before."""
        self.release_result()
        self.fields_owner = None
        code = _np_dtype_code(view.dtype)
        self._check(self._lib.xmca_set_field_strided(self._h, side, _vp(view.ptr), view.T, view.N, view.stride_t, view.stride_n, code))
        self.field_dtype = np.dtype(_real_np(code))

    def complexify(self, T):
        self.release_result()
        ht = hilbert_imag_column(T)
        self._check(self._lib.xmca_complexify(self._h, _ptr(ht)))

    def complexify_extended(self, T, period):
        """solve(complexify=True, extend='exp', period=period) on the resident fields: X~ = X + i G X with the operator of
        `extended_imag_parts` (xmca_complexify_extended).  Float32 fields become float64 fields on the device."""
        self.release_result()
        col3, hbar, U, W = extended_imag_parts(T, period)
        self._check(self._lib.xmca_complexify_extended(self._h, _ptr(col3), _ptr(hbar), _ptr(U), _ptr(W), U.shape[1]))
        self.field_dtype = np.dtype(np.float64)

    def complexify_theta(self, T, period):
        """solve(complexify=True, extend='theta', period=period) on the resident fields: X~ = X + i (G0 X + B C) with the parts of
        `theta_imag_parts` and the Theta fits C of every column made on the device (xmca_complexify_theta).  Float32 fields become
        float64 fields on the device."""
        self.release_result()
        col3, hbar, B = theta_imag_parts(T, period)
        self._check(self._lib.xmca_complexify_theta(self._h, _ptr(col3), _ptr(hbar), _ptr(B), int(period)))
        self.field_dtype = np.dtype(np.float64)

    def theta_fit(self, side, N, period):
        """The Theta fits of the columns of the resident real field of `side` (xmca_theta_fit): (2, 3 + period, N) float64 - forecast
        and backcast; rows alpha, b0, level, s_0 .. s_{period-1}."""
        out = np.empty((2, 3 + int(period), int(N)), dtype=np.float64)
        self._check(self._lib.xmca_theta_fit(self._h, side, int(period), _ptr(out)))
        return out

    def get_field_imag(self, side, shape):
        """Imaginary plane (float64) of the resident field of `side` after `complexify_extended` / `complexify_theta`."""
        out = np.empty(shape, dtype=np.float64)
        self._check(self._lib.xmca_get_field_imag(self._h, side, _ptr(out)))
        return out

    def decomplexify(self):
        """Back to the real resident fields (undoes `complexify` for the next solve)."""
        self.release_result()
        self._check(self._lib.xmca_complexify(self._h, None))

    # ---- solve --------------------------------------------------------------------------------
    def solve(self, n_fields, n_vec=-1):
        self.release_result()
        rank = _c_i64(0)
        self._check(self._lib.xmca_solve(self._h, n_fields, n_vec, ctypes.byref(rank)))
        return int(rank.value)

    def solve_info(self):
        """Per eigenproblem of the last solve (left Gram, right Gram, kernel): sweeps / tile / slots of the Jacobi solver, whether a
        Cholesky LR step or the tridiagonal route was taken, and `n_eigvec`, the eigenvectors actually formed - the order of the
        problem, or the k' >= n_vec of the partial stage for a one-field `solve(n_fields, n_vec=k)`."""
        info = np.zeros(18, dtype=np.int32)
        self._check(self._lib.xmca_get_solve_info(self._h, _ptr(info), 18))
        return [{"sweeps": int(info[3 * i]), "tile": int(info[3 * i + 1]), "slots": int(info[3 * i + 2]), "lr_step": int(info[9 + i]) & 1,
                 "tridiag": (int(info[9 + i]) >> 1) & 1, "n_eigvec": int(info[12 + i])} for i in range(3)]

    def result_info(self):
        """What the last solve left resident: `n_vec` modes, and the KiB their vector planes occupy per side."""
        info = np.zeros(18, dtype=np.int32)
        self._check(self._lib.xmca_get_solve_info(self._h, _ptr(info), 18))
        return {"n_vec": int(info[15]), "vector_kib": [int(info[16]), int(info[17])]}

    def singular_values(self, n):
        out = np.empty(n, dtype=np.float64)
        self._check(self._lib.xmca_get_singular_values(self._h, _ptr(out), n))
        return out

    def vectors(self, side, n_modes, N, dtype):
        """Returns Vt (n_modes x N); V = Vt.T."""
        cplx = bool(self._lib.xmca_is_complex(self._h))
        code = _np_dtype_code(dtype)
        out = np.empty((n_modes, N), dtype=_cplx_np(code) if cplx else _real_np(code))
        self._check(self._lib.xmca_get_vectors(self._h, side, _ptr(out), n_modes, code))
        return out

    def eofs(self, side, N, m, W, dtype):
        """(N x q) EOFs of `side` in their final layout: V[:, :m] @ W mixed on the device (W: m x q float64 / complex128), or the
        first m vectors as they are (W None).  xmca_get_eofs: array.py:615-646 + :676-721 without an N x m pass on the host."""
        cplx = bool(self._lib.xmca_is_complex(self._h))
        code = _np_dtype_code(dtype)
        W, w_cplx = _host_vectors(W)
        if W is not None:
            m, q = W.shape
        else:
            q = m
        out = np.empty((N, q), dtype=_cplx_np(code) if cplx or w_cplx else _real_np(code))
        self._check(self._lib.xmca_get_eofs(self._h, side, _ptr(W), m, q, int(w_cplx), _ptr(out), code))
        return out

    def maps(self, side, N, m, W, col_factor, keep_idx, N_full, kind, scaling, dtype, want_stats=False, alloc=None):
        """(N_full x q) spatial map of `side` in its final layout (xmca_get_maps): the values of `eofs(side, N, m, W, dtype)` times the
        q per-column factors `col_factor` (None: as they are), as EOFs, amplitudes or phases (`kind`: MAP_*), every column divided
        by its largest value or its standard deviation over the N kept points (`scaling`: SCALE_*), NaN at the rows not in keep_idx
        (None: N_full = N).  `dtype`: float32 / float64 components of the result.  want_stats: (map, the q float64 divisors).
        alloc: None, or `alloc(shape, numpy dtype) -> (array on this handle's GPU, its device address)`: the map is then written there
        by the device (xmca_get_maps_to, XMCA_DEVICE) and that array returned - nothing is copied to the host."""
        cplx = bool(self._lib.xmca_is_complex(self._h))
        code = _np_dtype_code(dtype)
        W, w_cplx = _host_vectors(W)
        if W is not None:
            m, q = W.shape
        else:
            q = m
        f, f_cplx = _host_vectors(col_factor)
        if f is not None and f.shape != (q,):
            raise ValueError("maps: col_factor must hold one value per column (%d), got shape %s" % (q, f.shape))
        idx = _kept_index("maps", keep_idx, N)
        o_cplx = kind == MAP_EOF and (cplx or w_cplx or f_cplx)
        out, out_ptr, where = _output(alloc, (int(N_full), q), _cplx_np(code) if o_cplx else _real_np(code))
        stats = np.full(q, np.nan) if want_stats else None
        self._check(self._lib.xmca_get_maps_to(self._h, side, _ptr(W), m, q, int(w_cplx), _ptr(f), int(f_cplx), _ptr(idx), int(N_full),
                                               int(kind), int(scaling), out_ptr, code, _ptr(stats), where))
        return (out, stats) if want_stats else out

    def project(self, side, V, T, m=None, N=None):
        """U = X~ V (T x m) on the resident field of `side` (the analytic signal when the model is complex);
        float64 / complex128.  MCA._get_U's `fields[k] @ V[k]` (array.py:391).  V None: the first m vectors of the last solve,
        still resident (N: their length)."""
        Vd, cplx = _host_vectors(V)
        if Vd is not None:
            N, m = Vd.shape
        out = np.empty((T, m), dtype=np.complex128)          # large enough for either result type
        out_cplx = _c_int(0)
        self._check(self._lib.xmca_project(self._h, side, _ptr(Vd), N, m, int(cplx), _ptr(out), ctypes.byref(out_cplx)))
        return _unpack(out, T, m, out_cplx.value)

    def predict(self, side, X, keep_idx, mean, std, V, W, weight=None):
        """((X[:, keep_idx] - mean) / std) V W (T' x q, float64 / complex128) on the device (xmca_predict): MCA.predict's product
        without the vectors leaving the device.  X: T' x N_full real new data (its dtype is the ingest's: mean / std are cast to
        it); keep_idx: kept columns or None; std None: no division; V: N' x m host vectors or None (the first m resident ones of
        the last solve of `side`); W: m x q mix.  weight: N' float64 factors applied after the division, numpy's in-place
        `x *= weight` (xmca_predict_weighted), or None.  The resident fields and vectors stay as they are."""
        if isinstance(X, DeviceView):        # new data on this GPU: read where it is (xmca_predict_strided, XMCA_DEVICE)
            x_ptr, x_strides, x_dtype, where = _vp(X.ptr), (X.stride_t, X.stride_n), X.dtype, DEVICE
        else:
            X = np.ascontiguousarray(X)
            if np.iscomplexobj(X) or X.ndim != 2:
                raise TypeError("predict: X must be a real 2-D array")
            x_ptr, x_strides, x_dtype, where = _ptr(X), (X.shape[1], 1), X.dtype, HOST
        code = _np_dtype_code(x_dtype)
        T, N_full = X.shape
        idx = _kept_index("predict", keep_idx)
        N = N_full if idx is None else idx.size
        mean = np.ascontiguousarray(np.broadcast_to(mean, (N,)), dtype=x_dtype)
        std = None if std is None else np.ascontiguousarray(np.broadcast_to(std, (N,)), dtype=x_dtype)
        Vd, v_cplx = _host_vectors(V)
        Wd, w_cplx = _host_vectors(W)
        m, q = Wd.shape
        if Vd is not None and Vd.shape != (N, m):
            raise ValueError("predict: V must be N' x m = %d x %d, got %s" % (N, m, Vd.shape))
        out = np.empty((T, q), dtype=np.complex128)
        out_cplx = _c_int(0)
        weight = None if weight is None else _column_weights("predict", weight, N)
        self._check(self._lib.xmca_predict_strided(self._h, side, x_ptr, T, N_full, x_strides[0], x_strides[1], where, code, _ptr(idx), N,
                                                   _ptr(mean), _ptr(std), _ptr(Vd), int(v_cplx), _ptr(Wd), m, q, int(w_cplx), _ptr(out),
                                                   ctypes.byref(out_cplx), _ptr(weight)))
        return _unpack(out, T, q, out_cplx.value)

    def reconstruct(self, side, B, V, N, keep_idx=None, N_full=None, mean=None, std=None, inv_weight=None, alloc=None):
        """Re(B V^H) (* std + mean) on the device (xmca_reconstruct), T x N_full float64 with NaN at the columns not in keep_idx.
        B: T x m coefficients; V: N x m host vectors or None (the first m resident ones of the last solve of `side`).
        inv_weight: N float64 factors the product is divided by first, numpy's `x /= inv_weight` (xmca_reconstruct_weighted), or
        None.  alloc: as in `maps` - the result is written on the device (xmca_reconstruct_to, XMCA_DEVICE).  The resident fields
        and vectors stay as they are."""
        Bd, b_cplx = _host_vectors(B)
        T, m = Bd.shape
        Vd, v_cplx = _host_vectors(V)
        if Vd is not None and Vd.shape != (N, m):
            raise ValueError("reconstruct: V must be N x m = %d x %d, got %s" % (N, m, Vd.shape))
        idx = _kept_index("reconstruct", keep_idx)
        N_full = N if N_full is None else N_full
        mean = None if mean is None else np.ascontiguousarray(np.broadcast_to(mean, (N,)), dtype=np.float64)
        std = None if std is None else np.ascontiguousarray(np.broadcast_to(std, (N,)), dtype=np.float64)
        out, out_ptr, where = _output(alloc, (T, int(N_full)), np.float64)
        inv_weight = None if inv_weight is None else _column_weights("reconstruct", inv_weight, N)
        self._check(self._lib.xmca_reconstruct_to(self._h, side, _ptr(Bd) if m else None, T, m, int(b_cplx), _ptr(Vd), int(v_cplx), _ptr(idx),
                                                  N, N_full, _ptr(mean), _ptr(std), out_ptr, _ptr(inv_weight), where))
        return out

    def center_field(self, side, N):
        """Centers the resident (raw) field of `side` in place.  Returns (mean[N], std[N], number of NaN entries).  Only the
        columns without NaN are centered; a column holding a NaN is left as it is, and its mean and std are NaN."""
        self.release_result()
        mean = np.empty(N, dtype=np.float64)
        std = np.empty(N, dtype=np.float64)
        n_nan = _c_i64(0)
        self._check(self._lib.xmca_center_field(self._h, side, _ptr(mean), _ptr(std), ctypes.byref(n_nan)))
        return mean, std, int(n_nan.value)

    def compact_field(self, side, N):
        """Drops the NaN columns of the resident raw field of `side`.  Returns (keep mask[N], number of kept columns)."""
        self.release_result()
        keep = np.empty(N, dtype=np.int32)
        n_keep = _c_i64(0)
        self._check(self._lib.xmca_compact_field(self._h, side, _ptr(keep), ctypes.byref(n_keep)))
        return keep.astype(bool), int(n_keep.value)

    def scale_field(self, side, w, divide=False):
        """Multiplies (divides) column c of the resident real field of `side` by w[c]; `w` in the field's dtype."""
        self.release_result()
        w = np.ascontiguousarray(w)
        self._check(self._lib.xmca_scale_field(self._h, side, _ptr(w), int(bool(divide))))

    def get_field(self, side, shape, dtype):
        """Real plane of the resident field of `side` as a (T, N) array of `dtype` (the dtype it was set with; a float32 field
        promoted by `complexify_extended` comes back exactly, through float64)."""
        resident = self.field_dtype if self.field_dtype is not None else np.dtype(dtype)
        out = np.empty(shape, dtype=resident)
        self._check(self._lib.xmca_get_field(self._h, side, _ptr(out)))
        return out.astype(dtype, copy=False)

    def bootstrap_begin(self, n_fields):
        """Working copies of the resident fields for `bootstrap_runs` (MCA.bootstrapping on the device)."""
        self.release_result()
        self._check(self._lib.xmca_bootstrap_begin(self._h, n_fields))

    def bootstrap_runs(self, T, complexify, idx_left, idx_right, n_runs, rotated, p, power, tol, n_out, extend_period=None,
                       theta_period=None, axis=0):
        """All replicates in one call (several in flight on the device).  idx_*: COMPOSED indices into the fields as they were at
        `bootstrap_begin`, or None - axis=0: (n_runs, T) row indices; axis=1: (n_runs, Nl) / (n_runs, Nr) column indices into
        [left | right] (xmca_bootstrap_runs_columns*).  `extend_period`: replicates of a complex model with extend='exp' and
        this period (xmca_bootstrap_runs*_extended; float64 fields).  `theta_period`: replicates of a complex model with
        extend='theta' and this season length, every one fitted again on the device (xmca_bootstrap_runs*_theta; float64 fields).
        Returns (spectra[n_runs, n_out], kept[n_runs])."""
        if axis not in (0, 1):
            raise ValueError('{:} not a valid axis. either 0 or 1.'.format(axis))
        if extend_period is not None and theta_period is not None:
            raise ValueError("bootstrap_runs: extend_period (extend='exp') and theta_period (extend='theta') exclude each other")
        il = None if idx_left is None else np.ascontiguousarray(idx_left, dtype=np.int64).reshape(n_runs, -1)
        ir = None if idx_right is None else np.ascontiguousarray(idx_right, dtype=np.int64).reshape(n_runs, -1)
        if axis == 0 and any(i is not None and i.shape[1] != T for i in (il, ir)):
            raise ValueError("bootstrap_runs: row indices must be n_runs x T")
        out = np.zeros((n_runs, n_out), dtype=np.float64)
        kept = np.zeros(n_runs, dtype=np.int32)
        columns = "_columns" if axis == 1 else ""
        # the operator of the replicates' complexification: the symbol's suffix and its leading arguments
        if complexify and extend_period is not None:
            col3, hbar, U, W = extended_imag_parts(T, extend_period)
            suffix, lead = "_extended", (_ptr(col3), _ptr(hbar), _ptr(U), _ptr(W), U.shape[1])
        elif complexify and theta_period is not None:
            col3, hbar, B = theta_imag_parts(T, theta_period)          # (once per call, not per replicate)
            suffix, lead = "_theta", (_ptr(col3), _ptr(hbar), _ptr(B), int(theta_period))
        else:
            ht = hilbert_imag_column(T) if complexify else None
            suffix, lead = "", (_ptr(ht),)
        run = getattr(self._lib, "xmca_bootstrap_runs" + columns + suffix)
        self._check(run(self._h, *lead, _ptr(il), _ptr(ir), n_runs, int(rotated), int(p), int(power), float(tol), _ptr(out), _ptr(kept),
                        n_out))
        return out, kept.astype(bool)

    def bootstrap_patterns(self, T, complexify, idx, n_runs, k, v0_left, v0_right=None):
        """Bootstrap mean and standard error of the k leading vectors (xmca_bootstrap_patterns), after `bootstrap_begin`: run r
        resamples the rows idx[r] (n_runs x T, the same for every field), is centred, complexified like the model and solved; its
        vectors are aligned with v0 (N x k per field, unit columns) and accumulated on the device.  Returns (mean, std, congruence,
        sigma, kept): mean / std lists of N x k arrays per field (mean complex for a complex model, std real), congruence and sigma
        n_runs x k, kept n_runs flags."""
        n_runs, k, cplx = int(n_runs), int(k), bool(complexify)
        if n_runs < 2:
            raise ValueError("bootstrap_patterns: a standard error needs n_runs >= 2")
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        if idx.shape != (n_runs, int(T)):
            raise ValueError("bootstrap_patterns: the row indices must be n_runs x T")
        sides = [_mode_major_planes("bootstrap_patterns", V, k, cplx) for V in (v0_left, v0_right)]
        mean = [np.empty((k, N), dtype=np.complex128 if cplx else np.float64) if re is not None else None for re, _, N in sides]
        std = [np.empty((k, N), dtype=np.float64) if re is not None else None for re, _, N in sides]
        congruence = np.empty((n_runs, k), dtype=np.float64)
        sigma = np.zeros((n_runs, k), dtype=np.float64)
        kept = np.zeros(n_runs, dtype=np.int32)
        ht = hilbert_imag_column(int(T)) if cplx else None
        self._check(self._lib.xmca_bootstrap_patterns(
            self._h, _ptr(ht), _ptr(idx), n_runs, k, _ptr(sides[0][0]), _ptr(sides[0][1]), _ptr(sides[1][0]), _ptr(sides[1][1]),
            _ptr(mean[0]), _ptr(std[0]), _ptr(mean[1]), _ptr(std[1]), _ptr(congruence), _ptr(sigma), _ptr(kept)))
        n = 1 if v0_right is None else 2
        return [m.T for m in mean[:n]], [s.T for s in std[:n]], congruence, sigma, kept.astype(bool)

    def pattern_stats(self, v0_left, v_left, v0_right=None, v_right=None, plane_dtype=np.float64, n_lanes=1):
        """(tests) The statistics of `bootstrap_patterns` from given replicate vectors (xmca_pattern_stats): v0_* N x k, v_* n_runs x
        N x k (complex: a complex model); the replicate planes are narrowed to `plane_dtype` on the device, run r goes to the
        accumulators r % n_lanes.  Returns (mean, std, congruence) as `bootstrap_patterns` does."""
        v_left = np.asarray(v_left)
        n_runs, _, k = v_left.shape
        cplx = any(V is not None and np.iscomplexobj(V) for V in (v0_left, v_left, v0_right, v_right))
        sides = [_mode_major_planes("pattern_stats", V, k, cplx) for V in (v0_left, v0_right)]
        reps = []
        for V, (_, _, N) in zip((v_left, v_right), sides):
            if V is None:
                reps.append((None, None))
                continue
            V = np.asarray(V)
            if V.shape != (n_runs, N, k):
                raise ValueError("pattern_stats: the replicate vectors of a field must be n_runs x N x k")
            Vt = np.swapaxes(V, 1, 2)
            reps.append((np.ascontiguousarray(Vt.real, dtype=np.float64), np.ascontiguousarray(Vt.imag, dtype=np.float64) if cplx else None))
        if (v0_right is None) != (v_right is None):
            raise ValueError("pattern_stats: a right side needs both its model vectors and its replicates")
        mean = [np.empty((k, N), dtype=np.complex128 if cplx else np.float64) if re is not None else None for re, _, N in sides]
        std = [np.empty((k, N), dtype=np.float64) if re is not None else None for re, _, N in sides]
        congruence = np.empty((n_runs, k), dtype=np.float64)
        self._check(self._lib.xmca_pattern_stats(
            self._h, _ptr(sides[0][0]), _ptr(sides[0][1]), _ptr(sides[1][0]), _ptr(sides[1][1]), _ptr(reps[0][0]), _ptr(reps[0][1]),
            _ptr(reps[1][0]), _ptr(reps[1][1]), int(n_runs), int(k), sides[0][2], sides[1][2], int(cplx), _np_dtype_code(plane_dtype),
            int(n_lanes), _ptr(mean[0]), _ptr(std[0]), _ptr(mean[1]), _ptr(std[1]), _ptr(congruence)))
        n = 1 if v0_right is None else 2
        return [m.T for m in mean[:n]], [s.T for s in std[:n]], congruence

    def correlate(self, side, Y, N):
        """r (N x m) = Pearson correlation of the real part of every column of the resident field `side` with the columns
        of Y (T x m).  tools/array.py:76-88 without the (N + m)^2 corrcoef matrix."""
        Yd = np.ascontiguousarray(np.asarray(Y).real, dtype=np.float64)
        T, m = Yd.shape
        r = np.empty((N, m), dtype=np.float64)
        self._check(self._lib.xmca_correlate(self._h, side, _ptr(Yd), T, m, _ptr(r)))
        return r

    def pearson_pvalues(self, r, n_obs):
        """Two-sided p-values of the correlations `r` of n_obs samples on the device (xmca_pearson_pvalues): float64, the shape of
        `r`; tools/array.py:86-88.  n_obs < 3 raises ValueError (the null distribution does not exist)."""
        rd = np.ascontiguousarray(r, dtype=np.float64)
        p = np.empty(rd.shape, dtype=np.float64)
        self._check(self._lib.xmca_pearson_pvalues(self._h, _ptr(rd), rd.size, int(n_obs), _ptr(p)))
        return p

    def correlation_maps(self, side, Y, keep_idx, N_full, r_dtype, alloc=None):
        """(r, p), both N_full x m in their final layout: correlations of the resident field `side` with the columns of Y (T x m)
        in `r_dtype`, their two-sided p-values (float64, from the rounded r), NaN at the rows not in keep_idx (None: every row
        is a column of the field).  alloc: as in `maps` - both maps are written on the device (xmca_correlation_maps_to,
        XMCA_DEVICE)."""
        Yd = np.ascontiguousarray(np.asarray(Y).real, dtype=np.float64)
        T, m = Yd.shape
        idx = _kept_index("correlation_maps", keep_idx)
        code = _np_dtype_code(r_dtype)
        r, r_ptr, where = _output(alloc, (int(N_full), m), _real_np(code))
        p, p_ptr, where = _output(alloc, (int(N_full), m), np.float64)
        self._check(self._lib.xmca_correlation_maps_to(self._h, side, _ptr(Yd), T, m, _ptr(idx), int(N_full), code, r_ptr, p_ptr, where))
        return r, p

    # ---- rotation -----------------------------------------------------------------------------
    def rotate_loadings(self, L, n_left, power=1, tol=1e-8, max_iter=1000, varimax_only=False, want_B=False, gamma=1.0):
        Ld, cplx = _host_vectors(L)
        N, p = Ld.shape
        cdt = Ld.dtype
        R = np.empty((p, p), dtype=cdt)
        Phi = np.empty((p, p), dtype=cdt)
        nl = np.zeros(p)
        nr = np.zeros(p)
        B = np.empty((N, p), dtype=cdt) if want_B else None
        iters = _c_int(0)
        rc = self._lib.xmca_rotate_loadings(self._h, _ptr(Ld), N, int(n_left), p, int(cplx), int(power), float(tol),
                                            int(max_iter), int(varimax_only), float(gamma), _ptr(B), _ptr(R), _ptr(Phi), _ptr(nl),
                                            _ptr(nr), ctypes.byref(iters))
        self.last_iters = int(iters.value)
        self._check(rc)
        return {"B": B, "R": R, "Phi": Phi, "norm_left": nl, "norm_right": nr, "n_iter": int(iters.value)}

    def rotate_solved(self, p, power=1, tol=1e-8, max_iter=1000):
        """MCA.rotate on the resident result of the last solve (the loadings are built on the device)."""
        cplx = bool(self._lib.xmca_is_complex(self._h))
        cdt = np.complex128 if cplx else np.float64
        R = np.empty((p, p), dtype=cdt)
        Phi = np.empty((p, p), dtype=cdt)
        nl = np.zeros(p)
        nr = np.zeros(p)
        iters = _c_int(0)
        rc = self._lib.xmca_rotate_solved(self._h, int(p), int(power), float(tol), int(max_iter), _ptr(R), _ptr(Phi), _ptr(nl),
                                          _ptr(nr), ctypes.byref(iters))
        self.last_iters = int(iters.value)
        self._check(rc)
        return {"B": None, "R": R, "Phi": Phi, "norm_left": nl, "norm_right": nr, "n_iter": int(iters.value)}

    def vectors_are_f32(self, side=0):
        """the vectors of the last solve are resident in float32 (real float32 field, dual side): include/xmca_hip.h"""
        return bool(self._lib.xmca_vectors_are_f32(self._h, int(side)))

    def holds_result_of(self, holder):
        ref = getattr(self, "_result_holder", None)
        return ref is not None and ref() is holder

    # ---- rule N -------------------------------------------------------------------------------
    def rule_n(self, T, Nx, Ny, n_fields, complexify, rotated, p, power, tol, run_begin, run_end, seed, dtype, n_out, ar1=None):
        """ar1 = (phi_left, phi_right or None): red-noise surrogates with these lag-1 autocorrelations per column (xmca_rule_n_ar1);
        None: the white surrogates of xmca_rule_n."""
        if ar1 is not None:
            ar1 = _phi_pair("rule_n", ar1, Nx, Ny, n_fields)
        self.release_result()
        n = run_end - run_begin
        self.fields_owner = None            # the surrogates overwrite the resident fields
        spectra = np.zeros((max(n, 0), n_out), dtype=np.float64)
        kept = np.zeros(max(n, 0), dtype=np.int32)
        ht = hilbert_imag_column(T) if complexify else None
        self.field_dtype = None
        if n > 0 and ar1 is None:
            self._check(self._lib.xmca_rule_n(self._h, T, Nx, Ny if n_fields == 2 else 0, n_fields, _ptr(ht), int(rotated),
                                              int(p), int(power), float(tol), run_begin, run_end, int(seed),
                                              _np_dtype_code(dtype), _ptr(spectra), _ptr(kept), n_out))
        elif n > 0:
            self._check(self._lib.xmca_rule_n_ar1(self._h, T, Nx, Ny if n_fields == 2 else 0, n_fields, _ptr(ht), int(rotated),
                                                  int(p), int(power), float(tol), run_begin, run_end, int(seed),
                                                  _np_dtype_code(dtype), _ptr(spectra), _ptr(kept), n_out, _ptr(ar1[0]), _ptr(ar1[1])))
        return spectra, kept

    def rule_n_sharded(self, comm, n_runs, T, Nx, Ny, n_fields, complexify, rotated, p, power, tol, seed, dtype, n_out, ar1=None):
        """xmca_rule_n_sharded: this rank's block of the runs [0, n_runs) + ONE ncclAllGather (native RCCL communicator
        `comm`, see `Comm`); every rank gets all n_runs x n_out spectra and kept flags.  ar1 = (phi_left, phi_right or None):
        red-noise surrogates (xmca_rule_n_ar1_sharded); the caller passes the same phi on every rank."""
        if ar1 is not None:
            ar1 = _phi_pair("rule_n_sharded", ar1, Nx, Ny, n_fields)
        self.release_result()
        self.fields_owner = None
        self.field_dtype = None
        spectra = np.zeros((max(n_runs, 0), n_out), dtype=np.float64)
        kept = np.zeros(max(n_runs, 0), dtype=np.int32)
        ht = hilbert_imag_column(T) if complexify else None
        if ar1 is None:
            self._check(self._lib.xmca_rule_n_sharded(self._h, comm._c, int(n_runs), T, Nx, Ny if n_fields == 2 else 0, n_fields,
                                                      _ptr(ht), int(rotated), int(p), int(power), float(tol), int(seed),
                                                      _np_dtype_code(dtype), _ptr(spectra), _ptr(kept), n_out))
        else:
            self._check(self._lib.xmca_rule_n_ar1_sharded(self._h, comm._c, int(n_runs), T, Nx, Ny if n_fields == 2 else 0, n_fields,
                                                          _ptr(ht), int(rotated), int(p), int(power), float(tol), int(seed),
                                                          _np_dtype_code(dtype), _ptr(spectra), _ptr(kept), n_out, _ptr(ar1[0]),
                                                          _ptr(ar1[1])))
        return spectra, kept

    def surrogate(self, n, seed, run, side):
        out = np.empty(n, dtype=np.float64)
        self._check(self._lib.xmca_surrogate(self._h, n, int(seed), int(run), int(side), _ptr(out)))
        return out

    def surrogate_ar1(self, T, N, phi, seed, run, side, dtype):
        """(tests) the red-noise surrogate of (seed, run, side) before it is centred: (T, N) float64 holding the values of the run
        `dtype` (xmca_surrogate_ar1).  phi: N values; one that is not finite or has |phi| >= 1 is refused by the library
        (ValueError) before anything is launched."""
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        if phi.shape != (int(N),):
            raise ValueError("surrogate_ar1: phi must hold one value per column (%d), got shape %s" % (N, phi.shape))
        out = np.empty((int(T), int(N)), dtype=np.float64)
        self._check(self._lib.xmca_surrogate_ar1(self._h, int(T), int(N), _ptr(phi), int(seed), int(run), int(side),
                                                 _np_dtype_code(dtype), _ptr(out)))
        return out

    def lag1_autocorrelation(self, side, N):
        """Lag-1 autocorrelation of every column of the resident real field of `side` (xmca_lag1_autocorrelation): N float64 values,
        0 for a constant column.  The field stays as it is; N doubles come back."""
        out = np.empty(int(N), dtype=np.float64)
        self._check(self._lib.xmca_lag1_autocorrelation(self._h, int(side), _ptr(out)))
        return out

    def lag_gram(self, G, embedding, tau, center):
        """(tests) The lag-sum and centring kernels of `extended_eofs` on a host matrix (xmca_lag_gram): K[t, s] = sum_j G[t + j tau,
        s + j tau] for the symmetric n x n float64 `G`, T' x T' with T' = n - (embedding - 1) tau, doubly centred when `center`."""
        G = np.ascontiguousarray(G, dtype=np.float64)
        if G.ndim != 2 or G.shape[0] != G.shape[1]:
            raise ValueError("lag_gram: G must be a square matrix, got shape %s" % (G.shape,))
        n_out = G.shape[0] - (int(embedding) - 1) * int(tau)
        if int(embedding) < 1 or int(tau) < 1 or n_out < 1:
            raise ValueError("lag_gram: embedding and tau must be >= 1 with (embedding - 1) * tau below n")
        out = np.empty((n_out, n_out), dtype=np.float64)
        self._check(self._lib.xmca_lag_gram(self._h, _ptr(G), G.shape[0], int(embedding), int(tau), int(bool(center)), _ptr(out)))
        return out

    def extended_eofs(self, T, N, embedding, tau, n_modes, keep_idx=None, N_full=None):
        """Extended EOFs of the resident real T x N field of side 0 (xmca_extended_eofs): (lam, pcs, eofs) - all T' = T - (embedding - 1)
        tau eigenvalues sigma^2 of the centred lag-embedded field, descending; the T' x n_modes PCs of unit variance; the patterns,
        embedding x N_full x n_modes in their final layout, NaN at the rows not in keep_idx (None: N_full = N).  All float64.  The
        result of a solve and the fields stay as they are."""
        M, tau, k = int(embedding), int(tau), int(n_modes)
        n_out = int(T) - (M - 1) * tau
        idx = _kept_index("extended_eofs", keep_idx, N)
        N_full = int(N) if N_full is None else int(N_full)
        if M < 1 or tau < 1 or n_out < 2 or not 1 <= k <= min(n_out - 1, M * int(N)):
            raise ValueError("extended_eofs: embedding, tau >= 1, T' >= 2 and 1 <= n_modes <= min(T' - 1, embedding * N) are needed")
        lam = np.empty(n_out, dtype=np.float64)
        pcs = np.empty((n_out, k), dtype=np.float64)
        eofs = np.empty((M, N_full, k), dtype=np.float64)
        self._check(self._lib.xmca_extended_eofs(self._h, M, tau, k, _ptr(idx), N_full, _ptr(lam), _ptr(pcs), _ptr(eofs)))
        return lam, pcs, eofs

    @staticmethod
    def _lag_modes(what, T, N, embedding, tau, n_modes):
        """(M, tau, k, T') of the Monte-Carlo SSA entries, with the argument rules of `extended_eofs`."""
        M, tau, k = int(embedding), int(tau), int(n_modes)
        n_out = int(T) - (M - 1) * tau
        if M < 1 or tau < 1 or n_out < 2 or not 1 <= k <= min(n_out - 1, M * int(N)):
            raise ValueError("%s: embedding, tau >= 1, T' >= 2 and 1 <= n_modes <= min(T' - 1, embedding * N) are needed" % what)
        return M, tau, k, n_out

    def extended_rule_n(self, T, N, embedding, tau, n_modes, phi, run_begin, run_end, seed):
        """Monte-Carlo SSA test of the extended EOFs of the resident real T x N field of side 0 (xmca_extended_rule_n): (lam, scale,
        surrogates) - all T' eigenvalues of `extended_eofs`; the N column standard deviations d (ddof = 1); Lambda of the runs
        [run_begin, run_end), (runs, n_modes).  phi: N values, every one finite with |phi| < 1.  All float64.  The result of a
        solve and the fields stay as they are."""
        M, tau, k, n_out = self._lag_modes("extended_rule_n", T, N, embedding, tau, n_modes)
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        run_begin, run_end = int(run_begin), int(run_end)
        if phi.shape != (int(N),):
            raise ValueError("extended_rule_n: phi must hold one value per column (%d), got shape %s" % (N, phi.shape))
        if not 0 <= run_begin <= run_end:
            raise ValueError("extended_rule_n: the runs must be a range [run_begin, run_end) with 0 <= run_begin <= run_end")
        lam = np.empty(n_out, dtype=np.float64)
        scale = np.empty(int(N), dtype=np.float64)
        surrogates = np.empty((run_end - run_begin, k), dtype=np.float64)
        self._check(self._lib.xmca_extended_rule_n(self._h, M, tau, k, _ptr(phi), run_begin, run_end, int(seed), _ptr(lam), _ptr(scale),
                                                   _ptr(surrogates)))
        return lam, scale, surrogates

    def extended_project(self, T, N, embedding, tau, n_modes, R, apply_scale):
        """(tests) Lambda_c(R) of the host T x N field `R` on the extended EOFs of the resident field of side 0
        (xmca_extended_project): n_modes float64 values from the front, scale, product and projection kernels of `extended_rule_n`;
        `apply_scale` multiplies column c of R by the resident field's standard deviation d_c."""
        M, tau, k, _ = self._lag_modes("extended_project", T, N, embedding, tau, n_modes)
        R = np.ascontiguousarray(R, dtype=np.float64)
        if R.shape != (int(T), int(N)):
            raise ValueError("extended_project: R must be the field's shape (%d, %d), got %s" % (T, N, R.shape))
        out = np.empty(k, dtype=np.float64)
        self._check(self._lib.xmca_extended_project(self._h, M, tau, k, _ptr(R), int(bool(apply_scale)), _ptr(out)))
        return out

    def lag_project(self, W, embedding, tau, k):
        """(tests) The projection kernels of `extended_rule_n` on a host matrix (xmca_lag_project): from the T x embedding k float64
        `W`, Q[t, c] = sum_j W[t + j tau, j k + c] over the T' = T - (embedding - 1) tau windows and the k sums of squares of its
        centred columns."""
        W = np.ascontiguousarray(W, dtype=np.float64)
        M, tau, k = int(embedding), int(tau), int(k)
        if M < 1 or tau < 1 or k < 1 or W.ndim != 2 or W.shape[1] != M * k or W.shape[0] - (M - 1) * tau < 1:
            raise ValueError("lag_project: W must be T x embedding k with embedding, tau, k >= 1 and (embedding - 1) * tau below T")
        out = np.empty(k, dtype=np.float64)
        self._check(self._lib.xmca_lag_project(self._h, _ptr(W), W.shape[0], M, tau, k, _ptr(out)))
        return out

    def fill_gaps(self, X, n_modes, max_iter, tol, cv_idx=None, embedding=None, tau=1):
        """DINEOF gap filling of the T x N float32 / float64 field `X` with NaN gaps (xmca_fill_gaps): (field, history, cv_rms, lam) -
        X with its gaps filled, in X's dtype and with the present entries untouched; the relative changes d_i of the iterations run;
        the RMS error at the withheld entries `cv_idx` (flat indices of present entries; None without any); the n_modes leading
        eigenvalues of the last iterate's Gram matrix.  Resident fields and the result of a solve stay as they are.
        With `embedding` (see `fill_gaps_lagged`) the call goes through xmca_fill_gaps_lagged."""
        X = _gap_plane("fill_gaps", X)
        T, N = X.shape
        idx = None if cv_idx is None else np.ascontiguousarray(cv_idx, dtype=np.int64).ravel()
        n_cv = 0 if idx is None else idx.size
        k, max_iter = int(n_modes), int(max_iter)
        if max_iter < 1:
            raise ValueError("fill_gaps: max_iter must be at least 1")
        out = np.empty_like(X)
        history = np.full(max_iter, np.nan, dtype=np.float64)
        lam = np.empty(max(k, 1), dtype=np.float64)
        iters, cv_rms = _c_int(0), _c_dbl(np.nan)
        head = (self._h, _ptr(X), T, N, _np_dtype_code(X.dtype), _ptr(idx) if n_cv else None, n_cv, k)
        tail = (max_iter, float(tol), _ptr(out), _ptr(history), ctypes.byref(iters), ctypes.byref(cv_rms), _ptr(lam))
        if embedding is None:
            self._check(self._lib.xmca_fill_gaps(*head, *tail))
        else:
            self._check(self._lib.xmca_fill_gaps_lagged(*head, int(embedding), int(tau), *tail))
        return out, history[:iters.value].copy(), (float(cv_rms.value) if n_cv else None), lam[:k]

    def fill_gaps_lagged(self, X, n_modes, embedding, tau, max_iter, tol, cv_idx=None):
        """M-SSA gap filling (xmca_fill_gaps_lagged): `fill_gaps` on the plane embedded with `embedding` windows `tau` steps apart;
        lam are the leading eigenvalues of the lag-summed Gram matrix.  embedding = 1 gives the bits of `fill_gaps`."""
        return self.fill_gaps(X, n_modes, max_iter, tol, cv_idx=cv_idx, embedding=embedding, tau=tau)

    def _regress_field(self, what, X):
        """The field of the regression entries as their leading arguments: (keep-alive, pointer, location, T, N, stride_t, stride_n,
        dtype code, numpy dtype) of a contiguous T x N host array or of a `DeviceView`."""
        if isinstance(X, DeviceView):
            return X, _vp(X.ptr), DEVICE, X.T, X.N, X.stride_t, X.stride_n, _np_dtype_code(X.dtype), X.dtype
        X = _gap_plane(what, X)
        return X, _ptr(X), HOST, X.shape[0], X.shape[1], X.shape[1], 1, _np_dtype_code(X.dtype), X.dtype

    def column_regress(self, X, basis, alloc=None):
        """Least-squares fit of every column of the T x N float32 / float64 field `X` (a host array or a `DeviceView`; NaN = missing)
        on the columns of `basis` (T x k float64, k <= 16) over its present entries, and the residual (xmca_column_regress):
        (field, coefficients, fitted) - T x N in X's dtype with NaN at the missing entries and in the columns that are not fitted,
        k x N float64 (NaN where not fitted), N bools.  alloc: as in `maps` - the field is written on the device.  Resident fields
        and the result of a solve stay as they are."""
        keep, ptr, where_in, T, N, st, sn, code, dt = self._regress_field("column_regress", X)
        B = np.ascontiguousarray(basis, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] != T or not 1 <= B.shape[1] <= 16:
            raise ValueError("column_regress: the basis must be T x k with T = %d and 1 <= k <= 16, got shape %s" % (T, B.shape))
        k = B.shape[1]
        field, f_ptr, where_out = _output(alloc, (T, N), dt)
        coef = np.empty((k, N), dtype=np.float64)
        fitted = np.empty(N, dtype=np.uint8)
        self._check(self._lib.xmca_column_regress(self._h, ptr, where_in, T, N, st, sn, code, _ptr(B), k, f_ptr, where_out, _ptr(coef),
                                                  _ptr(fitted)))
        return field, coef, fitted.astype(bool)

    def column_residual(self, X, basis, coef, alloc=None):
        """The residual step of `column_regress` alone with given coefficients (xmca_column_residual): the T x N field minus
        basis @ coef at its present entries, NaN at the missing ones and in the columns whose coefficients hold a NaN."""
        keep, ptr, where_in, T, N, st, sn, code, dt = self._regress_field("column_residual", X)
        B = np.ascontiguousarray(basis, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] != T or not 1 <= B.shape[1] <= 16:
            raise ValueError("column_residual: the basis must be T x k with T = %d and 1 <= k <= 16, got shape %s" % (T, B.shape))
        k = B.shape[1]
        C = np.ascontiguousarray(coef, dtype=np.float64)
        if C.shape != (k, N):
            raise ValueError("column_residual: the coefficients must be k x N = %d x %d, got shape %s" % (k, N, C.shape))
        field, f_ptr, where_out = _output(alloc, (T, N), dt)
        self._check(self._lib.xmca_column_residual(self._h, ptr, where_in, T, N, st, sn, code, _ptr(B), k, _ptr(C), f_ptr, where_out))
        return field

    def time_filter(self, X, weights, complement=False, renormalise=False, den_min=0.0, trim=False, alloc=None):
        """The FIR filter along time of the T x N float32 / float64 field `X` (a host array or a `DeviceView`; NaN = missing) with the
        odd number L = 2 h + 1 <= 1025 of float64 `weights` (xmca_time_filter): S[t] = sum_k w[k] x[t + k - h] as one float64 fma
        chain in ascending k, or x - S with `complement`, in X's dtype.  Strict (NaN where the window holds a missing entry or
        leaves the record; `trim` returns rows h .. T - h - 1 only), or `renormalise`: S = num / den over the present entries, NaN
        where x itself is missing or den < den_min.  alloc: as in `maps` - the field is written on the device.  Resident fields and
        the result of a solve stay as they are."""
        keep, ptr, where_in, T, N, st, sn, code, dt = self._regress_field("time_filter", X)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.ndim != 1 or w.size % 2 != 1 or w.size > 1025:
            raise ValueError("time_filter: the weights must be a vector of odd length, at most 1025, got shape %s" % (w.shape,))
        L = w.size
        if trim and T < L:
            raise ValueError("time_filter: trimmed edges need at least as many time steps (%d) as weights (%d)" % (T, L))
        field, f_ptr, where_out = _output(alloc, (T - (L - 1) if trim else T, N), dt)
        self._check(self._lib.xmca_time_filter(self._h, ptr, where_in, T, N, st, sn, code, _ptr(w), L, int(bool(complement)),
                                               int(bool(renormalise)), float(den_min), int(bool(trim)), f_ptr, where_out))
        return field

    def lead_lag_maps(self, X, Yc, lags, min_pairs, rho_y=None, alloc=None):
        """The lagged regression maps of the T x N float32 / float64 field `X` (a host array or a `DeviceView`; NaN = missing) on the
        q <= 8 columns of the CENTRED, finite index plane `Yc` (T x q) at the distinct `lags` (xmca_lead_lag_maps):
        (r, slope, p, dof, pairs, lag1) - r, slope (L, N, q) in X's dtype, p (L, N, q) float64, dof (L, N, q) int32, pairs (L, N)
        int32, and lag1 (N,) float64 or None.  rho_y: None - dof = pairs; the q lag-1 autocorrelations of the index - the
        effective sample size of Bretherton et al. (1999).  alloc: as in `maps` - every output is written on the device.
        Resident fields and the result of a solve stay as they are."""
        keep, ptr, where_in, T, N, st, sn, code, dt = self._regress_field("lead_lag_maps", X)
        Y = np.ascontiguousarray(Yc, dtype=np.float64)
        if Y.ndim != 2 or Y.shape[0] != T or not 1 <= Y.shape[1] <= 8:
            raise ValueError("lead_lag_maps: the index must be T x q with T = %d and 1 <= q <= 8, got shape %s" % (T, Y.shape))
        q = Y.shape[1]
        lg = np.ascontiguousarray(lags, dtype=np.int32)
        if lg.ndim != 1 or lg.size < 1 or lg.size * q > 1024:
            raise ValueError("lead_lag_maps: it needs a lag, and at most 1024 lags x index series, got %d x %d" % (lg.size, q))
        L = lg.size
        ry = None if rho_y is None else np.ascontiguousarray(rho_y, dtype=np.float64)
        if ry is not None and ry.shape != (q,):
            raise ValueError("lead_lag_maps: rho_y must hold one value per index series (%d), got shape %s" % (q, ry.shape))
        r, r_ptr, where_out = _output(alloc, (L, N, q), dt)
        slope, s_ptr, _ = _output(alloc, (L, N, q), dt)
        p, p_ptr, _ = _output(alloc, (L, N, q), np.float64)
        dof, d_ptr, _ = _output(alloc, (L, N, q), np.int32)
        pairs, n_ptr, _ = _output(alloc, (L, N), np.int32)
        lag1, l_ptr = None, None
        if ry is not None:
            lag1, l_ptr, _ = _output(alloc, (N,), np.float64)
        self._check(self._lib.xmca_lead_lag_maps(self._h, ptr, where_in, T, N, st, sn, code, _ptr(Y), q, _ptr(lg), L, int(min_pairs),
                                                 DOF_N if ry is None else DOF_BRETHERTON, _ptr(ry), r_ptr, s_ptr, p_ptr, d_ptr, n_ptr,
                                                 l_ptr, where_out))
        return r, slope, p, dof, pairs, lag1

    def spectral_maps(self, X, Yc, nperseg, step, weights, detrend_mean, bins, fs, min_segments, alloc=None):
        """The Welch spectra of the T x N float32 / float64 field `X` (a host array or a `DeviceView`; NaN = missing) over segments of
        `nperseg` rows every `step` rows with the float64 `weights`, at the distinct `bins`, and its cross-spectra with the q <= 4
        columns of the CENTRED, finite index plane `Yc` (T x q, or None) (xmca_spectral_maps): a dict with 'power' (F, N) in X's dtype
        and 'segments' (N,) int32, and with an index 'index_power', 'cospectrum', 'quadrature', 'coherence', 'phase', 'gain' (F, N, q)
        in X's dtype and 'p' (F, N, q) float64.  alloc: as in `maps` - every output is written on the device.  Resident fields and
        the result of a solve stay as they are."""
        keep, ptr, where_in, T, N, st, sn, code, dt = self._regress_field("spectral_maps", X)
        Y, q = None, 0
        if Yc is not None:
            Y = np.ascontiguousarray(Yc, dtype=np.float64)
            if Y.ndim != 2 or Y.shape[0] != T or not 1 <= Y.shape[1] <= 4:
                raise ValueError("spectral_maps: the index must be T x q with T = %d and 1 <= q <= 4, got shape %s" % (T, Y.shape))
            q = Y.shape[1]
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (int(nperseg),):
            raise ValueError("spectral_maps: it needs nperseg = %d weights, got shape %s" % (nperseg, w.shape))
        b = np.ascontiguousarray(bins, dtype=np.int32)
        if b.ndim != 1 or b.size < 1:
            raise ValueError("spectral_maps: it needs a bin, got shape %s" % (b.shape,))
        F = b.size
        out = {}
        out['power'], pw_ptr, where_out = _output(alloc, (F, N), dt)
        out['segments'], sg_ptr, _ = _output(alloc, (N,), np.int32)
        ptrs = [None] * 7
        if q:
            for i, key in enumerate(('index_power', 'cospectrum', 'quadrature', 'coherence', 'phase', 'gain', 'p')):
                out[key], ptrs[i], _ = _output(alloc, (F, N, q), np.float64 if key == 'p' else dt)
        self._check(self._lib.xmca_spectral_maps(self._h, ptr, where_in, T, N, st, sn, code, _ptr(Y), q, int(nperseg), int(step), _ptr(w),
                                                 DETREND_MEAN if detrend_mean else DETREND_NONE, _ptr(b), F, float(fs), int(min_segments),
                                                 pw_ptr, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], ptrs[6], sg_ptr, where_out))
        return out

    def reg_mask(self, X):
        """(tests) The mask / widen pass of `column_regress` on a host field (xmca_reg_mask): (mask, wide, missing) - the T x N mask
        bytes (0 present, 1 missing), the plane widened to float64 with 0 at the missing entries, and their number."""
        X = _gap_plane("reg_mask", X)
        T, N = X.shape
        mask = np.empty((T, N), dtype=np.uint8)
        wide = np.empty((T, N), dtype=np.float64)
        missing = _c_i64(0)
        self._check(self._lib.xmca_reg_mask(self._h, _ptr(X), T, N, _np_dtype_code(X.dtype), _ptr(mask), _ptr(wide), ctypes.byref(missing)))
        return mask, wide, int(missing.value)

    def reg_solve(self, normal, rhs):
        """(tests) The solve kernel of `column_regress` on host moments (xmca_reg_solve): (coefficients k x N, fitted N bools).
        rhs: k x N; normal: (k (k + 1) / 2 + 1) x N - the packed lower triangles, entry (i, j <= i) in row i (i + 1) / 2 + j, then the
        numbers of present entries - or 1-D of that length: one matrix shared by all columns."""
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        normal = np.ascontiguousarray(normal, dtype=np.float64)
        if rhs.ndim != 2 or not 1 <= rhs.shape[0] <= 16:
            raise ValueError("reg_solve: rhs must be k x N with 1 <= k <= 16, got shape %s" % (rhs.shape,))
        k, N = rhs.shape
        rows = k * (k + 1) // 2 + 1
        if normal.shape not in ((rows,), (rows, N)):
            raise ValueError("reg_solve: normal must hold %d rows of 1 or %d values, got shape %s" % (rows, N, normal.shape))
        coef = np.empty((k, N), dtype=np.float64)
        fitted = np.empty(N, dtype=np.uint8)
        self._check(self._lib.xmca_reg_solve(self._h, _ptr(normal), int(normal.ndim == 1), _ptr(rhs), N, k, _ptr(coef), _ptr(fitted)))
        return coef, fitted.astype(bool)

    def gap_center(self, X):
        """(tests) The centring and mask kernels of `fill_gaps` on a host field (xmca_gap_center): (mean, mask, A, scale) - the N column
        means over the present entries, the T x N mask bytes (0 present, 1 missing), the centred plane widened to float64 and the RMS
        of the present anomalies."""
        X = _gap_plane("gap_center", X)
        T, N = X.shape
        mean = np.empty(N, dtype=np.float64)
        mask = np.empty((T, N), dtype=np.uint8)
        A = np.empty((T, N), dtype=np.float64)
        scale = _c_dbl(0.0)
        self._check(self._lib.xmca_gap_center(self._h, _ptr(X), T, N, _np_dtype_code(X.dtype), _ptr(mean), _ptr(mask), _ptr(A),
                                              ctypes.byref(scale)))
        return mean, mask, A, float(scale.value)

    def gap_fill_step(self, A, mask, Z, P):
        """(tests) The fill kernel of `fill_gaps` on host inputs (xmca_gap_fill_step): (A_new, sum) - the T x N float32 / float64 plane
        `A` with Z.T @ P written where `mask` (T x N bytes) is non-zero, Z n_modes x T and P n_modes x N in float64, and the sum of
        the squared changes."""
        A = _gap_plane("gap_fill_step", A)
        T, N = A.shape
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        P = np.ascontiguousarray(P, dtype=np.float64)
        if mask.shape != (T, N) or Z.ndim != 2 or Z.shape[0] < 1 or Z.shape[1] != T or P.shape != (Z.shape[0], N):
            raise ValueError("gap_fill_step: need a T x N mask, Z of k x T and P of k x N, got %s, %s, %s" % (mask.shape, Z.shape, P.shape))
        out = np.empty_like(A)
        total = _c_dbl(0.0)
        self._check(self._lib.xmca_gap_fill_step(self._h, _ptr(A), _ptr(mask), _ptr(Z), _ptr(P), T, N, Z.shape[0], _np_dtype_code(A.dtype),
                                                 _ptr(out), ctypes.byref(total)))
        return out, float(total.value)

    def gap_lag_fill_step(self, A, mask, Z, P, embedding, tau):
        """(tests) The lagged fill kernel of `fill_gaps(embedding=)` on host inputs (xmca_gap_lag_fill_step): (A_new, sum) - the T x N
        float32 / float64 plane `A` with the diagonally averaged sum_j Z[:, t - j tau] . P[j k : (j + 1) k, n] written where `mask`
        (T x N bytes) is non-zero, Z k x T' and P embedding k x N in float64, T' = T - (embedding - 1) tau, and the sum of the squared
        changes."""
        A = _gap_plane("gap_lag_fill_step", A)
        T, N = A.shape
        M, tau = int(embedding), int(tau)
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        P = np.ascontiguousarray(P, dtype=np.float64)
        if M < 1 or tau < 1:
            raise ValueError("gap_lag_fill_step: embedding and tau must be at least 1")
        if mask.shape != (T, N) or Z.ndim != 2 or Z.shape[0] < 1 or Z.shape[1] != T - (M - 1) * tau or P.shape != (M * Z.shape[0], N):
            raise ValueError("gap_lag_fill_step: need a T x N mask, Z of k x T' and P of embedding k x N, got %s, %s, %s"
                             % (mask.shape, Z.shape, P.shape))
        out = np.empty_like(A)
        total = _c_dbl(0.0)
        self._check(self._lib.xmca_gap_lag_fill_step(self._h, _ptr(A), _ptr(mask), _ptr(Z), _ptr(P), T, N, Z.shape[0], M, tau,
                                                     _np_dtype_code(A.dtype), _ptr(out), ctypes.byref(total)))
        return out, float(total.value)

    def lag_expand(self, Z, embedding, tau, with_indicators):
        """(tests) The placement kernel of `extended_reconstruct` on a host matrix (xmca_lag_expand): (A, inv_count) from the q x T'
        float64 `Z` - A is T x embedding (q + 1) with the indicator columns, T x embedding q without, T = T' + (embedding - 1) tau;
        A[t, j q + c] = Z[c, t - j tau] inside window j, else 0; inv_count[t] = 1 / (number of windows that hold t)."""
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        M, tau = int(embedding), int(tau)
        if Z.ndim != 2 or Z.shape[0] < 1 or Z.shape[1] < 1:
            raise ValueError("lag_expand: Z must be a q x T' matrix, got shape %s" % (Z.shape,))
        q, n_win = Z.shape
        if M < 1 or tau < 1 or (M > 1 and tau > n_win):
            raise ValueError("lag_expand: embedding and tau must be >= 1, and tau <= T' when embedding > 1")
        T = n_win + (M - 1) * tau
        A = np.empty((T, M * (q + (1 if with_indicators else 0))), dtype=np.float64)
        inv_count = np.empty(T, dtype=np.float64)
        self._check(self._lib.xmca_lag_expand(self._h, _ptr(Z), q, n_win, M, tau, int(bool(with_indicators)), _ptr(A), _ptr(inv_count)))
        return A, inv_count

    def lag_window_means(self, T, N, embedding, tau):
        """(tests) The means of the `embedding` windows X[j tau : j tau + T'] of every column of the resident real T x N field of side
        0 (xmca_lag_window_means): embedding x N float64, summed in float64 in one pass over the field."""
        M, tau = int(embedding), int(tau)
        if M < 1 or tau < 1 or int(T) - (M - 1) * tau < 1:
            raise ValueError("lag_window_means: embedding and tau must be >= 1 with (embedding - 1) * tau below T")
        out = np.empty((M, int(N)), dtype=np.float64)
        self._check(self._lib.xmca_lag_window_means(self._h, M, tau, _ptr(out)))
        return out

    def extended_reconstruct(self, T, N, embedding, tau, modes, add_means, keep_idx=None, N_full=None, mean=None, std=None,
                             inv_weight=None, alloc=None):
        """The reconstructed component of the 0-based, increasing extended modes `modes` of the resident real T x N field of side 0
        (xmca_extended_reconstruct): T x N_full float64, the diagonal averaging of the truncated lag-embedded matrix, plus the
        window means when `add_means`, then / inv_weight, * std, + mean (None: left out), NaN at the columns not in keep_idx
        (None: N_full = N).  alloc: as in `reconstruct` - the result is written on the device.  The result of a solve and the fields
        stay as they are."""
        M, tau, T, N = int(embedding), int(tau), int(T), int(N)
        n_win = T - (M - 1) * tau
        sel = np.ascontiguousarray(modes, dtype=np.intc).reshape(-1)
        if M < 1 or tau < 1 or n_win < 2 or (M > 1 and tau > n_win):
            raise ValueError("extended_reconstruct: embedding, tau >= 1, T' >= 2 and tau <= T' (embedding > 1) are needed")
        if sel.size < 1 or sel[0] < 0 or sel[-1] >= min(n_win - 1, M * N) or np.any(np.diff(sel) <= 0):
            raise ValueError("extended_reconstruct: modes must be increasing 0-based indices below min(T' - 1, embedding * N)")
        idx = _kept_index("extended_reconstruct", keep_idx, N)
        N_full = N if N_full is None else int(N_full)
        mean = None if mean is None else np.ascontiguousarray(np.broadcast_to(mean, (N,)), dtype=np.float64)
        std = None if std is None else np.ascontiguousarray(np.broadcast_to(std, (N,)), dtype=np.float64)
        inv_weight = None if inv_weight is None else _column_weights("extended_reconstruct", inv_weight, N)
        out, out_ptr, where = _output(alloc, (T, N_full), np.float64)
        self._check(self._lib.xmca_extended_reconstruct(self._h, M, tau, _ptr(sel), int(sel.size), int(bool(add_means)), _ptr(idx), N, N_full,
                                                        _ptr(mean), _ptr(std), _ptr(inv_weight), out_ptr, where))
        return out

    # ---- instrumentation ----------------------------------------------------------------------
    def reduction_info(self):
        """names of the kernels of the last tridiagonal reduction (xmca_get_reduction_info)"""
        buf = ctypes.create_string_buffer(4096)
        n = self._lib.xmca_get_reduction_info(self._h, buf, 4096)
        if n < 0:
            self._check(n)
        return buf.value.decode()

    def timings(self):
        names = ctypes.create_string_buffer(4096)
        ms = np.zeros(64)
        n = self._lib.xmca_get_timings(self._h, names, 4096, _ptr(ms), 64)
        if n < 0:
            self._check(n)
        keys = names.value.decode().split(";") if n > 0 else []
        return {k: float(ms[i]) for i, k in enumerate(keys[:n])}

    def reset_timings(self):
        self._check(self._lib.xmca_reset_timings(self._h))

    def fft(self, x, sign=-1):
        """Batched DFT along the last axis of a 2-D array (rows), numpy.fft.fft convention for sign = -1 (csrc/fft.h)."""
        x = np.asarray(x)
        re = np.ascontiguousarray(x.real, dtype=np.float64)
        im = np.ascontiguousarray(x.imag, dtype=np.float64) if np.iscomplexobj(x) else None
        out_r, out_i = np.empty_like(re), np.empty_like(re)
        self._check(self._lib.xmca_fft(self._h, _ptr(re), _ptr(im), re.shape[0], re.shape[1], int(sign), _ptr(out_r), _ptr(out_i)))
        return out_r + 1j * out_i

    def pool_bytes(self):
        """device memory the handle keeps for re-use (solver temporaries; include/xmca_hip.h xmca_pool_bytes)"""
        n = ctypes.c_int64(0)
        self._check(self._lib.xmca_pool_bytes(self._h, ctypes.byref(n)))
        return int(n.value)

    def trim_pool(self):
        """give the kept device memory back to the driver"""
        self._check(self._lib.xmca_trim_pool(self._h))

    # ---- kernel-level entry points --------------------------------------------------------------
    @staticmethod
    def _gemm_operand(X, ld, dtype=None):
        """One operand of gemm / gemm_ex and its leading dimension.  Without `ld`: a contiguous copy, ld = its width.  With
        `ld`: X is the view buf[:, :width] of a C-contiguous (rows, ld) array - rows `ld` elements apart, and all
        rows * ld elements behind its first one exist, since the entry point uploads that many."""
        if ld is None:
            X = np.ascontiguousarray(X, dtype=dtype)
            return X, X.shape[1]
        ld = int(ld)
        root = X
        while isinstance(root.base, np.ndarray):
            root = root.base
        rows, width = X.shape
        it = X.itemsize
        ok = (X.ndim == 2 and (dtype is None or X.dtype == dtype) and ld >= width and X.strides[1] == it
              and (rows == 1 or X.strides[0] == ld * it) and root.flags.c_contiguous
              and X.ctypes.data + rows * ld * it <= root.ctypes.data + root.nbytes)
        if not ok:
            raise ValueError("gemm: with a leading dimension the operand must be buf[:, :width] of a contiguous (rows, ld) array")
        return X, ld

    def _gemm_shapes(self, A, B, a_kfast, b_nfast, lda, ldb):
        A, lda = self._gemm_operand(A, lda)
        B, ldb = self._gemm_operand(B, ldb, A.dtype)
        M, K = A.shape if a_kfast else A.shape[::-1]
        Kb, N = B.shape if b_nfast else B.shape[::-1]
        if K != Kb:
            raise ValueError("gemm: inner dimensions differ")
        return A, B, M, N, K, lda, ldb, _np_dtype_code(A.dtype)

    def gemm(self, A, B, a_kfast=True, b_nfast=True, alpha=1.0, upper_only=False, mirror=0, splits=0, lda=None, ldb=None):
        """C = alpha * op(A) op(B); A: (M,K) if a_kfast else (K,M); B: (K,N) if b_nfast else (N,K).  `lda` / `ldb`: rows
        of the operand that many elements apart (see _gemm_operand); default: its width."""
        A, B, M, N, K, lda, ldb, code = self._gemm_shapes(A, B, a_kfast, b_nfast, lda, ldb)
        C = np.zeros((M, N), dtype=np.float64)
        self._check(self._lib.xmca_gemm(self._h, _ptr(A), lda, int(a_kfast), _ptr(B), ldb, int(b_nfast),
                                        _ptr(C), M, N, K, code, float(alpha), int(upper_only), int(mirror), int(splits)))
        return C

    def gemm_ex(self, A, B, C, a_kfast=True, b_nfast=True, alpha=1.0, beta=0.0, row_scale=None, col_scale=None, upper_only=False,
                mirror=0, splits=0, lda=None, ldb=None):
        """alpha * row_scale[:, None] * col_scale[None, :] * op(A) op(B) + beta * C, returned in a copy of C: float64 or
        float32, (M, ldc) with ldc >= N - the columns from N on come back as they went in (xmca_gemm_ex)."""
        A, B, M, N, K, lda, ldb, code = self._gemm_shapes(A, B, a_kfast, b_nfast, lda, ldb)
        C = np.array(C, order="C", copy=True)
        if C.ndim != 2 or C.shape[0] != M or C.shape[1] < N:
            raise ValueError("gemm_ex: C must be (M, ldc) with ldc >= N")
        rs = None if row_scale is None else np.ascontiguousarray(row_scale, dtype=np.float64)
        cs = None if col_scale is None else np.ascontiguousarray(col_scale, dtype=np.float64)
        if (rs is not None and rs.shape != (M,)) or (cs is not None and cs.shape != (N,)):
            raise ValueError("gemm_ex: row_scale has M and col_scale N elements")
        self._check(self._lib.xmca_gemm_ex(self._h, _ptr(A), lda, int(a_kfast), _ptr(B), ldb, int(b_nfast), _ptr(C), C.shape[1],
                                           _np_dtype_code(C.dtype), M, N, K, code, float(alpha), float(beta), _ptr(rs), _ptr(cs),
                                           int(upper_only), int(mirror), int(splits)))
        return C

    def eigh(self, A, vectors=True, n_lead=None):
        """Returns (lam descending, U) with A = U diag(lam) U^H; `vectors=False`: (lam, None), eigenvalues only.  `n_lead=k`: all
        eigenvalues, and U (n x k) of the k leading ones only, posed as solve(n_modes=k) poses it (xmca_eigh_lead);
        `last_eigh_info` then also says how many vectors were formed (`n_eigvec`) and whether the guard row and padding columns
        around the k x n result came back untouched (`guard_rows_clean`; None without `n_lead`)."""
        Ad, cplx = _host_vectors(A)
        n = Ad.shape[0]
        lam = np.empty(n)
        if n_lead is None:
            Zh = np.empty((n, n), dtype=Ad.dtype) if vectors else None
            info = np.zeros(4, dtype=np.int32)
            self._check(self._lib.xmca_eigh(self._h, _ptr(Ad), n, int(cplx), _ptr(lam), _ptr(Zh) if vectors else None, _ptr(info)))
            n_eigvec, clean = (n if vectors else 0), None
        else:
            if not vectors or isinstance(n_lead, bool) or int(n_lead) != n_lead or not 1 <= n_lead <= n:
                raise ValueError("eigh: n_lead is an integer between 1 and n, and needs vectors=True")
            Zh = np.empty((int(n_lead), n), dtype=Ad.dtype)
            info = np.zeros(6, dtype=np.int32)
            self._check(self._lib.xmca_eigh_lead(self._h, _ptr(Ad), n, int(cplx), int(n_lead), _ptr(lam), _ptr(Zh), _ptr(info)))
            n_eigvec, clean = int(info[4]), bool(info[5])
        self.last_eigh_info = {"sweeps": int(info[0]), "tile": int(info[1]), "slots": int(info[2]), "lr_step": int(info[3]) & 1,
                               "tridiag": (int(info[3]) >> 1) & 1, "n_eigvec": n_eigvec, "guard_rows_clean": clean}
        return lam, (Zh.conj().T if vectors else None)

    def cholesky(self, A, rel_shift=0.0):
        """Returns (R upper triangular with R^H R = A + rel_shift max(diag A) I, ok)."""
        Ad, cplx = _host_vectors(A)
        n = Ad.shape[0]
        R = np.empty((n, n), dtype=Ad.dtype)
        ok = _c_int(0)
        self._check(self._lib.xmca_cholesky(self._h, _ptr(Ad), n, int(cplx), float(rel_shift), _ptr(R), ctypes.byref(ok)))
        return R, bool(ok.value)

    def cholesky_ex(self, A, first=0, lda=None, rel_shift=0.0):
        """The factorisation of the trailing block A[first:n, first:n] inside a buffer of n rows of lda >= n elements, posed
        as the one-sided solves pose it (xmca_cholesky_ex).  A: (n, n), padded here to (n, lda) with NaN, or (n, lda) as it
        is.  Returns (the whole buffer as it comes back, ok): the block holds R, everything else what it held before."""
        Ad, cplx = _host_vectors(A)
        n = Ad.shape[0]
        lda = Ad.shape[1] if lda is None else int(lda)
        if Ad.ndim != 2 or lda < n or Ad.shape[1] not in (n, lda):
            raise ValueError("cholesky_ex: A must be (n, n) or (n, lda) with lda >= n")
        if Ad.shape[1] != lda:
            buf = np.full((n, lda), np.nan, dtype=Ad.dtype)
            buf[:, :n] = Ad
            Ad = buf
        R = np.empty_like(Ad)
        ok = _c_int(0)
        self._check(self._lib.xmca_cholesky_ex(self._h, _ptr(Ad), n, lda, int(first), int(cplx), float(rel_shift), _ptr(R),
                                               ctypes.byref(ok)))
        return R, bool(ok.value)

    def lead_rows(self, A, B, b_kfast, K, n, scale=None, out=None):
        """out[r, j] = scale[r] * sum_k A[r, k] B(k, j) by the skinny kernel of the one-field solve (xmca_lead_rows): A is
        (rows <= 16, lda >= K); B is (n, ldb >= K) when b_kfast - B(k, j) = B[j, k] - and (K, ldb >= n) otherwise; only the
        leading K (or n) columns of a row are operands, the rest is padding.  `out`: the (rows, ldo >= n) buffer as it is
        before the call (default: NaN, ldo = n).  Returns (a copy of it with the product written, the number of pieces the
        contraction was cut into)."""
        Ad = np.ascontiguousarray(A, dtype=np.float64)
        Bd = np.ascontiguousarray(B, dtype=np.float64)
        rows = Ad.shape[0]
        if Ad.ndim != 2 or Bd.ndim != 2 or Ad.shape[1] < K or Bd.shape != ((n, Bd.shape[1]) if b_kfast else (K, Bd.shape[1])):
            raise ValueError("lead_rows: A is (rows, lda >= K), B is (n, ldb) or (K, ldb)")
        od = np.full((rows, n), np.nan) if out is None else np.array(out, dtype=np.float64, order="C", copy=True)
        sd = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
        if od.shape[0] != rows or (sd is not None and sd.size != rows):
            raise ValueError("lead_rows: out and scale have one row / entry per row of A")
        chunks = _c_int(0)
        self._check(self._lib.xmca_lead_rows(self._h, _ptr(Ad), Ad.shape[1], _ptr(Bd), Bd.shape[1], int(bool(b_kfast)), rows, int(K),
                                             int(n), None if sd is None else _ptr(sd), _ptr(od), od.shape[1], ctypes.byref(chunks)))
        return od, chunks.value

    def fft_ex(self, in_re, in_im, batch, n, out_re, out_im, sign=-1, in_bs=None, in_es=1, n_in=None, conj_in=False, sin=None,
               out_bs=None, out_es=1, n_keep=None, sa=None, sb=None, scale=1.0):
        """fft_batch of csrc/fft.h with every argument (xmca_fft_ex): element (b, t) of the input at in_re[b*in_bs + t*in_es]
        of the flattened buffers, element (b, k) of the output at out[b*out_bs + k*out_es]; out_re / out_im are the buffers as
        they are before the call.  Returns copies of them (same shapes) with the n_keep outputs of every transform written."""
        n_in = n if n_in is None else int(n_in)
        n_keep = n if n_keep is None else int(n_keep)
        in_bs = n_in if in_bs is None else int(in_bs)
        out_bs = n_keep if out_bs is None else int(out_bs)
        ir = np.ascontiguousarray(in_re, dtype=np.float64)
        ii = None if in_im is None else np.ascontiguousarray(in_im, dtype=np.float64)
        if ii is not None and ii.size != ir.size:
            raise ValueError("fft_ex: in_re and in_im differ in size")
        outr = np.array(out_re, dtype=np.float64, order="C", copy=True)
        outi = np.array(out_im, dtype=np.float64, order="C", copy=True)
        if outr.size != outi.size:
            raise ValueError("fft_ex: out_re and out_im differ in size")
        fs = None if sin is None else np.ascontiguousarray(sin, dtype=np.float64)
        fa = None if sa is None else np.ascontiguousarray(sa, dtype=np.float64)
        fb = None if sb is None else np.ascontiguousarray(sb, dtype=np.float64)
        if ((fs is not None and fs.size != n_in) or (fa is not None and fa.size != n_keep) or (fb is not None and fb.size != batch)):
            raise ValueError("fft_ex: sin has n_in, sa n_keep and sb batch elements")
        self._check(self._lib.xmca_fft_ex(self._h, _ptr(ir), _ptr(ii), ir.size, in_bs, int(in_es), n_in, int(bool(conj_in)), _ptr(fs),
                                          int(batch), int(n), int(sign), _ptr(outr), _ptr(outi), outr.size, out_bs, int(out_es),
                                          n_keep, _ptr(fa), _ptr(fb), float(scale)))
        return outr, outi

    @staticmethod
    def _tridiagonal(what, d, e):
        """(d, e, n) of a symmetric tridiagonal matrix as contiguous float64: d has n >= 1 entries, e n - 1 (None: none)."""
        dd = np.ascontiguousarray(d, dtype=np.float64)
        ee = np.zeros(0) if e is None else np.ascontiguousarray(e, dtype=np.float64)
        if dd.ndim != 1 or ee.ndim != 1 or dd.size < 1 or ee.size != dd.size - 1:
            raise ValueError("%s: d has n >= 1 entries and e n - 1, got shapes %s and %s" % (what, dd.shape, ee.shape))
        return dd, ee, int(dd.size)

    def tridiag_eigenvalues(self, d, e):
        """All eigenvalues, descending, of the symmetric tridiagonal matrix with diagonal d (n) and off-diagonal e (n - 1) by the
        Sturm multisection kernel of the eigensolver alone, scaled and launched as a solve does it (xmca_tridiag_eigenvalues)."""
        dd, ee, n = Handle._tridiagonal("tridiag_eigenvalues", d, e)
        lam = np.empty(n)
        self._check(self._lib.xmca_tridiag_eigenvalues(self._h, _ptr(dd), _ptr(ee) if n > 1 else None, n, _ptr(lam)))
        return lam

    def tridiag_vectors(self, d, e, lam, out=None):
        """The unit eigenvectors of the tridiagonal matrix (d, e) for the nev <= n eigenvalues `lam` (ascending, the caller's) by
        the twisted-factorisation kernel of the eigensolver alone (xmca_tridiag_vectors).  `out`: the (n, ldy >= nev) plane as it
        is before the call (default: NaN, ldy = nev).  Returns a copy of it with column k the vector of lam[k]."""
        dd, ee, n = Handle._tridiagonal("tridiag_vectors", d, e)
        ll = np.ascontiguousarray(lam, dtype=np.float64)
        if ll.ndim != 1 or not 1 <= ll.size <= n:
            raise ValueError("tridiag_vectors: lam holds between 1 and n eigenvalues, got shape %s" % (ll.shape,))
        Y = np.full((n, ll.size), np.nan) if out is None else np.array(out, dtype=np.float64, order="C", copy=True)
        if Y.ndim != 2 or Y.shape[0] != n or Y.shape[1] < ll.size:
            raise ValueError("tridiag_vectors: out is (n, ldy >= nev), got shape %s" % (Y.shape,))
        self._check(self._lib.xmca_tridiag_vectors(self._h, _ptr(dd), _ptr(ee) if n > 1 else None, n, _ptr(ll), int(ll.size), _ptr(Y),
                                                   Y.shape[1]))
        return Y

    def bench_gemm(self, M, N, K, dtype, a_kfast=True, b_nfast=True, upper_only=False, splits=0, reps=5):
        """ms per product C = op(A) op(B) on device-resident random operands."""
        ms = _c_dbl(0)
        self._check(self._lib.xmca_bench_gemm(self._h, M, N, K, _np_dtype_code(dtype), int(a_kfast), int(b_nfast), int(upper_only),
                                              int(splits), int(reps), ctypes.byref(ms)))
        return ms.value

    def bench_gram(self, side, reps):
        a, k, f = _c_dbl(0), _c_dbl(0), _c_dbl(0)
        self._check(self._lib.xmca_bench_gram(self._h, side, reps, ctypes.byref(a), ctypes.byref(k), ctypes.byref(f)))
        return {"avg_ms": a.value, "kernel_ms": k.value, "flops": f.value}


_default = {}


def default_handle(device=None):
    """Process-wide handle per device (LOCAL_RANK selects the device when not given)."""
    if device is None:
        device = int(os.environ.get("XMCA_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        n = load_library().xmca_device_count()
        if n > 0:
            device %= n
    if device not in _default:
        _default[device] = Handle(device)
    return _default[device]


COMM_ID_BYTES = 128


def comm_unique_id():
    """An ncclUniqueId (128 bytes) made by rank 0 for `Comm`; NotImplementedError when RCCL cannot be loaded."""
    lib = load_library()
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    rc = lib.xmca_comm_unique_id(buf)
    if rc != 0:
        _raise(rc, "xmca_comm_unique_id failed (RCCL not available?)")
    return buf.raw


class Comm:
    """RCCL communicator of the C ABI (xmca_comm_*): one per process / GPU, created collectively by all `world` ranks from
    the unique id rank 0 made.  The only collective of the path is the all-gather of the rule_n spectra."""

    def __init__(self, handle, unique_id, rank, world):
        self._lib = load_library()
        self._c = None
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("unique id must be %d bytes" % COMM_ID_BYTES)
        out = _vp()
        rc = self._lib.xmca_comm_create(handle._h, ctypes.c_char_p(bytes(unique_id)), int(rank), int(world), ctypes.byref(out))
        if rc != 0:
            handle._check(rc)
        self._c = out
        self._fin = weakref.finalize(self, self._lib.xmca_comm_destroy, out)

    def _check(self, rc):
        if rc != 0:
            _raise(rc, (self._lib.xmca_comm_last_error(self._c) or b"").decode())

    def allgather(self, local):
        local = np.ascontiguousarray(local, dtype=np.float64)
        rank, world, _, _ = self.info()
        out = np.empty((world,) + local.shape, dtype=np.float64)
        self._check(self._lib.xmca_comm_allgather(self._c, _ptr(local), _ptr(out), local.size))
        return out

    def broadcast(self, values, root=0):
        buf = np.ascontiguousarray(values, dtype=np.float64).copy()
        self._check(self._lib.xmca_comm_broadcast(self._c, _ptr(buf), buf.size, int(root)))
        return buf

    def info(self):
        r, w = _c_int(), _c_int()
        n, b = _c_i64(), _c_i64()
        self._check(self._lib.xmca_comm_info(self._c, ctypes.byref(r), ctypes.byref(w), ctypes.byref(n), ctypes.byref(b)))
        return r.value, w.value, n.value, b.value

    def close(self):
        if self._c is not None:
            self._fin()
            self._c = None
