"""ctypes binding of the C ABI in ``include/chicdiff_hip.h`` (``chicdiff_amd/lib/libchicdiff_hip.so``).

This is the product path: there is NO CPU fallback.  If the shared library has not been
built, or no MI355X is visible, construction raises — it never routes to ``oracle/``.
PyTorch is used only as plumbing: device buffers (``torch.Tensor``), the current HIP stream,
and ``torch.distributed`` for the sum-all-reduce hook.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .dist import ALLGATHER_FN, ALLREDUCE_FN

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libchicdiff_hip.so")

ST_TREND_FAILED, ST_PRIORVAR_MC, ST_BETA_NONCONV, ST_ALLZERO_ROWS, ST_TREND_LOCAL = 1, 2, 4, 8, 16


# every symbol include/chicdiff_hip.h declares (tests check the library exports each)
EXPORTS = [
    "chicdiff_hip_create", "chicdiff_hip_destroy", "chicdiff_hip_last_error", "chicdiff_hip_set_stream",
    "chicdiff_hip_set_allreduce", "chicdiff_hip_set_allgather", "chicdiff_hip_last_refits", "chicdiff_hip_set_option", "chicdiff_hip_default_opts", "chicdiff_hip_size_factors_dev",
    "chicdiff_hip_offsets_dev", "chicdiff_hip_window_sums_dev", "chicdiff_hip_count_join_dev",
    "chicdiff_hip_fragment_background_dev", "chicdiff_hip_bh_adjust_dev", "chicdiff_hip_ihw_apply_dev",
    "chicdiff_hip_ihw_train_dev", "chicdiff_hip_ihw_caps", "chicdiff_hip_selftest_ihw_knots_dev", "chicdiff_hip_selftest_ihw_orient",
    "chicdiff_hip_region_universe_count_dev", "chicdiff_hip_region_universe_fill_dev", "chicdiff_hip_region_universe_dev", "chicdiff_hip_count_table_dev",
    "chicdiff_hip_candidate_interactions_dev", "chicdiff_hip_candidate_interactions_method_dev", "chicdiff_hip_selftest_landau_dev", "chicdiff_hip_chicago_tables_dev", "chicdiff_hip_chicago_tables_caps",
    "chicdiff_hip_control_draws_dev", "chicdiff_hip_countput_dev", "chicdiff_hip_countput_caps",
    "chicdiff_hip_table_check", "chicdiff_hip_table_text_dev", "chicdiff_hip_table_write_dev", "chicdiff_hip_table_text_caps",
    "chicdiff_hip_selftest_format_double_dev", "chicdiff_hip_selftest_format_double",
    "chicdiff_hip_chinput_read", "chicdiff_hip_chinput_table_dev", "chicdiff_hip_region_avdist_dev",
    "chicdiff_hip_chinput_parse_dev", "chicdiff_hip_chinput_read_dev", "chicdiff_hip_chinput_caps",
    "chicdiff_hip_peaks_parse_dev", "chicdiff_hip_peaks_read_dev", "chicdiff_hip_peaks_columns_dev", "chicdiff_hip_peaks_filter_dev",
    "chicdiff_hip_peaks_caps", "chicdiff_hip_selftest_peaks",
    "chicdiff_hip_peaks_textkeys_dev", "chicdiff_hip_peaks_merge_dev", "chicdiff_hip_peaks_header", "chicdiff_hip_selftest_peaks_textkeys",
    "chicdiff_hip_count_join_inner_dev", "chicdiff_hip_count_join_multi_dev", "chicdiff_hip_region_assemble_dev",
    "chicdiff_hip_count_tables_merge_dev",
    "chicdiff_hip_malloc", "chicdiff_hip_free", "chicdiff_hip_outstanding_allocations", "chicdiff_hip_memcpy_h2d", "chicdiff_hip_memcpy_d2h",
    "chicdiff_hip_rccl_unique_id", "chicdiff_hip_rccl_init", "chicdiff_hip_cooks_filter_dev",
    "chicdiff_hip_independent_filtering_dev",
    "chicdiff_hip_nbglm_fit_dev", "chicdiff_hip_nbglm_fit", "chicdiff_hip_wald_test_dev", "chicdiff_hip_theta_grid_dev",
    "chicdiff_hip_wald_pvalues_dev", "chicdiff_hip_selftest_math_dev", "chicdiff_hip_selftest_math3_dev", "chicdiff_hip_selftest_objective_dev", "chicdiff_hip_selftest_global_stage_dev", "chicdiff_hip_selftest_resid_hist_dev", "chicdiff_hip_selftest_r_random", "chicdiff_hip_selftest_sched_class", "chicdiff_hip_selftest_queue_claim", "chicdiff_hip_selftest_trend_exchange", "chicdiff_hip_selftest_sf_bin",
    "chicdiff_hip_selftest_prior_mc", "chicdiff_hip_selftest_chinput", "chicdiff_hip_kernel_times", "chicdiff_hip_enable_timing",
]


class Opts(C.Structure):
    _fields_ = [("minDisp", C.c_double), ("dispTol", C.c_double), ("kappa0", C.c_double),
                ("maxit", C.c_int32), ("betaMaxit", C.c_int32), ("betaTol", C.c_double),
                ("minmu", C.c_double), ("outlierSD", C.c_double), ("dispPriorVar", C.c_double),
                ("trendCoef", C.c_double * 2), ("fitType", C.c_int32), ("_pad", C.c_int32)]


OUT_DOUBLE = ["baseMean", "baseVar", "dispGeneEst", "dispFit", "dispMAP", "dispersion", "log2FoldChange",
              "lfcSE", "stat", "pvalue", "intercept", "interceptSE", "deviance", "maxCooks"]
OUT_INT = ["dispGeneIter", "dispIter", "dispOutlier", "betaConv", "betaIter", "allZero", "cooksArgmax"]
FIT_COLUMNS = ["baseMean", "dispersion", "log2FoldChange", "lfcSE", "stat", "pvalue"]   # what a device fit returns unless told otherwise


_OUT_COLUMNS = {k: (f"outputs[{k!r}]", k in OUT_DOUBLE) for k in OUT_DOUBLE + OUT_INT}   # name -> (its argument's name, float64?)


class Out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in OUT_DOUBLE + OUT_INT]


class Scalars(C.Structure):
    _fields_ = [("trendCoef", C.c_double * 2), ("varLogDispEsts", C.c_double), ("dispPriorVar", C.c_double),
                ("sumDeviance", C.c_double), ("nAllZero", C.c_int64), ("trendOuterIter", C.c_int32),
                ("status", C.c_int32)]


class ResultsInfo(C.Structure):
    _fields_ = [("filterThreshold", C.c_double), ("filterTheta", C.c_double), ("alpha", C.c_double), ("index", C.c_int32),
                ("_pad", C.c_int32), ("theta", C.c_double * 50), ("numRej", C.c_double * 50), ("lowess", C.c_double * 50)]


IHW_MAX_FOLDS = 16   # CHICDIFF_IHW_MAX_FOLDS (include/chicdiff_hip.h)


class IhwInfo(C.Structure):
    """chicdiff_ihw_info (include/chicdiff_hip.h)."""
    _fields_ = [("m", C.c_int64), ("nbins", C.c_int32), ("nfolds", C.c_int32), ("chunk_len", C.c_int32), ("_pad", C.c_int32),
                ("nseg", C.c_int64 * IHW_MAX_FOLDS), ("T", C.c_double * IHW_MAX_FOLDS), ("H", C.c_double * IHW_MAX_FOLDS)]


class TableColumn(C.Structure):
    """chicdiff_table_column (include/chicdiff_hip.h)."""
    _fields_ = [("kind", C.c_int32), ("ndict", C.c_int32), ("d_data", C.c_void_p), ("dict_off", C.c_void_p), ("dict_bytes", C.c_void_p)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ms", C.c_double), ("launches", C.c_int32), ("_pad", C.c_int32), ("bytes", C.c_double)]


CAND_METHODS = {"min": 0, "hmp": 1}   # CHICDIFF_CAND_MIN, CHICDIFF_CAND_HMP (include/chicdiff_hip.h)


class ChicdiffHipError(RuntimeError):
    pass


_lib = None


def load_library() -> C.CDLL:
    """Load the HIP library; raise (never fall back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: it ships its own ROCm runtime (libamdhip64 & co.), and whichever copy is loaded first serves the
    # whole process.  Loading this library before torch would bind everybody to /opt/rocm's copy, which torch's
    # build does not match ("no ROCm-capable device is detected").
    import torch  # noqa: F401

    path = os.environ.get("CHICDIFF_HIP_LIB", LIB_PATH)  # (override: A/B runs of two builds)
    if not os.path.exists(path):
        raise ChicdiffHipError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
    L = C.CDLL(path)
    vp, i64, i32, dbl = C.c_void_p, C.c_int64, C.c_int32, C.c_double
    L.chicdiff_hip_create.argtypes = [C.POINTER(vp), i32]
    L.chicdiff_hip_destroy.argtypes = [vp]
    L.chicdiff_hip_destroy.restype = None
    L.chicdiff_hip_last_error.argtypes = [vp]
    L.chicdiff_hip_last_error.restype = C.c_char_p
    L.chicdiff_hip_set_stream.argtypes = [vp, vp]
    L.chicdiff_hip_set_allreduce.argtypes = [vp, ALLREDUCE_FN, vp, i32, i32]
    L.chicdiff_hip_set_allgather.argtypes = [vp, ALLGATHER_FN, vp]
    L.chicdiff_hip_last_refits.argtypes = [vp]
    L.chicdiff_hip_last_refits.restype = i32
    L.chicdiff_hip_set_option.argtypes = [vp, C.c_char_p, i64]
    L.chicdiff_hip_default_opts.argtypes = [C.POINTER(Opts)]
    L.chicdiff_hip_default_opts.restype = None
    L.chicdiff_hip_size_factors_dev.argtypes = [vp, vp, i64, i32, C.POINTER(dbl)]
    L.chicdiff_hip_offsets_dev.argtypes = [vp, vp, C.POINTER(dbl), i64, i32, dbl, vp]
    L.chicdiff_hip_window_sums_dev.argtypes = [vp, vp, vp, i64, i32, vp, i64, vp, vp]
    L.chicdiff_hip_count_join_dev.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp]
    L.chicdiff_hip_fragment_background_dev.argtypes = [vp, vp, vp, i64, i32, i32, vp, i32, vp, vp, vp, vp, vp, i32, i32,
                                                       C.POINTER(dbl), vp, vp, vp]
    L.chicdiff_hip_cooks_filter_dev.argtypes = [vp, vp, i64, i32, C.POINTER(i32), vp, vp, dbl, vp, C.POINTER(i64)]
    L.chicdiff_hip_independent_filtering_dev.argtypes = [vp, vp, vp, i64, dbl, vp, C.POINTER(ResultsInfo)]
    L.chicdiff_hip_rccl_unique_id.argtypes = [vp, C.c_char_p, vp]
    L.chicdiff_hip_rccl_init.argtypes = [vp, C.c_char_p, vp, i32, i32]
    L.chicdiff_hip_malloc.argtypes = [vp, C.c_uint64, C.POINTER(vp)]
    L.chicdiff_hip_free.argtypes = [vp, vp]
    L.chicdiff_hip_outstanding_allocations.argtypes = [vp]
    L.chicdiff_hip_outstanding_allocations.restype = i64
    L.chicdiff_hip_memcpy_h2d.argtypes = [vp, vp, vp, C.c_uint64]
    L.chicdiff_hip_memcpy_d2h.argtypes = [vp, vp, vp, C.c_uint64]
    L.chicdiff_hip_count_table_dev.argtypes = [vp, vp, vp, vp, i64, vp, i32, vp, vp, C.POINTER(i64)]
    L.chicdiff_hip_chinput_read.argtypes = [vp, C.c_char_p, i32, C.POINTER(i64)]
    L.chicdiff_hip_chinput_table_dev.argtypes = [vp, vp, i32, vp, vp, C.POINTER(i64)]
    L.chicdiff_hip_chinput_parse_dev.argtypes = [vp, vp, i64, i32, i32, i32, vp, vp, vp, i64, C.POINTER(i64), C.POINTER(i64)]
    L.chicdiff_hip_chinput_read_dev.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
    L.chicdiff_hip_chinput_caps.argtypes = [C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.chicdiff_hip_peaks_parse_dev.argtypes = [vp, vp, i64, i32, C.POINTER(i32), i32, vp, vp, vp, vp, i64, C.POINTER(i64)]
    L.chicdiff_hip_peaks_read_dev.argtypes = [vp, C.c_char_p, C.POINTER(C.c_char_p), i32, C.POINTER(i32), C.POINTER(i64)]
    L.chicdiff_hip_peaks_columns_dev.argtypes = [vp, vp, vp, vp, vp, i64]
    L.chicdiff_hip_peaks_filter_dev.argtypes = [vp, vp, vp, vp, vp, i64, i32, dbl, C.POINTER(i32), i32, i32, i64, vp, vp, vp, vp,
                                                C.POINTER(i64), C.POINTER(i64)]
    L.chicdiff_hip_peaks_caps.argtypes = [C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.chicdiff_hip_selftest_peaks.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), i32, dbl, C.POINTER(i32), i32, i32, i64, vp, vp, vp, vp, vp, vp,
                                              C.POINTER(i32), C.POINTER(i64), C.c_char_p, i32]
    L.chicdiff_hip_peaks_textkeys_dev.argtypes = [vp, vp, vp, i64, C.POINTER(i64)]
    L.chicdiff_hip_peaks_merge_dev.argtypes = [vp, i32] + [C.POINTER(vp)] * 5 + [C.POINTER(i64), C.POINTER(i32), i64, vp, vp, vp, vp, vp, C.POINTER(i64)]
    L.chicdiff_hip_peaks_header.argtypes = [C.c_char_p, C.c_char_p, i32, C.POINTER(i32), C.POINTER(i32), C.c_char_p, i32]
    L.chicdiff_hip_selftest_peaks_textkeys.argtypes = [C.c_char_p, i64, vp, vp, C.POINTER(i64), C.c_char_p, i32]
    L.chicdiff_hip_bh_adjust_dev.argtypes = [vp, vp, i64, vp]
    L.chicdiff_hip_region_avdist_dev.argtypes = [vp, vp, vp, i64, vp, i64, i32, i32, vp, vp, vp]
    L.chicdiff_hip_count_join_inner_dev.argtypes = [vp, vp, vp, i64, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), vp]
    L.chicdiff_hip_count_join_multi_dev.argtypes = [vp, vp, vp, i64, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), vp]
    L.chicdiff_hip_count_tables_merge_dev.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), i64, vp, vp, C.POINTER(i64)]
    L.chicdiff_hip_region_assemble_dev.argtypes = [vp, vp, vp, i64, vp, i64, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), i32, i32,
                                                   vp, vp, vp, vp, vp, vp, i32, i32, C.POINTER(dbl), vp, vp]
    L.chicdiff_hip_ihw_apply_dev.argtypes = [vp, vp, vp, i64, C.POINTER(dbl), C.POINTER(dbl), i32, vp, vp, vp, vp]
    L.chicdiff_hip_ihw_train_dev.argtypes = [vp, vp, vp, i64, dbl, i32, i32, C.c_uint64, vp, vp, vp, C.POINTER(IhwInfo)]
    L.chicdiff_hip_ihw_caps.argtypes = [C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), i32, C.POINTER(i32)]
    L.chicdiff_hip_selftest_ihw_knots_dev.argtypes = [vp, vp, vp, i64, i32, i32, C.c_uint64, i32, i64, vp, vp, vp, C.POINTER(i32), C.POINTER(i64)]
    L.chicdiff_hip_selftest_ihw_orient.argtypes = [vp, vp, vp, vp, vp, vp, i64, vp]
    L.chicdiff_hip_region_universe_count_dev.argtypes = [vp, vp, vp, i64, i32, vp, i32, vp, vp, vp, C.POINTER(i64)]
    L.chicdiff_hip_region_universe_fill_dev.argtypes = [vp, vp, vp, i64, i32, vp, i32, vp, vp, vp, vp]
    L.chicdiff_hip_region_universe_dev.argtypes = [vp, vp, vp, i64, i32, vp, i32, vp, vp, vp, vp, vp, vp, i64, C.POINTER(i64)]
    L.chicdiff_hip_candidate_interactions_dev.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, vp, i64, i32, i32, i32, i32, dbl, dbl, dbl, i64,
                                                          vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64)]
    L.chicdiff_hip_candidate_interactions_method_dev.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, vp, i64, i32, i32, i32, i32, dbl, dbl, dbl, i32,
                                                                 i64, vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64)]
    L.chicdiff_hip_selftest_landau_dev.argtypes = [vp, vp, i64, vp]
    L.chicdiff_hip_chicago_tables_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp,
                                                  C.POINTER(i32)]
    L.chicdiff_hip_chicago_tables_caps.argtypes = [C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.chicdiff_hip_control_draws_dev.argtypes = [vp, vp, i64, vp, vp, vp, i64, vp, vp, i64, C.POINTER(i32), C.POINTER(i32), i32, C.c_uint64,
                                                 vp, vp, vp, C.POINTER(i64), C.POINTER(i64)]
    L.chicdiff_hip_countput_dev.argtypes = [vp, i32] + [C.POINTER(vp)] * 6 + [C.POINTER(i64), i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64)]
    L.chicdiff_hip_countput_caps.argtypes = [C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.chicdiff_hip_table_check.argtypes = [C.POINTER(TableColumn), i32, i64, i32, C.c_char_p, i32]
    L.chicdiff_hip_table_text_dev.argtypes = [vp, C.POINTER(TableColumn), i32, i64, i32, vp, i64, C.POINTER(i64)]
    L.chicdiff_hip_table_write_dev.argtypes = [vp, C.c_char_p, i32, C.c_char_p, i64, C.POINTER(TableColumn), i32, i64, i32, C.POINTER(i64)]
    L.chicdiff_hip_table_text_caps.argtypes = [C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.chicdiff_hip_selftest_format_double_dev.argtypes = [vp, vp, i64, vp, vp]
    L.chicdiff_hip_selftest_format_double.argtypes = [vp, i64, vp, vp]
    L.chicdiff_hip_nbglm_fit_dev.argtypes = [vp, vp, vp, i64, i32, C.POINTER(i32), C.POINTER(Opts), C.POINTER(Out),
                                             C.POINTER(Scalars)]
    L.chicdiff_hip_nbglm_fit.argtypes = L.chicdiff_hip_nbglm_fit_dev.argtypes
    L.chicdiff_hip_wald_test_dev.argtypes = [vp, vp, vp, i64, i32, C.POINTER(i32), dbl, C.POINTER(Opts), C.POINTER(Out),
                                             C.POINTER(Scalars), C.POINTER(dbl)]
    L.chicdiff_hip_theta_grid_dev.argtypes = [vp, vp, vp, C.POINTER(dbl), i64, i32, C.POINTER(dbl), i32,
                                              C.POINTER(Opts), C.POINTER(dbl)]
    L.chicdiff_hip_wald_pvalues_dev.argtypes = [vp, vp, i64, vp]
    L.chicdiff_hip_selftest_math_dev.argtypes = [vp, i32, vp, i64, vp]
    L.chicdiff_hip_selftest_math3_dev.argtypes = [vp, i32, vp, vp, i64, vp, vp]
    L.chicdiff_hip_selftest_objective_dev.argtypes = [vp, vp, vp, i64, i32, C.POINTER(i32), C.POINTER(Opts), vp, i32, vp, dbl, i32, vp, vp,
                                                      vp, vp, C.POINTER(i32)]
    L.chicdiff_hip_selftest_global_stage_dev.argtypes = [vp, vp, vp, vp, i64, i32, i32, C.POINTER(Opts), vp, vp, C.POINTER(dbl), C.POINTER(i32),
                                                         C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl), C.POINTER(Scalars)]
    L.chicdiff_hip_selftest_resid_hist_dev.argtypes = [vp, vp, i64, C.POINTER(dbl)]
    # the host forms of device rules (no context): what the CPU tests call directly
    u32, pd, pi = C.c_uint32, C.POINTER(dbl), C.POINTER(i32)
    L.chicdiff_hip_selftest_chinput.argtypes = [C.c_char_p, i32, i64, pi, pi, pi, C.POINTER(i64), C.c_char_p, i32]
    L.chicdiff_hip_selftest_r_random.argtypes = [i32, u32, dbl, dbl, i64, pd]
    L.chicdiff_hip_selftest_prior_mc.argtypes = [i32, vp, vp, vp]
    L.chicdiff_hip_selftest_sched_class.argtypes = [i32, dbl, pd, pd, i64, pi, pi]
    L.chicdiff_hip_selftest_queue_claim.argtypes = [C.c_uint64, i32, u32, u32, i32, i32, C.POINTER(u32), pi]
    L.chicdiff_hip_selftest_trend_exchange.argtypes = [i32, u32, i64, pd, C.POINTER(C.c_uint64), pi]
    L.chicdiff_hip_selftest_sf_bin.argtypes = [i32, pd, i64, pi, pi, i32, pi]
    L.chicdiff_hip_kernel_times.argtypes = [vp, C.POINTER(KernelTime), i32]
    L.chicdiff_hip_kernel_times.restype = i32
    L.chicdiff_hip_enable_timing.argtypes = [vp, i32]
    _lib = L
    return L


def default_opts(**kw) -> Opts:
    o = Opts()
    load_library().chicdiff_hip_default_opts(C.byref(o))
    for k, v in kw.items():
        if k == "trendCoef":
            o.trendCoef[0], o.trendCoef[1] = float(v[0]), float(v[1])
        else:
            setattr(o, k, v)
    return o


def chicago_tables_caps() -> dict:
    """The limits of ``HipContext.chicago_tables`` as the library was built (include/chicdiff_hip.h, CHICDIFF_CHICAGO_*): the most
    (tblb, tlb) pairs and distbin codes its LDS tables hold, and the consecutive rows a workgroup takes in each pass."""
    a, b, r = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    load_library().chicdiff_hip_chicago_tables_caps(C.byref(a), C.byref(b), C.byref(r))
    return dict(max_pairs=a.value, max_distbin=b.value, rows_per_workgroup=r.value)


def countput_caps() -> dict:
    """The limits of ``HipContext.countput`` as the library was built (include/chicdiff_hip.h, CHICDIFF_COUNTPUT_*): the most replicates
    of one condition, and the consecutive rows a workgroup takes in the key pass and in the heads / reduce passes."""
    m, k, r = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    load_library().chicdiff_hip_countput_caps(C.byref(m), C.byref(k), C.byref(r))
    return dict(max_rep=m.value, key_rows_per_workgroup=k.value, reduce_rows_per_workgroup=r.value)


def ihw_caps() -> dict:
    """The limits of ``HipContext.ihw_train`` as the library was built (include/chicdiff_hip.h, CHICDIFF_IHW_*): the most groups and
    folds, the largest automatic number of groups, and the chunk lengths it accepts (ascending; the last is the default)."""
    a, b, c, k = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    lens = (C.c_int32 * 16)()
    load_library().chicdiff_hip_ihw_caps(C.byref(a), C.byref(b), C.byref(c), lens, 16, C.byref(k))
    return dict(max_bins=a.value, max_folds=b.value, auto_max_bins=c.value, chunk_lens=[lens[i] for i in range(min(k.value, 16))])


def selftest_ihw_orient(ax, ac, bx, bc, cx, cc):
    """The exact knot test of the IHW training stage as compiled for the host (chicdiff_hip_selftest_ihw_orient): the sign, per triple
    of points (x, count), of (b.c - a.c) (c.x - a.x) - (c.c - a.c) (b.x - a.x).  No GPU is needed."""
    xs = [np.ascontiguousarray(v, dtype=np.float64) for v in (ax, bx, cx)]
    cs = [np.ascontiguousarray(v, dtype=np.int32) for v in (ac, bc, cc)]
    n = len(xs[0])
    if any(v.shape != (n,) for v in xs + cs):
        raise ValueError(f"selftest_ihw_orient: six vectors of one length are required, got shapes {[v.shape for v in xs + cs]}")
    out = np.empty(n, dtype=np.int32)
    rc = load_library().chicdiff_hip_selftest_ihw_orient(xs[0].ctypes.data, cs[0].ctypes.data, xs[1].ctypes.data, cs[1].ctypes.data,
                                                         xs[2].ctypes.data, cs[2].ctypes.data, n, out.ctypes.data)
    if rc:
        raise ChicdiffHipError(f"[{rc}] selftest_ihw_orient: bad arguments")
    return out


# include/chicdiff_hip.h, CHICDIFF_COL_* / CHICDIFF_TABLE_*
COL_INT32, COL_INT64, COL_FLOAT64, COL_DICT = 0, 1, 2, 3
TABLE_MAX_CELL_BYTES = 24


def table_text_caps() -> dict:
    """The limits of ``HipContext.table_text`` / ``write_table`` as the library was built (include/chicdiff_hip.h, CHICDIFF_TABLE_*): the
    rows a workgroup takes, the bytes of text it stages in LDS at a time, the most columns and the most entries of a dictionary."""
    r, b, c, d = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    load_library().chicdiff_hip_table_text_caps(C.byref(r), C.byref(b), C.byref(c), C.byref(d))
    return dict(rows_per_tile=r.value, lds_bytes=b.value, max_columns=c.value, max_dict=d.value)


def _format_double_cells(text, length):
    return [text[i, :k].tobytes() for i, k in enumerate(length.tolist())]


def selftest_format_double(x):
    """The library's double -> text function compiled for the HOST (chicdiff_hip_selftest_format_double: no device, no context) on
    an array of float64: the list of the cells as bytes — repr(float), nothing for NaN."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    text, length = np.zeros((len(x), TABLE_MAX_CELL_BYTES), dtype=np.uint8), np.zeros(len(x), dtype=np.int32)
    rc = load_library().chicdiff_hip_selftest_format_double(x.ctypes.data, len(x), text.ctypes.data, length.ctypes.data)
    if rc:
        raise ValueError(f"selftest_format_double: error {rc}")
    return _format_double_cells(text, length)


def table_columns(columns, n=None, device=None):
    """The column descriptors of ``HipContext.table_text`` / ``write_table`` from ``columns``: a one-dimensional contiguous int32,
    int64 or float64 tensor is a column of that kind; a pair ``(codes, entries)`` is a dictionary column — ``codes`` an int32 tensor
    or None (entry 0 for every row), ``entries`` a sequence of bytes or str.  ``n``: the number of rows, needed where no column is a
    tensor.  ``device``: where every tensor must live (None: not checked).  Returns (array of TableColumn, n, what the array points
    into — to be kept alive for the call).  Anything else raises ValueError; the rule's own refusals are the library's."""
    import torch
    kinds = {torch.int32: COL_INT32, torch.int64: COL_INT64, torch.float64: COL_FLOAT64}
    columns = list(columns)
    arr = (TableColumn * max(len(columns), 1))()
    keep = []

    def tensor(name, t, dtypes):
        nonlocal n
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: a torch tensor is required, got {type(t).__name__}")
        if t.dtype not in dtypes:
            raise ValueError(f"{name}: dtype {' / '.join(str(d) for d in dtypes)} is required, got {t.dtype}")
        if device is not None and t.device != device:
            raise ValueError(f"{name}: must be on {device}, is on {t.device}")
        if t.dim() != 1:
            raise ValueError(f"{name}: a one-dimensional tensor is required, got shape {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: must be contiguous")
        if n is None:
            n = t.numel()
        if t.numel() != n:
            raise ValueError(f"{name}: {n} rows are required, got {t.numel()}")
        keep.append(t)
        return t.data_ptr() if t.numel() else None

    for j, col in enumerate(columns):
        if isinstance(col, (tuple, list)):
            if len(col) != 2:
                raise ValueError(f"columns[{j}]: a dictionary column is (codes, entries)")
            codes, entries = col
            ent = [e.encode() if isinstance(e, str) else bytes(e) for e in entries]
            off = np.zeros(len(ent) + 1, dtype=np.int32)
            off[1:] = np.cumsum([len(e) for e in ent], dtype=np.int64).astype(np.int32) if ent else 0
            blob = np.frombuffer(b"".join(ent) + b"\0", dtype=np.uint8).copy()
            keep += [off, blob]
            arr[j].kind, arr[j].ndict = COL_DICT, len(ent)
            arr[j].d_data = None if codes is None else tensor(f"columns[{j}] codes", codes, (torch.int32,))
            arr[j].dict_off, arr[j].dict_bytes = off.ctypes.data, blob.ctypes.data
        else:
            ptr = tensor(f"columns[{j}]", col, tuple(kinds))
            arr[j].kind, arr[j].d_data = kinds[col.dtype], ptr
    if n is None:
        raise ValueError("table: the number of rows is required where no column is a tensor")
    return arr, int(n), keep


def _sep_byte(sep):
    b = sep.encode() if isinstance(sep, str) else bytes(sep)
    if len(b) != 1:
        raise ValueError(f"table: the separator is one byte, got {sep!r}")
    return b[0]


def table_check(columns, sep=",", n=None):
    """The refusals of the table rule on their own (chicdiff_hip_table_check: host only, no context, the tensors are not read): raises
    ValueError with the library's message."""
    arr, n, keep = table_columns(columns, n=n)
    err = C.create_string_buffer(512)
    if load_library().chicdiff_hip_table_check(arr, len(list(columns)), n, _sep_byte(sep), err, 512):
        raise ValueError(err.value.decode())


def chinput_caps() -> dict:
    """The limits of the device path of ``HipContext.read_chinput`` / ``parse_chinput_text`` as the library was built
    (include/chicdiff_hip.h, CHICDIFF_CHINPUT_*): the body bytes a workgroup takes, the bytes of it one lane marks, and the bytes staged
    in LDS per tile (the tile and its overhang)."""
    t, l, w = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    load_library().chicdiff_hip_chinput_caps(C.byref(t), C.byref(l), C.byref(w))
    return dict(tile_bytes=t.value, lane_bytes=l.value, window_bytes=w.value)


# include/chicdiff_hip.h, CHICDIFF_PEAKS_*
PEAKS_ST_QUOTE, PEAKS_ST_SLOW_OVERFLOW = 1, 2
PEAKS_INFO = ("nrows", "status", "maxbait", "nslow", "bad", "body", "sep", "nscore", "nkept", "nfiltered")
PEAKS_INT_COLUMNS = ("baitStart", "baitEnd", "baitID", "oeStart", "oeEnd", "oeID")


def peaks_caps() -> dict:
    """The limits of ``HipContext.read_peaks`` / ``parse_peaks_text`` as the library was built (include/chicdiff_hip.h): the tile and
    the staged window (chinput's), the most score columns, and the entries of the slow-token list."""
    t, w, m, sl = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    load_library().chicdiff_hip_peaks_caps(C.byref(t), C.byref(w), C.byref(m), C.byref(sl))
    return dict(tile_bytes=t.value, window_bytes=w.value, max_scores=m.value, max_slow=sl.value)


def _c_strings(names):
    arr = (C.c_char_p * max(len(names), 1))()
    for k, v in enumerate(names):
        arr[k] = str(v).encode()
    return arr


def selftest_peaks(path, targetColumns, score=5.0, cond_of_target=None, replicate_rule=False):
    """The library's HOST statement of the peak-matrix rule (chicdiff_hip_selftest_peaks: no device, no context) on a file: a dict
    with ``info`` (PEAKS_INFO), the columns of all rows (``ints`` (6, n), ``dist``, ``scores`` (nscore, n), ``line_off``),
    ``score_target``, ``kept_idx`` and ``filtered``.  A header or malformed-row error raises ValueError with the library's message
    (``.offset``: the body offset of a malformed row, else None)."""
    lib = load_library()
    targets = list(targetColumns)
    T = len(targets)
    cond = np.zeros(max(T, 1), dtype=np.int32)
    if cond_of_target is not None:
        cond[:T] = np.asarray(cond_of_target, dtype=np.int32)
    ncond = int(cond[:T].max()) + 1 if T else 0
    names = _c_strings(targets)
    info = (C.c_int64 * len(PEAKS_INFO))()
    err = C.create_string_buffer(512)
    st = np.zeros(max(T, 1), dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))

    def call(cap, ints, dist, scores, line_off, kept, filt):
        ptr = lambda a: a.ctypes.data if a is not None else None
        rc = lib.chicdiff_hip_selftest_peaks(os.fsencode(path), names, T, float(score), ip(cond), ncond, int(bool(replicate_rule)), cap, ptr(ints),
                                             ptr(dist), ptr(scores), ptr(line_off), ptr(kept), ptr(filt), ip(st), info, err, 512)
        if rc:
            e = ValueError(err.value.decode() or f"selftest_peaks: error {rc}")
            e.offset = info[4] if info[4] >= 0 else None
            raise e
    call(0, None, None, None, None, None, None)
    d = dict(zip(PEAKS_INFO, info))
    n, ns = d["nrows"], d["nscore"]
    if d["status"]:
        return dict(info=d)
    ints, dist = np.zeros((6, n), dtype=np.int32), np.zeros(n)
    scores, line_off = np.zeros((ns, n)), np.zeros(n, dtype=np.int64)
    kept, filt = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    if n:
        call(n, ints, dist, scores, line_off, kept, filt)
    d = dict(zip(PEAKS_INFO, info))
    return dict(info=d, ints=ints, dist=dist, scores=scores, line_off=line_off, score_target=st[:ns].copy(), kept_idx=kept[:d["nkept"]],
                filtered=filt[:d["nfiltered"]])


# .multimerge on the device (include/chicdiff_hip.h, above chicdiff_hip_peaks_textkeys_dev)
PEAKS_MERGE_MAX_FILES = 16
PEAKS_ST_CHR_LONG, PEAKS_ST_CHR_AMBIGUOUS, PEAKS_ST_MERGE_DUPLICATE, PEAKS_ST_MERGE_NAME, PEAKS_ST_MERGE_DIST = 4, 8, 16, 32, 64
PEAKS_KEY_INT, PEAKS_KEY_TEXT, PEAKS_KEY_MIXED = 0, 1, 2


def peaks_header(path):
    """The column names of a peak matrix and its separator byte, through the header rule of ``HipContext.read_peaks``
    (chicdiff_hip_peaks_header: host only).  A header the rule refuses raises ValueError with the library's message."""
    lib = load_library()
    cap = 1 << 16
    while True:
        names, err = C.create_string_buffer(cap), C.create_string_buffer(512)
        ncols, sep = C.c_int32(0), C.c_int32(0)
        rc = lib.chicdiff_hip_peaks_header(os.fsencode(path), names, cap, C.byref(ncols), C.byref(sep), err, 512)
        if rc and err.value.startswith(b"peaks_header: the names take") and cap < (1 << 28):
            cap *= 16
            continue
        if rc:
            raise ValueError(err.value.decode() or f"peaks_header: error {rc}")
        return names.value.decode().split("\n"), sep.value


def selftest_peaks_textkeys(path):
    """The library's HOST statement of the text-key rule (chicdiff_hip_selftest_peaks_textkeys: no device, no context) on a file: a dict
    with ``status`` (PEAKS_ST_CHR_* bits), ``key_class`` (baitChr, oeChr), ``chr_keys`` (2, n) and ``name_hash`` (2, n) int64."""
    lib = load_library()
    info, err = (C.c_int64 * 4)(), C.create_string_buffer(512)

    def call(cap, chr_, name):
        rc = lib.chicdiff_hip_selftest_peaks_textkeys(os.fsencode(path), cap, chr_.ctypes.data if chr_ is not None else None,
                                                      name.ctypes.data if name is not None else None, info, err, 512)
        if rc:
            raise ValueError(err.value.decode() or f"selftest_peaks_textkeys: error {rc}")
    call(0, None, None)
    n = info[3]
    chr_, name = np.zeros((2, n), dtype=np.int64), np.zeros((2, n), dtype=np.int64)
    if n and not info[0]:
        call(n, chr_, name)
    return dict(status=info[0], key_class=(info[1], info[2]), chr_keys=chr_, name_hash=name, nrows=n)


class Peaks:
    """A peak matrix on the device (``HipContext.read_peaks`` / ``parse_peaks_text``): ``ints`` (6, n) int32 — PEAKS_INT_COLUMNS, also
    as attributes —, ``dist`` (n) and ``scores`` (nscore, n) float64, ``line_off`` (n) int64: the offset of every row's line in the body;
    ``info``: the words of PEAKS_INFO; ``score_names``: the score rows' column names (file order).  ``status`` != 0 (PEAKS_ST_*): the
    device did not parse this body and no column is held.  After ``read_peaks(text_keys=True)`` also ``chr_keys`` (2, n) int64 — the
    sort keys of baitChr and oeChr —, ``name_hash`` (2, n) int64 — baitName, oeName —, ``key_class`` (PEAKS_KEY_* of the two
    chromosome columns) and ``key_status`` (PEAKS_ST_CHR_* bits).  After ``merge_peaks`` also ``src_file`` (int32) and ``src_row``
    (int64): the file (an index into ``paths``) and the row there that every merged row's key columns come from; ``line_off`` is then
    that row's offset in ITS file's body; ``bodies`` / ``seps``: per file."""

    chr_keys = name_hash = key_class = key_status = src_file = src_row = paths = bodies = seps = None

    def __init__(self, info, ints=None, dist=None, scores=None, line_off=None, score_names=None, path=None):
        self.info, self.ints, self.dist, self.scores, self.line_off = info, ints, dist, scores, line_off
        self.score_names, self.path = score_names, path
        self.n, self.nscore, self.status, self.maxbait = info["nrows"], info["nscore"], info["status"], info["maxbait"]
        if ints is not None:
            for k, name in enumerate(PEAKS_INT_COLUMNS):
                setattr(self, name, ints[k])


def _contiguous(t):
    """A column of a ``Peaks`` laid out for the C ABI (anything but a tensor goes on as it is, to the marshalling layer's refusal)."""
    return t.contiguous() if hasattr(t, "contiguous") else t


def _scalars_dict(s: Scalars) -> dict:
    return dict(trendCoef=np.array(s.trendCoef[:]), varLogDispEsts=s.varLogDispEsts, dispPriorVar=s.dispPriorVar,
                sumDeviance=s.sumDeviance, nAllZero=s.nAllZero, trendOuterIter=s.trendOuterIter, status=s.status)


class HipContext:
    """One context per process/GPU.  Device buffers are torch tensors on ``cuda:<device>``
    (torch's name for a ROCm device), laid out sample-major: a tensor of shape (S, n),
    contiguous, is the C ABI's column-major n x S matrix."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        import torch

        self.torch = torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise ChicdiffHipError("no MI355X visible to PyTorch-ROCm: the HIP path cannot run (there is no CPU fallback)")
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        rc = self.lib.chicdiff_hip_create(C.byref(h), device)
        if rc:
            raise ChicdiffHipError(self.lib.chicdiff_hip_last_error(None).decode())
        self.h = h
        self._cb = None
        self._comm_tensors = {}
        if use_torch_stream:
            self.use_stream(torch.cuda.current_stream(self.device))

    # -- plumbing ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.chicdiff_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise ChicdiffHipError(f"[{rc}] " + self.lib.chicdiff_hip_last_error(self.h).decode())

    def use_stream(self, stream):
        self._check(self.lib.chicdiff_hip_set_stream(self.h, C.c_void_p(stream.cuda_stream)))

    def set_option(self, name: str, value: int):
        """Tuning / test options: every name and range is listed above chicdiff_hip_set_option in include/chicdiff_hip.h; an
        unknown name or a value outside its range raises ChicdiffHipError.

        Most options are bit-neutral.  These select another summation order and so move results at the 1e-13 level (a row in
        about 1e5 then stops its line search a step apart): ``trend_one_launch_per_pass`` and
        ``sharded_trend_gather`` (the trend's sums over another partition of the rows), ``theta_grid_concurrency`` (with more than
        one fit in flight the fits of a theta grid run the trend as one launch per pass; one fit in flight, or a one-point grid,
        is the default single fit by bits, and any two settings above 1 agree by bits), ``trend_persistent_blocks`` (the
        partition of the single-launch trend kernel) and ``wald_final_row_constant`` (``deviance`` and ``sumDeviance`` only).
        ``trend_mad_in_kernel = 0`` keeps the trend's bits and was found bit-identical in ``varLogDispEsts`` and the prior
        variance as well (tests/test_gpu_theta_scan.py).  ``local_trend_substitute`` changes the outcome of a fit whose
        parametric trend fails, as DESeq2's fitType does."""
        self._check(self.lib.chicdiff_hip_set_option(self.h, name.encode(), int(value)))

    def enable_timing(self, on=True):
        self.lib.chicdiff_hip_enable_timing(self.h, int(on))

    def kernel_times(self) -> dict:
        buf = (KernelTime * 32)()
        k = self.lib.chicdiff_hip_kernel_times(self.h, buf, 32)
        return {buf[i].name.decode(): (buf[i].ms, buf[i].launches) for i in range(min(k, 32))}

    def collective_stats(self) -> dict:
        """Collectives of the last call (timing mode 1): {"allreduce" / "allgather": (count, ms on the stream, bytes handed over)}."""
        buf = (KernelTime * 32)()
        k = self.lib.chicdiff_hip_kernel_times(self.h, buf, 32)
        return {buf[i].name.decode(): (buf[i].launches, buf[i].ms, buf[i].bytes) for i in range(min(k, 32))
                if buf[i].name in (b"allreduce", b"allgather")}

    def last_refits(self) -> int:
        """Refits the last call went through (select overflow / barrier timeout / local substitute); the same on every rank."""
        return int(self.lib.chicdiff_hip_last_refits(self.h))

    def set_process_group(self, group=None, memory="device", allgather=True):
        """Route the library's collectives through torch.distributed (backend nccl = RCCL): the sum-all-reduce hook and,
        unless ``allgather`` is False, the all-gather hook for the rows of the dispersion trend."""
        from .dist import AllReduceHook

        self._hook = AllReduceHook(group, memory=memory, device=self.device)
        self._sharded = True  # (from here on the context's fits are pieces of a sharded fit: dist.theta_grid_replicas refuses it)
        self._check(self.lib.chicdiff_hip_set_allreduce(self.h, self._hook.fn, None, self._hook.world, self._hook.rank))
        if allgather:
            self._check(self.lib.chicdiff_hip_set_allgather(self.h, self._hook.gather_fn, None))

    def init_rccl(self, group=None, librccl_path=None):
        """Direct RCCL: the library makes its own communicator over the ranks of ``group`` and issues
        ncclAllReduce itself (no Python callback per collective).  torch.distributed only carries the
        128-byte unique id.  Uses the librccl torch itself loaded unless ``librccl_path`` says otherwise."""
        import os

        import torch.distributed as dist

        torch = self.torch
        if librccl_path is None:
            cand = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
            librccl_path = cand if os.path.exists(cand) else "librccl.so"
        path = librccl_path.encode()
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        dev = self.device if dist.get_backend(group) == "nccl" else "cpu"

        def all_ok(ok: bool) -> bool:  # every rank must take the same branch, or the collectives that follow hang
            flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
            return bool(flag.item())

        # phase 1, local: can this rank open librccl at all?  (every rank makes an id; only rank 0's is used)
        ident = (C.c_char * 128)()
        rc = self.lib.chicdiff_hip_rccl_unique_id(self.h, path, ident)
        msg = self.lib.chicdiff_hip_last_error(self.h).decode() if rc else ""
        if not all_ok(rc == 0):
            raise ChicdiffHipError(f"librccl not usable on every rank ({msg or 'another rank failed'})")
        # phase 2, collective: share rank 0's id, create the communicator
        box = [bytes(ident.raw)]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        buf = (C.c_char * 128).from_buffer_copy(box[0])
        rc = self.lib.chicdiff_hip_rccl_init(self.h, path, buf, world, rank)
        msg = self.lib.chicdiff_hip_last_error(self.h).decode() if rc else ""
        if not all_ok(rc == 0):
            self.lib.chicdiff_hip_set_allreduce(self.h, C.cast(None, ALLREDUCE_FN), None, 1, 0)
            raise ChicdiffHipError(f"ncclCommInitRank did not succeed on every rank ({msg or 'another rank failed'})")
        self._hook = None
        self._sharded = True

    def to_device(self, a, dtype):
        """(n, S) host array -> (S, n) contiguous device tensor (sample-major)."""
        t = self.torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=dtype).T))
        return t.to(self.device)

    # -- marshalling: the one way a caller's object reaches the C ABI -------------------------------------
    # (One exception, kept as it was: the columns of ``table_text`` / ``write_table`` go through ``table_columns`` above.  Its rule is
    # another one — a column may have one of three dtypes, all columns share a row count — it also serves ``table_check``, which has no
    # context or device, and the tests hold its messages word for word.)
    def _check_tensor(self, name, t, dtype, shape=None):
        """ValueError unless ``t`` is a contiguous tensor of ``dtype`` on this context's device (and of ``shape``, -1 = any)."""
        torch = self.torch
        if isinstance(t, torch.Tensor) and t.dtype is dtype and t.device == self.device and t.is_contiguous() and (shape is None or t.shape == shape):
            return                                                     # (the whole rule at once; below, which part of it failed)
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: a torch tensor is required, got {type(t).__name__}")
        if t.dtype != dtype:
            raise ValueError(f"{name}: dtype {dtype} is required, got {t.dtype}")
        if t.device != self.device:
            raise ValueError(f"{name}: must be on {self.device}, is on {t.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: must be contiguous")
        if shape is not None and (t.dim() != len(shape) or any(w != -1 and w != g for w, g in zip(shape, t.shape))):
            raise ValueError(f"{name}: shape {tuple(shape)} is required (-1 = any), got {tuple(t.shape)}")

    def _ptr(self, name, t, dtype, shape=None):
        """``_check_tensor``, then the tensor's device address."""
        self._check_tensor(name, t, dtype, shape)
        return t.data_ptr()

    def _ptr_or_none(self, name, t, dtype, shape=None):
        """``_ptr``; None stays None, the C ABI's NULL for an argument left out."""
        return None if t is None else self._ptr(name, t, dtype, shape)

    def _tables(self, who, tables):
        """``tables`` = [(keys, vals)] per replicate, int64 / int32 device vectors of one length each, 1 <= S <= 64 of them ->
        (S, keys' addresses, vals' addresses, lengths) as the C ABI takes them."""
        torch = self.torch
        try:
            S = len(tables)
        except TypeError:
            raise ValueError(f"{who}: tables must be a sequence of (keys, vals) pairs") from None
        if not 1 <= S <= 64:
            raise ValueError(f"{who}: 1 <= S <= 64 replicates are supported, got {S}")
        kp, vp, nk = (C.c_void_p * S)(), (C.c_void_p * S)(), (C.c_int64 * S)()
        for s, kv in enumerate(tables):
            if not isinstance(kv, (tuple, list)) or len(kv) != 2:
                raise ValueError(f"tables[{s}]: a (keys, vals) pair is required")
            kp[s] = self._ptr(f"tables[{s}] keys", kv[0], torch.int64, (-1,))
            vp[s] = self._ptr(f"tables[{s}] vals", kv[1], torch.int32, (-1,))
            nk[s] = kv[0].numel()
            if kv[0].numel() != kv[1].numel():
                raise ValueError(f"tables[{s}]: {kv[0].numel()} keys but {kv[1].numel()} vals")
        return S, kp, vp, nk

    def _matrices(self, name, d_counts, d_other):
        """The counts, int32 (S, n), and the float64 matrix ``name`` of the same shape beside them -> (their addresses, S, n)."""
        pk = self._ptr("d_counts", d_counts, self.torch.int32, (-1, -1))
        S, n = d_counts.shape
        return pk, self._ptr(name, d_other, self.torch.float64, (S, n)), S, n

    @staticmethod
    def _group(group, S):
        """The condition code of every sample, S integers -> int32[S]."""
        g = np.asarray(group)
        if g.dtype.kind not in "iu" or g.ndim != 1:
            raise ValueError(f"group: a sequence of {S} integers is required, got {group!r}")
        if len(g) != S:
            raise ValueError(f"group: one entry per sample ({S}) is required, got {len(g)}")
        return (C.c_int32 * S)(*g.tolist())

    def _outputs(self, want, default, n, outputs=None, host=False):
        """The columns asked for -> (Out, {name: buffer of n entries}).  ``outputs``: the caller's device buffers by name, used where
        present; ``host``: numpy buffers instead of device tensors (always fresh)."""
        torch = self.torch
        out, bufs, shape = Out(), ({} if outputs is None else outputs), (n,)
        for k in (default if want is None else want):
            column = _OUT_COLUMNS.get(k)
            if column is None:
                raise ValueError(f"want: unknown column {k!r}; the columns are {OUT_DOUBLE + OUT_INT}")
            name, double = column
            if host:
                bufs[k] = np.empty(n, dtype=np.float64 if double else np.int32)
                setattr(out, k, bufs[k].ctypes.data)
                continue
            dtype = torch.float64 if double else torch.int32
            if k not in bufs:
                bufs[k] = torch.empty(n, dtype=dtype, device=self.device)
            setattr(out, k, self._ptr(name, bufs[k], dtype, shape))
        return out, bufs

    @staticmethod
    def _opts(opts):
        """``Opts`` or None (the library's defaults) -> what the C ABI takes for ``const chicdiff_nbglm_opts *``."""
        if opts is None:
            return None
        if not isinstance(opts, Opts):
            raise ValueError(f"opts: an Opts (hip.default_opts(...)) or None is required, got {type(opts).__name__}")
        return C.byref(opts)

    @staticmethod
    def _seed(who, seed):
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
            raise ValueError(f"{who}: seed must be an integer in [0, 2^64), got {seed!r}")
        return int(seed)

    @staticmethod
    def _host(name, a, dtype, shape):
        """A host vector or matrix -> (contiguous numpy array of ``dtype`` and ``shape``, -1 = any; its address as the C ABI's typed
        pointer).  The array is to be kept alive for the call."""
        try:
            a = np.ascontiguousarray(a, dtype=dtype)
        except (TypeError, ValueError):
            raise ValueError(f"{name}: numbers convertible to {np.dtype(dtype).name} are required, got {type(a).__name__}") from None
        if a.ndim != len(shape) or any(w != -1 and w != g for w, g in zip(shape, a.shape)):
            raise ValueError(f"{name}: shape {tuple(shape)} is required{' (-1 = any)' if -1 in shape else ''}, got {a.shape}")
        return a, a.ctypes.data_as(C.POINTER(C.c_double if dtype is np.float64 else C.c_int32))

    # -- a5 ---------------------------------------------------------------------------------
    def size_factors(self, d_counts) -> np.ndarray:
        dc = self._ptr("d_counts", d_counts, self.torch.int32, (-1, -1))
        S, n = d_counts.shape
        sf = (C.c_double * S)()
        self._check(self.lib.chicdiff_hip_size_factors_dev(self.h, dc, n, S, sf))
        return np.array(sf[:])

    # -- a4 ---------------------------------------------------------------------------------
    def offsets(self, d_fullmean, size_factors, theta=None, out=None):
        torch = self.torch
        dfm = self._ptr("d_fullmean", d_fullmean, torch.float64, (-1, -1))
        S, n = d_fullmean.shape
        sf, psf = self._host("size_factors", size_factors, np.float64, (S,))
        if out is None:
            out = torch.empty_like(d_fullmean)
        pout = self._ptr("out", out, torch.float64, (S, n))
        th = float("nan") if theta is None else float(theta)
        self._check(self.lib.chicdiff_hip_offsets_dev(self.h, dfm, psf, n, S, th, pout))
        return out

    # -- a2 ---------------------------------------------------------------------------------
    def window_sums(self, d_fragN, d_fragFM, d_region_ptr):
        torch = self.torch
        if d_fragN is not None:
            self._check_tensor("d_fragN", d_fragN, torch.int32, (-1, -1))
            S, nfrag = d_fragN.shape
        else:
            self._check_tensor("d_fragFM", d_fragFM, torch.float64, (-1, -1))
            S, nfrag = d_fragFM.shape
        pN = self._ptr_or_none("d_fragN", d_fragN, torch.int32, (S, nfrag))
        pFM = self._ptr_or_none("d_fragFM", d_fragFM, torch.float64, (S, nfrag))
        ptr = self._ptr("d_region_ptr", d_region_ptr, torch.int64, (-1,))
        n = d_region_ptr.numel() - 1
        N = torch.empty((S, n), dtype=torch.int32, device=self.device) if d_fragN is not None else None
        FM = torch.empty((S, n), dtype=torch.float64, device=self.device) if d_fragFM is not None else None
        self._check(self.lib.chicdiff_hip_window_sums_dev(self.h, pN, pFM, nfrag, S, ptr, n, N.data_ptr() if N is not None else None,
                                                          FM.data_ptr() if FM is not None else None))
        return N, FM

    # -- a1 ---------------------------------------------------------------------------------
    def count_join(self, d_bait, d_oe, d_keys, d_vals):
        torch = self.torch
        pb = self._ptr("d_bait", d_bait, torch.int32, (-1,))
        nru = d_bait.numel()
        po = self._ptr("d_oe", d_oe, torch.int32, (nru,))
        pk = self._ptr("d_keys", d_keys, torch.int64, (-1,))
        pv = self._ptr("d_vals", d_vals, torch.int32, (d_keys.numel(),))
        out = torch.empty_like(d_bait)
        self._check(self.lib.chicdiff_hip_count_join_dev(self.h, pb, po, nru, pk, pv, d_keys.numel(), out.data_ptr()))
        return out

    def count_join_multi(self, d_bait, d_oe, tables, out=None):
        """The chinput branch for all replicates at once (chicdiff.R:843-858, the loop over the replicates): ``tables`` =
        [(keys, vals)] per replicate; N (S, nru), row s = ``count_join`` with table s, from ONE read of the RU rows."""
        torch = self.torch
        S, kp, vp, nk = self._tables("count_join_multi", tables)
        pb = self._ptr("d_bait", d_bait, torch.int32, (-1,))
        nru = d_bait.numel()
        po = self._ptr("d_oe", d_oe, torch.int32, (nru,))
        if out is None:
            out = torch.empty((S, nru), dtype=torch.int32, device=self.device)
        pout = self._ptr("out", out, torch.int32, (S, nru))
        self._check(self.lib.chicdiff_hip_count_join_multi_dev(self.h, pb, po, nru, S, kp, vp, nk, pout))
        return out

    def region_assemble(self, d_bait, d_oe, d_region_ptr, tables, id_min, d_midsum, d_sj, d_si, d_tblb, d_tlb, d_T, distfun,
                        want_N=True, want_FullMean=True):
        """Region-level N and FullMean (S, n) of the chinput branch in one kernel (chicdiff.R:843-858, 628-703, 894-896, 1540-1547):
        bit for bit ``count_join_multi`` -> ``fragment_background(only_fullmean=True)`` -> ``window_sums`` on the same tensors, without
        the two (S, nru) matrices in between.  ``tables`` = [(keys, vals)] per replicate; the other arguments as those three take
        them.  Returns (N, FullMean); the one not wanted is None and its inputs are not read."""
        torch = self.torch
        if not (want_N or want_FullMean):
            raise ValueError("region_assemble: neither N nor FullMean is wanted")
        S, kp, vp, nk = self._tables("region_assemble", tables)
        pb = self._ptr("d_bait", d_bait, torch.int32, (-1,))
        nru = d_bait.numel()
        po = self._ptr("d_oe", d_oe, torch.int32, (nru,))
        ptr = self._ptr("d_region_ptr", d_region_ptr, torch.int64, (-1,))
        n = d_region_ptr.numel() - 1
        if n < 1:
            raise ValueError("region_assemble: region_ptr must hold at least one region (two entries)")
        nid, pm, tabs, _df = self._background(S, d_midsum, d_sj, d_si, d_tblb, d_tlb, d_T, distfun)
        N = torch.empty((S, n), dtype=torch.int32, device=self.device) if want_N else None
        FM = torch.empty((S, n), dtype=torch.float64, device=self.device) if want_FullMean else None
        self._check(self.lib.chicdiff_hip_region_assemble_dev(
            self.h, pb, po, nru, ptr, n, S, kp, vp, nk, int(id_min), nid, pm, *tabs,
            N.data_ptr() if want_N else None, FM.data_ptr() if want_FullMean else None))
        return N, FM

    def _background(self, S, d_midsum, d_sj, d_si, d_tblb, d_tlb, d_T, distfun):
        """The Chicago background tables of S replicates as ``region_assemble`` and ``fragment_background`` take them -> (nid, d_midsum's
        address, the C ABI's eight arguments from d_sj to distfun_host, which follow one another in both entry points, and the
        distfun array those point into, to be kept alive for the call)."""
        torch = self.torch
        pm = self._ptr("d_midsum", d_midsum, torch.int64, (-1,))
        nid = d_midsum.numel()
        if nid < 1:
            raise ValueError("d_midsum: empty restriction map")
        psj = self._ptr("d_sj", d_sj, torch.float64, (S, nid))
        psi = self._ptr("d_si", d_si, torch.float64, (S, nid))
        ptb = self._ptr("d_tblb", d_tblb, torch.int32, (S, nid))
        ptl = self._ptr("d_tlb", d_tlb, torch.int32, (S, nid))
        pT = self._ptr("d_T", d_T, torch.float64, (S, -1, -1))
        if d_T.shape[1] < 1 or d_T.shape[2] < 1:
            raise ValueError(f"d_T: shape (S, ntblb >= 1, ntlb >= 1) is required, got {tuple(d_T.shape)}")
        df, pdf = self._host("distfun", distfun, np.float64, (S, 10))
        return nid, pm, (psj, psi, ptb, ptl, pT, d_T.shape[1], d_T.shape[2], pdf), df

    def count_join_inner(self, d_bait, d_oe, tables):
        """No-chinput branch (chicdiff.R:774-807): ``tables`` = [(keys, vals)] per replicate (device tensors as
        ``count_table`` returns them); N (S, nru) with the reference's Reduce(merge) semantics — a pair keeps its
        counts only when every replicate's table holds it."""
        torch = self.torch
        S, kp, vp, nk = self._tables("count_join_inner", tables)
        pb = self._ptr("d_bait", d_bait, torch.int32, (-1,))
        nru = d_bait.numel()
        po = self._ptr("d_oe", d_oe, torch.int32, (nru,))
        out = torch.empty((S, nru), dtype=torch.int32, device=self.device)
        self._check(self.lib.chicdiff_hip_count_join_inner_dev(self.h, pb, po, nru, S, kp, vp, nk, out.data_ptr()))
        return out

    def merge_count_tables(self, count_tables):
        """No-chinput branch, the merge alone (chicdiff.R:778, the Reduce(merge) of :774-807): ``count_tables`` = [(keys, vals)] per replicate as
        ``count_table`` returns them -> [(keys, vals_s)] per replicate, the pairs that EVERY table holds (key equality: N = 0 is a count)
        with each replicate's counts.  One keys tensor is shared by all replicates; the values are the rows of one (S, cap) tensor cut
        to the merged length, so every ``vals_s`` is contiguous.  ``count_join_multi`` / ``region_assemble`` on the result equal
        ``count_join_inner`` (-> ``fragment_background`` -> ``window_sums``) on ``count_tables`` bit for bit."""
        torch = self.torch
        S, kp, vp, nk = self._tables("merge_count_tables", count_tables)
        cap = min(nk)
        keys = torch.empty(cap, dtype=torch.int64, device=self.device)
        vals = torch.empty((S, cap), dtype=torch.int32, device=self.device)
        n = C.c_int64(0)
        self._check(self.lib.chicdiff_hip_count_tables_merge_dev(
            self.h, S, kp, vp, nk, cap, self._ptr("keys", keys, torch.int64, (cap,)), self._ptr("vals", vals, torch.int32, (S, cap)), C.byref(n)))
        keys = keys[: n.value]
        return [(keys, vals[s, : n.value]) for s in range(S)]

    def region_avdist(self, d_bait, d_oe, d_region_ptr, id_min, d_midsum, d_chr=None):
        """avDist = mean(distSign) by regionID (chicdiff.R:1965-1967, :868-882) for CSR-ordered RU rows: the covariate
        IHWcorrection() takes from the long table."""
        torch = self.torch
        pb = self._ptr("d_bait", d_bait, torch.int32, (-1,))
        nru = d_bait.numel()
        po = self._ptr("d_oe", d_oe, torch.int32, (nru,))
        ptr = self._ptr("d_region_ptr", d_region_ptr, torch.int64, (-1,))
        pm = self._ptr("d_midsum", d_midsum, torch.int64, (-1,))
        nid = d_midsum.numel()
        pc = self._ptr_or_none("d_chr", d_chr, torch.int32, (nid,))
        n = d_region_ptr.numel() - 1
        out = torch.empty(n, dtype=torch.float64, device=self.device)
        self._check(self.lib.chicdiff_hip_region_avdist_dev(self.h, pb, po, nru, ptr, n, int(id_min), nid, pm, pc, out.data_ptr()))
        return out

    # -- a3 ---------------------------------------------------------------------------------
    def fragment_background(self, d_bait, d_oe, id_min, d_midsum, d_sj, d_si, d_tblb, d_tlb, d_T, distfun, only_fullmean=False):
        """Bmean, Tmean, FullMean (S, nru) for RU rows (d_bait, d_oe); tables as in the header.  ``only_fullmean``: the first two
        come back as None and are never written (FullMean is the one column DESeq2Wrap reads, chicdiff.R:896, :1543)."""
        torch = self.torch
        pb = self._ptr("d_bait", d_bait, torch.int32, (-1,))
        nru = d_bait.numel()
        po = self._ptr("d_oe", d_oe, torch.int32, (nru,))
        self._check_tensor("d_sj", d_sj, torch.float64, (-1, -1))
        S = d_sj.shape[0]
        nid, pm, tabs, _df = self._background(S, d_midsum, d_sj, d_si, d_tblb, d_tlb, d_T, distfun)
        outs = [None if (only_fullmean and k < 2) else torch.empty((S, nru), dtype=torch.float64, device=self.device) for k in range(3)]
        self._check(self.lib.chicdiff_hip_fragment_background_dev(
            self.h, pb, po, nru, int(id_min), nid, pm, S, *tabs, *[None if t is None else t.data_ptr() for t in outs]))
        return outs

    # -- f2: chinput columns -> key table of the count join -------------------------------------
    def count_table(self, d_bait, d_oe, d_N, d_bait_in_RU=None):
        """(keys, vals) of ``count_join`` from unsorted chinput columns; rows whose bait is not flagged in
        ``d_bait_in_RU`` (uint8 per ID) are dropped (chicdiff.R:828-831, :849)."""
        torch = self.torch
        pb = self._ptr("d_bait", d_bait, torch.int32, (-1,))
        n = d_bait.numel()
        po, pN = self._ptr("d_oe", d_oe, torch.int32, (n,)), self._ptr("d_N", d_N, torch.int32, (n,))
        pf, max_id = self._bait_flags(d_bait_in_RU)
        keys = torch.empty(n, dtype=torch.int64, device=self.device)
        vals = torch.empty(n, dtype=torch.int32, device=self.device)
        nk = C.c_int64(0)
        self._check(self.lib.chicdiff_hip_count_table_dev(self.h, pb, po, pN, n, pf, max_id, keys.data_ptr(), vals.data_ptr(), C.byref(nk)))
        return keys[: nk.value], vals[: nk.value]

    def _bait_flags(self, d_bait_in_RU):
        """uint8 per ID 0 .. max_id (non-zero = keep), or None = keep every bait -> (address, max_id)."""
        if d_bait_in_RU is None:
            return None, 0
        return self._ptr("d_bait_in_RU", d_bait_in_RU, self.torch.uint8, (-1,)), d_bait_in_RU.numel() - 1

    def _text(self, d_text):
        """The body of a text file, a one-dimensional uint8 device tensor -> (the tensor, or its copy on a 16-byte boundary where it
        does not start on one; its address)."""
        pt = self._ptr("d_text", d_text, self.torch.uint8, (-1,))
        if pt % 16:
            d_text = d_text.clone()
            pt = d_text.data_ptr()
        return d_text, pt

    def parse_chinput_text(self, d_text, cols):
        """The body of a .chinput file (the bytes after its header line) as a uint8 device tensor -> (bait, oe, N), int32 device
        tensors in file order; ``cols`` = the 0-based columns (ib, io, in) of baitID, otherEndID, N.  The rule stands above
        chicdiff_hip_chinput_parse_dev in include/chicdiff_hip.h.  A malformed line raises, the message naming its byte offset."""
        torch = self.torch
        d_text, pt = self._text(d_text)
        n = d_text.numel()
        ib, io, in_ = (int(x) for x in cols)
        nrows, bad = C.c_int64(0), C.c_int64(-1)
        # first with no room at all: the call reports the row count before it writes anything
        rc = self.lib.chicdiff_hip_chinput_parse_dev(self.h, pt, n, ib, io, in_, None, None, None, 0, C.byref(nrows), C.byref(bad))
        if rc and nrows.value == 0:
            self._check(rc)
        out = [torch.empty(nrows.value, dtype=torch.int32, device=self.device) for _ in range(3)]
        if nrows.value:
            rc = self.lib.chicdiff_hip_chinput_parse_dev(self.h, pt, n, ib, io, in_, out[0].data_ptr(), out[1].data_ptr(),
                                                         out[2].data_ptr(), nrows.value, C.byref(nrows), C.byref(bad))
            if rc:
                err = ChicdiffHipError(f"[{rc}] " + self.lib.chicdiff_hip_last_error(self.h).decode())
                err.offset = bad.value if bad.value >= 0 else None   # body-relative offset of the first malformed line
                raise err
        return tuple(out)

    def read_chinput(self, path, d_bait_in_RU=None, nthreads=0, device=False):
        """fread(chinput)[, c("baitID", "otherEndID", "N")] restricted to the RU baits -> (keys, vals) of ``count_join``
        (chicdiff.R:828-831, :849): text parsed by host threads, bait filter + sort on the device.  ``device=True``: the text goes up
        as bytes and is parsed there (chicdiff_hip_chinput_read_dev; ``nthreads`` is not used: the upload runs with the context's
        host_copy_threads) — the same triple."""
        torch = self.torch
        pf, max_id = self._bait_flags(d_bait_in_RU)
        nrows = C.c_int64(0)
        if device:
            self._check(self.lib.chicdiff_hip_chinput_read_dev(self.h, os.fsencode(path), C.byref(nrows)))
        else:
            self._check(self.lib.chicdiff_hip_chinput_read(self.h, os.fsencode(path), int(nthreads), C.byref(nrows)))
        keys = torch.empty(nrows.value, dtype=torch.int64, device=self.device)
        vals = torch.empty(nrows.value, dtype=torch.int32, device=self.device)
        nk = C.c_int64(0)
        self._check(self.lib.chicdiff_hip_chinput_table_dev(self.h, pf, max_id, keys.data_ptr(), vals.data_ptr(), C.byref(nk)))
        return keys[: nk.value], vals[: nk.value], nrows.value

    # -- readAndFilterPeakMatrix on the device (chicdiff.R:218-277) -------------------------------------
    def _peaks_empty(self, n, ns):
        torch = self.torch
        return (torch.empty((6, n), dtype=torch.int32, device=self.device), torch.empty(n, dtype=torch.float64, device=self.device),
                torch.empty((ns, n), dtype=torch.float64, device=self.device), torch.empty(n, dtype=torch.int64, device=self.device))

    def parse_peaks_text(self, d_text, sep, score_cols):
        """The body of a peak matrix (the bytes after its header line) as a uint8 device tensor -> ``Peaks``; ``sep``: the separator
        (one character), ``score_cols``: the 0-based fields of the score columns, ascending, from 11 on.  The rule stands above
        chicdiff_hip_peaks_parse_dev in include/chicdiff_hip.h.  A malformed line raises, ``.offset`` its body offset."""
        d_text, pt = self._text(d_text)
        n = d_text.numel()
        cols, cp = self._host("score_cols", score_cols, np.int32, (-1,))
        ns = len(cols)
        sepb = ord(sep) if isinstance(sep, str) else int(sep)
        info = (C.c_int64 * len(PEAKS_INFO))()
        # first with no room at all: the call reports the row count before it writes anything
        rc = self.lib.chicdiff_hip_peaks_parse_dev(self.h, pt, n, sepb, cp, ns, None, None, None, None, 0, info)
        if rc and info[0] == 0:
            self._check(rc)
        if info[1]:
            return Peaks(dict(zip(PEAKS_INFO, info)))
        ints, dist, scores, line_off = self._peaks_empty(info[0], ns)
        if info[0]:
            rc = self.lib.chicdiff_hip_peaks_parse_dev(self.h, pt, n, sepb, cp, ns, ints.data_ptr(), dist.data_ptr(),
                                                       scores.data_ptr(), line_off.data_ptr(), info[0], info)
            if rc:
                err = ChicdiffHipError(f"[{rc}] " + self.lib.chicdiff_hip_last_error(self.h).decode())
                err.offset = info[4] if info[4] >= 0 else None
                raise err
        d = dict(zip(PEAKS_INFO, info))
        return Peaks(d) if d["status"] else Peaks(d, ints, dist, scores, line_off)

    def read_peaks(self, path, targetColumns, text_keys=False):
        """fread(peakFile)[, c(1:11, sel)] on the device (chicdiff_hip_peaks_read_dev): header on the host, the body uploaded as bytes
        and parsed there -> ``Peaks`` (its tensors are copies of the context's columns).  ``status`` != 0: the caller reads the file
        some other way.  A header the rule refuses or a malformed row raises.  ``text_keys=True``: the sort keys of the four text
        columns are taken from the body while it is still on the device (chicdiff_hip_peaks_textkeys_dev), for ``merge_peaks``."""
        targets = list(targetColumns)
        info = (C.c_int64 * len(PEAKS_INFO))()
        st = (C.c_int32 * max(len(targets), 1))()
        self._check(self.lib.chicdiff_hip_peaks_read_dev(self.h, os.fsencode(path), _c_strings(targets), len(targets), st, info))
        d = dict(zip(PEAKS_INFO, info))
        names = [targets[st[j]] for j in range(d["nscore"])]
        if d["status"]:
            return Peaks(d, score_names=names, path=path)
        ints, dist, scores, line_off = self._peaks_empty(d["nrows"], d["nscore"])
        if d["nrows"]:
            self._check(self.lib.chicdiff_hip_peaks_columns_dev(self.h, ints.data_ptr(), dist.data_ptr(), scores.data_ptr(), line_off.data_ptr(),
                                                                d["nrows"]))
        pk = Peaks(d, ints, dist, scores, line_off, score_names=names, path=path)
        if text_keys:
            self.peaks_text_keys(pk)
        return pk

    def peaks_text_keys(self, pk):
        """The sort keys of the four text columns of ``pk``, the ``Peaks`` of the ``read_peaks`` that came LAST on this context, taken
        from its body while that is still on the device (chicdiff_hip_peaks_textkeys_dev): sets ``chr_keys``, ``name_hash``,
        ``key_class``, ``key_status``."""
        torch = self.torch
        pk.chr_keys, pk.name_hash = (torch.empty((2, pk.n), dtype=torch.int64, device=self.device) for _ in range(2))
        ki = (C.c_int64 * 4)()
        self._check(self.lib.chicdiff_hip_peaks_textkeys_dev(self.h, pk.chr_keys.data_ptr(), pk.name_hash.data_ptr(), pk.n, ki))
        if ki[3] != pk.n:
            raise ChicdiffHipError("peaks_text_keys: another file was read on this context since")
        pk.key_status, pk.key_class = ki[0], (ki[1], ki[2])
        return pk

    def merge_peaks(self, peaks):
        """.multimerge (chicdiff.R:218-228, 234-236) of the ``Peaks`` of ``read_peaks(text_keys=True)``, one per file, in the files'
        order (chicdiff_hip_peaks_merge_dev; the rule stands above chicdiff_hip_peaks_textkeys_dev in include/chicdiff_hip.h) -> one
        ``Peaks`` in the pandas twin's row order, its score rows file after file, plus ``src_file`` / ``src_row`` / ``paths``.
        ``status`` != 0 (PEAKS_ST_MERGE_*): the device declined and no column is held.  The caller has checked that the files'
        chromosome columns have one class."""
        torch = self.torch
        peaks = list(peaks)
        F = len(peaks)
        if not 2 <= F <= PEAKS_MERGE_MAX_FILES:
            raise ValueError(f"merge_peaks: 2 .. {PEAKS_MERGE_MAX_FILES} files")
        if any(p.status or p.ints is None or p.chr_keys is None for p in peaks):
            raise ValueError("merge_peaks: every file comes from read_peaks(text_keys=True) with status 0")
        keep, arrs = [], []          # the columns as the C ABI reads them, and per column the files' addresses (NULL for no rows)
        for name, dtype in (("ints", torch.int32), ("dist", torch.float64), ("scores", torch.float64), ("chr_keys", torch.int64),
                            ("name_hash", torch.int64)):
            arr = (C.c_void_p * F)()
            for f, p in enumerate(peaks):
                shape = {"ints": (6, p.n), "dist": (p.n,), "scores": (p.nscore, p.n)}.get(name, (2, p.n))
                t = _contiguous(getattr(p, name))                              # (a merged file's columns are views)
                arr[f] = self._ptr(f"peaks[{f}].{name}", t, dtype, shape) or None
                keep.append(t)
            arrs.append(arr)
        nrows, nsc = (C.c_int64 * F)(*[p.n for p in peaks]), (C.c_int32 * F)(*[p.nscore for p in peaks])
        N, T = sum(p.n for p in peaks), sum(p.nscore for p in peaks)
        ints, dist, scores, _ = self._peaks_empty(N, T)
        src_file, src_row = torch.empty(N, dtype=torch.int32, device=self.device), torch.empty(N, dtype=torch.int64, device=self.device)
        info = (C.c_int64 * 2)()
        self._check(self.lib.chicdiff_hip_peaks_merge_dev(self.h, F, *arrs, nrows, nsc, N, ints.data_ptr(),
                                                          dist.data_ptr(), scores.data_ptr(), src_file.data_ptr(), src_row.data_ptr(), info))
        n = info[0]
        d = dict(zip(PEAKS_INFO, [0] * len(PEAKS_INFO)))
        d.update(nrows=n, status=info[1], maxbait=max(p.maxbait for p in peaks), nscore=T, bad=-1)
        names = [c for p in peaks for c in p.score_names]
        if d["status"]:
            out = Peaks(d, score_names=names)
        else:
            src_file, src_row = src_file[:n], src_row[:n]
            line_off = torch.empty(n, dtype=torch.int64, device=self.device)
            for f, p in enumerate(peaks):                                      # every merged row's line in its own file's body
                m = src_file == f
                line_off[m] = p.line_off[src_row[m]]
            out = Peaks(d, ints[:, :n], dist[:n], scores[:, :n], line_off, score_names=names)
            out.src_file, out.src_row = src_file, src_row
        out.paths = [p.path for p in peaks]
        out.bodies, out.seps = [p.info["body"] for p in peaks], [p.info["sep"] for p in peaks]
        return out

    def filter_peaks(self, peaks, score, cond_of_col, replicate_rule):
        """The four filters of readAndFilterPeakMatrix (chicdiff.R:246-270) on a ``Peaks``: ``cond_of_col[j]`` = the condition (0-based,
        -1 = none) of score row j.  Returns ``kept_idx`` (int64, file order), the kept rows' ``baitID`` / ``oeID`` (int32) and
        ``filtered_baits`` (int32: the baits without a kept row, in order of first appearance), device tensors."""
        torch = self.torch
        n, ns = peaks.n, peaks.nscore
        cond = np.ascontiguousarray(cond_of_col, dtype=np.int32)
        if cond.shape != (ns,):
            raise ValueError("filter_peaks: one condition per score column")
        ncond = int(cond.max()) + 1 if ns else 0
        if peaks.status or peaks.ints is None:
            raise ValueError("filter_peaks: a Peaks with status 0, its columns held, is required")
        bait, oe, dist, scores = (_contiguous(t) for t in (peaks.baitID, peaks.oeID, peaks.dist, peaks.scores))   # (views after a merge)
        pb, po = self._ptr("peaks.baitID", bait, torch.int32, (n,)), self._ptr("peaks.oeID", oe, torch.int32, (n,))
        pd, ps = self._ptr("peaks.dist", dist, torch.float64, (n,)), self._ptr("peaks.scores", scores, torch.float64, (ns, n))
        kept = torch.empty(n, dtype=torch.int64, device=self.device)
        kb, ko, fb = (torch.empty(n, dtype=torch.int32, device=self.device) for _ in range(3))
        nk, nf = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.chicdiff_hip_peaks_filter_dev(
            self.h, pb, po, pd, ps, n, ns, float(score), cond.ctypes.data_as(C.POINTER(C.c_int32)), ncond, int(bool(replicate_rule)),
            int(peaks.maxbait), kept.data_ptr(), kb.data_ptr(), ko.data_ptr(), fb.data_ptr(), C.byref(nk), C.byref(nf)))
        return dict(kept_idx=kept[: nk.value], baitID=kb[: nk.value], oeID=ko[: nk.value], filtered_baits=fb[: nf.value])

    # -- a9: results() ---------------------------------------------------------------------------
    def cooks_filter(self, d_counts, group, d_maxCooks, d_cooksArgmax, d_pvalue, cutoff):
        """p <- NA for Cook's outliers, in place on ``d_pvalue``; returns the number of rows set to NA."""
        torch = self.torch
        dc = self._ptr("d_counts", d_counts, torch.int32, (-1, -1))
        S, n = d_counts.shape
        g = self._group(group, S)
        pmc, pam = self._ptr("d_maxCooks", d_maxCooks, torch.float64, (n,)), self._ptr("d_cooksArgmax", d_cooksArgmax, torch.int32, (n,))
        pp = self._ptr("d_pvalue", d_pvalue, torch.float64, (n,))
        nout = C.c_int64(0)
        self._check(self.lib.chicdiff_hip_cooks_filter_dev(self.h, dc, n, S, g, pmc, pam, float(cutoff), pp, C.byref(nout)))
        return nout.value

    def independent_filtering(self, d_baseMean, d_pvalue, alpha=0.1):
        """DESeq2 pvalueAdjustment(independentFiltering = TRUE): returns (padj device tensor, info dict)."""
        torch = self.torch
        pp = self._ptr("d_pvalue", d_pvalue, torch.float64, (-1,))
        n = d_pvalue.numel()
        pm = self._ptr("d_baseMean", d_baseMean, torch.float64, (n,))
        padj = torch.empty(n, dtype=torch.float64, device=self.device)
        info = ResultsInfo()
        self._check(self.lib.chicdiff_hip_independent_filtering_dev(self.h, pm, pp, n, float(alpha), padj.data_ptr(), C.byref(info)))
        return padj, dict(filterThreshold=info.filterThreshold, filterTheta=info.filterTheta, index=info.index,
                          theta=np.array(info.theta[:]), numRej=np.array(info.numRej[:]), lowess=np.array(info.lowess[:]))

    # -- f1 / f3: BH and the IHW application side ----------------------------------------------
    def bh_adjust(self, d_p):
        """p.adjust(p, "BH") on a device vector (NaN = NA)."""
        torch = self.torch
        pp = self._ptr("d_p", d_p, torch.float64, (-1,))
        out = torch.empty_like(d_p)
        self._check(self.lib.chicdiff_hip_bh_adjust_dev(self.h, pp, d_p.numel(), out.data_ptr()))
        return out

    def ihw_apply(self, d_avDist, d_pvalue, breaks, avWeights):
        """chicdiff.R:2038-2049: returns dict(group, weight, weighted_pvalue, weighted_padj) of device tensors."""
        torch = self.torch
        pa = self._ptr("d_avDist", d_avDist, torch.float64, (-1,))
        n = d_avDist.numel()
        pp = self._ptr("d_pvalue", d_pvalue, torch.float64, (n,))
        w, pw = self._host("avWeights", avWeights, np.float64, (-1,))
        b, pb = self._host("breaks", breaks, np.float64, (len(w) + 1,))
        group = torch.empty(n, dtype=torch.int32, device=self.device)
        weight, wp, wpadj = (torch.empty(n, dtype=torch.float64, device=self.device) for _ in range(3))
        self._check(self.lib.chicdiff_hip_ihw_apply_dev(self.h, pa, pp, n, pb, pw, len(w), group.data_ptr(), weight.data_ptr(),
                                                        wp.data_ptr(), wpadj.data_ptr()))
        return dict(group=group, weight=weight, weighted_pvalue=wp, weighted_padj=wpadj)

    def _ihw_args(self, d_pvalue, d_covariate, nbins, nfolds, seed, chunk_len):
        torch = self.torch
        pp = self._ptr("d_pvalue", d_pvalue, torch.float64, (-1,))
        pc = self._ptr("d_covariate", d_covariate, torch.float64, (d_pvalue.numel(),))
        sd = self._seed("ihw_train", seed)
        return pp, pc, d_pvalue.numel(), 0 if nbins is None else int(nbins), int(nfolds), sd, 0 if chunk_len is None else int(chunk_len)

    def ihw_train(self, d_pvalue, d_covariate, alpha=0.05, nbins=None, nfolds=5, seed=0, chunk_len=None):
        """The training side of IHWcorrection, ihw(pvalue ~ covariate, alpha) of chicdiff.R:1994, by this library's own statement of
        it (the rule and its differences from the IHW package are above chicdiff_hip_ihw_train_dev in include/chicdiff_hip.h).
        ``d_pvalue, d_covariate``: float64 (n,) device tensors, NaN p = a row left out; ``nbins`` None = automatic; ``chunk_len`` None
        = the default, else one of ``ihw_caps()["chunk_lens"]`` (the results never depend on it).

        Returns dict(group, fold: int32 device tensors (INT32_MIN / -1 on left-out rows), weights: (nbins, nfolds) numpy array,
        m, nbins, nseg, T, H: the info block)."""
        torch = self.torch
        pp, pc, n, nb, nf, sd, cl = self._ihw_args(d_pvalue, d_covariate, nbins, nfolds, seed, chunk_len)
        group, fold = (torch.empty(max(n, 1), dtype=torch.int32, device=self.device) for _ in range(2))
        w = np.zeros(IHW_MAX_FOLDS * 256, dtype=np.float64)
        info = IhwInfo()
        info.chunk_len = cl
        self._check(self.lib.chicdiff_hip_ihw_train_dev(self.h, pp, pc, n, float(alpha), nb, nf, sd,
                                                        group.data_ptr(), fold.data_ptr(), w.ctypes.data, C.byref(info)))
        self.last_ihw_train_ms = {k: v[0] for k, v in self.kernel_times().items() if k.startswith("ihw_")}
        k = info.nbins
        return dict(group=group[:n], fold=fold[:n], weights=w[: k * nf].reshape(nf, k).T.copy(), m=info.m, nbins=k, chunk_len=info.chunk_len,
                    nseg=np.array(info.nseg[:nf]), T=np.array(info.T[:nf]), H=np.array(info.H[:nf]))

    def selftest_ihw_knots(self, d_pvalue, d_covariate, nbins=None, nfolds=5, seed=0, chunk_len=None):
        """The knots of every (fold, group) as the device finds them (chicdiff_hip_selftest_ihw_knots_dev): dict(ptr, x, c, nbins),
        entry f * nbins + (g - 1) owning x, c [ptr[q] .. ptr[q + 1])."""
        pp, pc, n, nb, nf, sd, cl = self._ihw_args(d_pvalue, d_covariate, nbins, nfolds, seed, chunk_len)
        k, nk = C.c_int32(0), C.c_int64(0)
        args = (self.h, pp, pc, n, nb, nf, sd, cl)
        self._check(self.lib.chicdiff_hip_selftest_ihw_knots_dev(*args, 0, None, None, None, C.byref(k), C.byref(nk)))
        ptr = np.zeros(nf * k.value + 1, dtype=np.int64)
        x, c = np.zeros(nk.value, dtype=np.float64), np.zeros(nk.value, dtype=np.int32)
        self._check(self.lib.chicdiff_hip_selftest_ihw_knots_dev(*args, nk.value, ptr.ctypes.data, x.ctypes.data, c.ctypes.data, C.byref(k),
                                                                 C.byref(nk)))
        return dict(ptr=ptr, x=x, c=c, nbins=k.value)

    # -- f4: region universe ---------------------------------------------------------------------
    def region_universe(self, d_bait, d_oe, RUexpand, d_chr_of):
        """getRegionUniverse window mode (chicdiff.R:353-426).  d_chr_of: int32 (maxfrag + 1,), -1 = not on the map.
        Returns dict(region_ptr, minOE, maxOE, baitID, regionID, otherEndID); the RU rows are in
        (regionID, otherEndID) order."""
        torch = self.torch
        pb = self._ptr("d_bait", d_bait, torch.int32, (-1,))
        n = d_bait.numel()
        po = self._ptr("d_oe", d_oe, torch.int32, (n,))
        pc = self._ptr("d_chr_of", d_chr_of, torch.int32, (-1,))
        maxfrag = d_chr_of.numel() - 1
        ptr = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        mn, mx = (torch.empty(n, dtype=torch.int32, device=self.device) for _ in range(2))
        total = C.c_int64(0)
        cap = n * max(2 * int(RUexpand) + 1, 2)   # the upper bound (two for RUexpand = 0: R's descending a:b beside a bait): scan and fill in one call (round 5)
        rb, rr, ro = (torch.empty(max(cap, 1), dtype=torch.int32, device=self.device) for _ in range(3))
        self._check(self.lib.chicdiff_hip_region_universe_dev(
            self.h, pb, po, n, int(RUexpand), pc, maxfrag, ptr.data_ptr(), mn.data_ptr(), mx.data_ptr(), rb.data_ptr(), rr.data_ptr(),
            ro.data_ptr(), cap, C.byref(total)))
        self.last_region_universe_ms = self.kernel_times().get("region_universe", (0.0, 0))[0]
        rb, rr, ro = rb[: total.value], rr[: total.value], ro[: total.value]
        if 2 * total.value < cap:  # (a view would pin the whole upper-bound allocation for as long as the universe lives)
            rb, rr, ro = rb.clone(), rr.clone(), ro.clone()
        return dict(region_ptr=ptr, minOE=mn, maxOE=mx, baitID=rb, regionID=rr, otherEndID=ro)

    # -- getCandidateInteractions ----------------------------------------------------------------
    def candidate_interactions(self, d_baitID, d_minOE, d_maxOE, d_p, d_peak_baitID, d_peak_oeID, d_scores, ncond1, ncond2, merged,
                               score, pvcut, minDeltaAsinhScore, pair_row=None, method="min"):
        """getCandidateInteractions' join and filter (chicdiff.R:2068-2163; the rules are above
        chicdiff_hip_candidate_interactions_dev in include/chicdiff_hip.h).  Region table: int32 (n,) tensors and the chosen
        p column, float64 (n,), in the rows' own order; peak matrix rows as read: int32 (npeaks,) IDs and ``d_scores`` of shape
        (ncols, npeaks), contiguous (= the C ABI's column-major npeaks x ncols), condition 1's columns first.

        Returns dict(group_peak, group_ptr, group_min_p, group_delta, pair_row, ngroups, npairs), the tensors trimmed to the
        surviving groups and their pairs.  The first call gives room for 16 npeaks pairs; if that is too little (duplicate
        regions have no bound) it is repeated once with exactly the reported need.  ``pair_row``: a caller's int32 buffer
        instead — its length is the capacity, and there is no second call: too small raises, with ``.need = (ngroups, npairs)``.

        ``method``: "min" or "hmp" (or the C ABI's CHICDIFF_CAND_* number) — what ``group_min_p`` carries and the filter reads:
        the minimum of the group's p values, or harmonicmeanp::p.hmp of them (chicdiff_hip_candidate_interactions_method_dev)."""
        torch = self.torch
        if isinstance(method, str):
            if method not in CAND_METHODS:
                raise ValueError(f"candidate_interactions: unknown method {method!r} (should be 'min' or 'hmp')")
            method = CAND_METHODS[method]
        pb = self._ptr("d_baitID", d_baitID, torch.int32, (-1,))
        n = d_baitID.numel()
        pmn, pmx = self._ptr("d_minOE", d_minOE, torch.int32, (n,)), self._ptr("d_maxOE", d_maxOE, torch.int32, (n,))
        pp = self._ptr("d_p", d_p, torch.float64, (n,))
        ps = self._ptr("d_scores", d_scores, torch.float64, (-1, -1))
        ncols, npeaks = d_scores.shape
        ppb = self._ptr("d_peak_baitID", d_peak_baitID, torch.int32, (npeaks,))
        ppo = self._ptr("d_peak_oeID", d_peak_oeID, torch.int32, (npeaks,))
        gpeak = torch.empty(max(npeaks, 1), dtype=torch.int32, device=self.device)
        gptr = torch.empty(npeaks + 1, dtype=torch.int64, device=self.device)
        gmin, gdelta = (torch.empty(max(npeaks, 1), dtype=torch.float64, device=self.device) for _ in range(2))
        ng, npairs = C.c_int64(0), C.c_int64(0)

        def call(pairs):
            ppairs = self._ptr("pair_row", pairs, torch.int32, (-1,))
            return self.lib.chicdiff_hip_candidate_interactions_method_dev(
                self.h, pb, pmn, pmx, pp, n, ppb, ppo, ps, npeaks, ncols, int(ncond1), int(ncond2), int(bool(merged)), float(score),
                float(pvcut), float(minDeltaAsinhScore), int(method), pairs.numel(), gpeak.data_ptr(), gptr.data_ptr(), gmin.data_ptr(),
                gdelta.data_ptr(), ppairs, C.byref(ng), C.byref(npairs))

        own = pair_row is None
        pairs = torch.empty(max(16 * npeaks, 1), dtype=torch.int32, device=self.device) if own else pair_row
        rc = call(pairs)
        if rc and npairs.value > pairs.numel():          # the capacity status: both counts are written, no pair is
            if not own:
                e = ChicdiffHipError(f"[{rc}] " + self.lib.chicdiff_hip_last_error(self.h).decode())
                e.need = (ng.value, npairs.value)
                raise e
            pairs = torch.empty(npairs.value, dtype=torch.int32, device=self.device)
            rc = call(pairs)
        self._check(rc)
        self.last_candidates_ms = self.kernel_times().get("candidates", (0.0, 0))[0]
        g, m = ng.value, npairs.value
        pairs = pairs[:m]
        if own and 2 * m < pairs.numel():   # (a view would pin the whole 16 npeaks allocation)
            pairs = pairs.clone()
        return dict(group_peak=gpeak[:g].clone(), group_ptr=gptr[: g + 1].clone(), group_min_p=gmin[:g].clone(), group_delta=gdelta[:g].clone(),
                    pair_row=pairs, ngroups=g, npairs=m)

    # -- getControlRegionUniverse: the seeded draws ------------------------------------------------
    def control_draws(self, d_ru_baitID, d_region_ptr, d_minOE, d_maxOE, d_bmap_id, d_bmap_chr, chr_min, chr_max, seed):
        """The draws of getControlRegionUniverse from a seed (chicdiff.R:430-481; the rules and the Philox counter layout are above
        chicdiff_hip_control_draws_dev in include/chicdiff_hip.h).  RU as ``region_universe`` returns it: ``d_ru_baitID`` int32 (nru,)
        in (regionID, otherEndID) order, ``d_region_ptr`` int64 (n + 1,), ``d_minOE, d_maxOE`` int32 (n,).  The baitmap in file
        order: ``d_bmap_id, d_bmap_chr`` int32 (nb,) device tensors, the chromosome as a code of the restriction map (-1 = a name
        not on it); ``chr_min, chr_max``: host arrays, smallest and largest map ID per code; ``seed``: 0 <= seed < 2^64.

        Returns dict(baitID, oeID, max_contact, n_regions, m): the m kept pairs sorted by (baitID, oeID) as int32 device tensors,
        the largest contact per chromosome code (int32 device tensor, 0 = none) and the number of non-empty regions of RU."""
        torch = self.torch
        pru = self._ptr("d_ru_baitID", d_ru_baitID, torch.int32, (-1,))
        ptr = self._ptr("d_region_ptr", d_region_ptr, torch.int64, (-1,))
        n = d_region_ptr.numel() - 1
        if n < 1:
            raise ValueError("control_draws: region_ptr must hold at least one region (two entries)")
        pmn, pmx = self._ptr("d_minOE", d_minOE, torch.int32, (n,)), self._ptr("d_maxOE", d_maxOE, torch.int32, (n,))
        pbi = self._ptr("d_bmap_id", d_bmap_id, torch.int32, (-1,))
        nb = d_bmap_id.numel()
        if nb < 1:
            raise ValueError("control_draws: the baitmap is empty (nb = 0)")
        pbc = self._ptr("d_bmap_chr", d_bmap_chr, torch.int32, (nb,))
        lo, hi = (np.ascontiguousarray(a, dtype=np.int32) for a in (chr_min, chr_max))
        if lo.ndim != 1 or lo.shape != hi.shape or len(lo) < 1:
            raise ValueError(f"chr_min, chr_max: two vectors of one length >= 1 are required, got shapes {lo.shape} and {hi.shape}")
        seed = self._seed("control_draws", seed)
        bait, oe = (torch.empty(n, dtype=torch.int32, device=self.device) for _ in range(2))
        contact = torch.empty(len(lo), dtype=torch.int32, device=self.device)
        n_regions, m = C.c_int64(0), C.c_int64(0)
        P = C.POINTER(C.c_int32)
        self._check(self.lib.chicdiff_hip_control_draws_dev(
            self.h, pru, d_ru_baitID.numel(), ptr, pmn, pmx, n, pbi, pbc, nb, lo.ctypes.data_as(P), hi.ctypes.data_as(P), len(lo), seed,
            bait.data_ptr(), oe.data_ptr(), contact.data_ptr(), C.byref(n_regions), C.byref(m)))
        self.last_control_draws_ms = self.kernel_times().get("control_draws", (0.0, 0))[0]
        k = m.value
        if 2 * k < n:   # (a view would pin the whole n-entry allocation)
            bait, oe = bait[:k].clone(), oe[:k].clone()
        return dict(baitID=bait[:k], oeID=oe[:k], max_contact=contact, n_regions=n_regions.value, m=k)

    # -- the Chicago background tables ----------------------------------------------------------
    def chicago_tables(self, d_bait, d_oe, d_s_j, d_s_i, d_Tmean, d_refBinMean, d_tblb, d_tlb, d_distbin, id_min, ndistbin,
                       sj, si, tblb_of, tlb_of, T, ref=None):
        """The background tables of ONE replicate from the columns of its Chicago table, rows in any order (chicdiff.R:656-692,
        538-548; the winner rule is above chicdiff_hip_chicago_tables_dev in include/chicdiff_hip.h).  Columns: int32 IDs, float64
        values (NaN = NA), int32 level codes (-1 = NA), all (nrows,).  Outputs, written in place: ``sj, si`` float64 and
        ``tblb_of, tlb_of`` int32 (nid,) — row s of the (S, nid) tables ``fragment_background`` takes; ``T`` float64 (ntblb, ntlb).
        Returns (ref, flag): ``ref`` float64 (ndistbin + 1,), the refBinMean of every distbin code (last entry: the NA code; NaN =
        none), and whether some code carries two different values — ``ref`` is then not the distance function's input, and the
        caller builds that replicate's on the host."""
        torch = self.torch
        pb = self._ptr("d_bait", d_bait, torch.int32, (-1,))
        n = d_bait.numel()
        if not 1 <= n < 1 << 32:
            raise ValueError(f"chicago_tables: 1 <= nrows < 2^32 rows are supported, got {n}")
        cols = [pb, self._ptr("d_oe", d_oe, torch.int32, (n,))]
        cols += [self._ptr(name, t, torch.float64, (n,))
                 for name, t in (("d_s_j", d_s_j), ("d_s_i", d_s_i), ("d_Tmean", d_Tmean), ("d_refBinMean", d_refBinMean))]
        cols += [self._ptr(name, t, torch.int32, (n,)) for name, t in (("d_tblb", d_tblb), ("d_tlb", d_tlb), ("d_distbin", d_distbin))]
        psj = self._ptr("sj", sj, torch.float64, (-1,))
        nid = sj.numel()
        if nid < 1:
            raise ValueError("sj: empty restriction map")
        outs = [psj, self._ptr("si", si, torch.float64, (nid,)), self._ptr("tblb_of", tblb_of, torch.int32, (nid,)),
                self._ptr("tlb_of", tlb_of, torch.int32, (nid,)), self._ptr("T", T, torch.float64, (-1, -1))]
        caps = chicago_tables_caps()
        if T.shape[0] < 1 or T.shape[1] < 1 or T.numel() > caps["max_pairs"]:
            raise ValueError(f"T: shape (ntblb >= 1, ntlb >= 1) with at most {caps['max_pairs']} cells is required, got {tuple(T.shape)}")
        ndistbin = int(ndistbin)
        if not 0 <= ndistbin <= caps["max_distbin"]:
            raise ValueError(f"chicago_tables: 0 <= ndistbin <= {caps['max_distbin']} is required, got {ndistbin}")
        if ref is None:
            ref = torch.empty(ndistbin + 1, dtype=torch.float64, device=self.device)
        outs.append(self._ptr("ref", ref, torch.float64, (ndistbin + 1,)))
        flag = C.c_int32(0)
        self._check(self.lib.chicdiff_hip_chicago_tables_dev(self.h, *cols, n, int(id_min), nid, T.shape[0], T.shape[1], ndistbin, *outs,
                                                             C.byref(flag)))
        kt = self.kernel_times()
        self.last_chicago_tables_ms = {k[len("chicago_tables_"):]: v[0] for k, v in kt.items() if k.startswith("chicago_tables_")}
        return ref, bool(flag.value)

    # -- countput ---------------------------------------------------------------------------------
    def countput(self, reps, id_min, d_midsum, d_chr):
        """countput of ONE condition (chicdiff.R:708-735, 754-768; the rule is above chicdiff_hip_countput_dev in
        include/chicdiff_hip.h): ``reps`` = [(baitID, otherEndID, N, Bmean, score, distSign)] per replicate, in the order the rows
        are to be stacked — int32, int32, int32, float64, float64, float64 device tensors of one length per replicate (0 rows are
        fine).  The map: ``id_min``, ``d_midsum`` int64 (nid,), ``d_chr`` int32 (nid,), -1 = not on the map.

        Returns dict(baitID, otherEndID, Nav, Bav, score, oeID_mid): one entry per (baitID, otherEndID) group in order of first
        appearance, int32 / float64 device tensors — pipeline._countput's frame for that condition, bit for bit."""
        torch = self.torch
        reps = [tuple(r) for r in reps]
        caps = countput_caps()
        if not 1 <= len(reps) <= caps["max_rep"]:
            raise ValueError(f"countput: 1 <= replicates <= {caps['max_rep']} are supported, got {len(reps)}")
        dtypes = (torch.int32, torch.int32, torch.int32, torch.float64, torch.float64, torch.float64)
        names = ("baitID", "otherEndID", "N", "Bmean", "score", "distSign")
        nrep = len(reps)
        ptrs = [(C.c_void_p * nrep)() for _ in range(6)]
        for r, cols in enumerate(reps):
            if len(cols) != 6:
                raise ValueError(f"countput: replicate {r} must be (baitID, otherEndID, N, Bmean, score, distSign), got {len(cols)} columns")
            ptrs[0][r] = self._ptr(f"reps[{r}].baitID", cols[0], torch.int32, (-1,)) or None
            for k in range(1, 6):
                ptrs[k][r] = self._ptr(f"reps[{r}].{names[k]}", cols[k], dtypes[k], (cols[0].numel(),)) or None
        pm = self._ptr("d_midsum", d_midsum, torch.int64, (-1,))
        nid = d_midsum.numel()
        if nid < 1:
            raise ValueError("d_midsum: empty restriction map")
        pc = self._ptr("d_chr", d_chr, torch.int32, (nid,))
        n = sum(cols[0].numel() for cols in reps)
        if n >= 1 << 31:
            raise ValueError(f"countput: the replicates of one condition must hold fewer than 2^31 rows together, got {n}")
        nrows = (C.c_int64 * nrep)(*[cols[0].numel() for cols in reps])
        ob, oo = (torch.empty(n, dtype=torch.int32, device=self.device) for _ in range(2))
        nav, bav, sc, mid = (torch.empty(n, dtype=torch.float64, device=self.device) for _ in range(4))
        g = C.c_int64(0)
        self._check(self.lib.chicdiff_hip_countput_dev(
            self.h, nrep, *ptrs, nrows, int(id_min), nid, pm, pc, ob.data_ptr(), oo.data_ptr(),
            nav.data_ptr(), bav.data_ptr(), sc.data_ptr(), mid.data_ptr(), C.byref(g)))
        self.last_countput_ms = self.kernel_times().get("countput", (0.0, 0))[0]
        k = g.value
        out = dict(baitID=ob[:k], otherEndID=oo[:k], Nav=nav[:k], Bav=bav[:k], score=sc[:k], oeID_mid=mid[:k])
        if 2 * k < n:   # (a view would pin the whole n-entry allocation)
            out = {name: t.clone() for name, t in out.items()}
        return out

    # -- tables as text ---------------------------------------------------------------------------
    def table_text(self, columns, sep=",", n=None):
        """A table of device columns as text, what ``DataFrame.to_csv(index=False)`` writes below its header, byte for byte
        (chicdiff_hip_table_text_dev; the rule stands above it in include/chicdiff_hip.h): a uint8 device tensor.  ``columns`` as for
        ``table_columns``; 2 .. 64 of them."""
        torch = self.torch
        columns = list(columns)
        arr, n, keep = table_columns(columns, n=n, device=self.device)
        sepb, size = _sep_byte(sep), C.c_int64(0)
        self._check(self.lib.chicdiff_hip_table_text_dev(self.h, arr, len(columns), n, sepb, None, 0, C.byref(size)))
        out = torch.empty(size.value, dtype=torch.uint8, device=self.device)
        if size.value:
            self._check(self.lib.chicdiff_hip_table_text_dev(self.h, arr, len(columns), n, sepb, out.data_ptr(), size.value, C.byref(size)))
        return out

    def write_table(self, path, columns, header, append=False, sep=",", n=None):
        """The same text into the file ``path`` (chicdiff_hip_table_write_dev): the line of the column names ``header`` first, unless
        ``append`` — then the rows go behind what the file holds.  Returns the bytes written.  ``last_table_write_ms``: the call's
        timers (len, scan, write, download) when timing is enabled."""
        columns = list(columns)
        arr, n, keep = table_columns(columns, n=n, device=self.device)
        names = [str(h) for h in header]
        if len(names) != len(columns):
            raise ValueError(f"write_table: {len(columns)} column names are required, got {len(names)}")
        head = (sep.join(names) + "\n").encode()
        written = C.c_int64(0)
        self._check(self.lib.chicdiff_hip_table_write_dev(self.h, os.fsencode(path), int(bool(append)), head, len(head), arr, len(columns), n,
                                                          _sep_byte(sep), C.byref(written)))
        kt = self.kernel_times()
        self.last_table_write_ms = {k[len("table_"):]: v[0] for k, v in kt.items() if k.startswith("table_")}
        return written.value

    def selftest_format_double_dev(self, d_x):
        """The library's double -> text function on the device (chicdiff_hip_selftest_format_double_dev): the cells as a list of bytes."""
        torch = self.torch
        px = self._ptr("d_x", d_x, torch.float64, (-1,))
        n = d_x.numel()
        text = torch.empty((n, TABLE_MAX_CELL_BYTES), dtype=torch.uint8, device=self.device)
        length = torch.empty(n, dtype=torch.int32, device=self.device)
        self._check(self.lib.chicdiff_hip_selftest_format_double_dev(self.h, px, n, text.data_ptr(), length.data_ptr()))
        return _format_double_cells(text.cpu().numpy(), length.cpu().numpy())

    # -- a6 + a7 ----------------------------------------------------------------------------
    def nbglm_fit(self, d_counts, d_nf, group, want=None, opts: Opts | None = None, outputs: dict | None = None):
        """estimateDispersions + nbinomWaldTest on device-resident (S, n) tensors.

        Returns (outputs, scalars): ``outputs`` maps the requested column names to device
        tensors of length n (pass ``outputs`` to reuse buffers)."""
        pk, pnf, S, n = self._matrices("d_nf", d_counts, d_nf)
        g, o = self._group(group, S), self._opts(opts)
        out, bufs = self._outputs(want, FIT_COLUMNS, n, outputs)
        sc = Scalars()
        self._check(self.lib.chicdiff_hip_nbglm_fit_dev(self.h, pk, pnf, n, S, g, o, C.byref(out), C.byref(sc)))
        return bufs, _scalars_dict(sc)

    def wald_test(self, d_counts, d_fullmean, group, theta=None, want=None, opts: Opts | None = None,
                  outputs: dict | None = None):
        """size factors -> offsets(theta) -> dispersions -> Wald test in one enqueue (device-resident)."""
        pk, pfm, S, n = self._matrices("d_fullmean", d_counts, d_fullmean)
        g, o = self._group(group, S), self._opts(opts)
        out, bufs = self._outputs(want, FIT_COLUMNS, n, outputs)
        sc = Scalars()
        sf = (C.c_double * S)()
        self._check(self.lib.chicdiff_hip_wald_test_dev(self.h, pk, pfm, n, S, g, float("nan") if theta is None else float(theta), o,
                                                        C.byref(out), C.byref(sc), sf))
        res = _scalars_dict(sc)
        res["sizeFactors"] = np.array(sf[:])
        return bufs, res

    def nbglm_fit_host(self, counts, nf, group, want=None, opts: Opts | None = None):
        """Host-buffer entry point (what the R .Call shim uses): numpy (n, S) in, numpy out."""
        k = np.asfortranarray(np.asarray(counts, dtype=np.int32))
        f = np.asfortranarray(np.asarray(nf, dtype=np.float64))
        if k.ndim != 2 or f.shape != k.shape:
            raise ValueError(f"counts, nf: two (n, S) matrices of one shape are required, got shapes {k.shape} and {f.shape}")
        n, S = k.shape
        g, o = self._group(group, S), self._opts(opts)
        out, res = self._outputs(want, OUT_DOUBLE + OUT_INT, n, host=True)
        sc = Scalars()
        self._check(self.lib.chicdiff_hip_nbglm_fit(self.h, k.ctypes.data, f.ctypes.data, n, S, g, o, C.byref(out), C.byref(sc)))
        return res, _scalars_dict(sc)

    # -- a8 ---------------------------------------------------------------------------------
    def theta_grid(self, d_counts, d_fullmean, size_factors, thetas, opts: Opts | None = None) -> np.ndarray:
        pk, pfm, S, n = self._matrices("d_fullmean", d_counts, d_fullmean)
        sf, psf = self._host("size_factors", size_factors, np.float64, (S,))
        th, pth = self._host("thetas", thetas, np.float64, (-1,))
        o = self._opts(opts)
        dev = (C.c_double * len(th))()
        self._check(self.lib.chicdiff_hip_theta_grid_dev(self.h, pk, pfm, psf, n, S, pth, len(th), o, dev))
        return np.array(dev[:])

    def selftest_math(self, op: int, d_x):
        px = self._ptr("d_x", d_x, self.torch.float64)
        out = self.torch.empty_like(d_x)
        self._check(self.lib.chicdiff_hip_selftest_math_dev(self.h, op, px, d_x.numel(), out.data_ptr()))
        return out

    def selftest_landau(self, d_z):
        """landau_tail(z) (devmath.h), the Landau tail behind method = "hmp", as the overlap kernel calls it."""
        pz = self._ptr("d_z", d_z, self.torch.float64)
        out = self.torch.empty_like(d_z)
        self._check(self.lib.chicdiff_hip_selftest_landau_dev(self.h, pz, d_z.numel(), out.data_ptr()))
        return out

    def selftest_math3(self, op: int, d_x, d_y):
        """Two-argument / two-result building blocks (include/chicdiff_hip.h: the op numbers) -> (out, out2)."""
        px = self._ptr("d_x", d_x, self.torch.float64)
        py = self._ptr("d_y", d_y, self.torch.float64, tuple(d_x.shape))
        out, out2 = self.torch.empty_like(d_x), self.torch.empty_like(d_x)
        self._check(self.lib.chicdiff_hip_selftest_math3_dev(self.h, op, px, py, d_x.numel(), out.data_ptr(), out2.data_ptr()))
        return out, out2

    def selftest_objective(self, d_counts, d_nf, group, d_log_alpha, d_prior_mean=None, prior_var=1.0, live_rows=0,
                           opts: Opts | None = None):
        """The dispersion objective at d_log_alpha (n, K): dict of lp, dlp, alpha (n, K), mu (S, n) and lanes_per_row."""
        t = self.torch
        pk, pnf, S, n = self._matrices("d_nf", d_counts, d_nf)
        pla = self._ptr("d_log_alpha", d_log_alpha, t.float64, (n, -1))
        K = d_log_alpha.shape[1]
        ppm = self._ptr_or_none("d_prior_mean", d_prior_mean, t.float64, (n,))
        g, o = self._group(group, S), self._opts(opts)
        lp, dlp, alpha = (t.empty((n, K), dtype=t.float64, device=self.device) for _ in range(3))
        mu = t.empty((S, n), dtype=t.float64, device=self.device)
        lanes = C.c_int32(0)
        self._check(self.lib.chicdiff_hip_selftest_objective_dev(
            self.h, pk, pnf, n, S, g, o, pla, K, ppm, float(prior_var),
            int(live_rows), lp.data_ptr(), dlp.data_ptr(), alpha.data_ptr(), mu.data_ptr(), C.byref(lanes)))
        return dict(lp=lp, dlp=dlp, alpha=alpha, mu=mu, lanes_per_row=lanes.value)

    def selftest_global_stage(self, d_baseMean, d_dispGeneEst, d_allZero, S, p, opts: Opts | None = None):
        """TEST ENTRY: the fit's global stage (trend, residuals, median / MAD, prior variance) on the caller's columns.  Returns a dict:
        dispFit, resid (device tensors, n), hist (40 counts), vertices (dict of nv and x, h, f, d: the local trend's, ascending x)
        and the scalars with their status bits."""
        t = self.torch
        pbm = self._ptr("d_baseMean", d_baseMean, t.float64, (-1,))
        n = d_baseMean.numel()
        pdg = self._ptr("d_dispGeneEst", d_dispGeneEst, t.float64, (n,))
        paz = self._ptr("d_allZero", d_allZero, t.int32, (n,))
        o = self._opts(opts)
        fit, resid = (t.empty(n, dtype=t.float64, device=self.device) for _ in range(2))
        hist = (C.c_double * 40)()
        nv = C.c_int32(0)
        vx, vh, vf, vd = ((C.c_double * 100)() for _ in range(4))
        sc = Scalars()
        self._check(self.lib.chicdiff_hip_selftest_global_stage_dev(
            self.h, pbm, pdg, paz, n, int(S), int(p), o, fit.data_ptr(), resid.data_ptr(), hist, C.byref(nv), vx, vh, vf, vd, C.byref(sc)))
        k = nv.value
        return dict(dispFit=fit, resid=resid, hist=np.array(hist[:]),
                    vertices=dict(nv=k, x=np.array(vx[:k]), h=np.array(vh[:k]), f=np.array(vf[:k]), d=np.array(vd[:k])),
                    scalars=_scalars_dict(sc))

    def selftest_resid_hist(self, d_resid) -> np.ndarray:
        """TEST ENTRY: the 40 counts of hist(x[x > -10 & x < 10], breaks = -20:20/2) over a device column, by the fit's kernel."""
        pr = self._ptr("d_resid", d_resid, self.torch.float64, (-1,))
        hist = (C.c_double * 40)()
        self._check(self.lib.chicdiff_hip_selftest_resid_hist_dev(self.h, pr, d_resid.numel(), hist))
        return np.array(hist[:])

    def wald_pvalues(self, d_stat):
        ps = self._ptr("d_stat", d_stat, self.torch.float64)
        out = self.torch.empty_like(d_stat)
        self._check(self.lib.chicdiff_hip_wald_pvalues_dev(self.h, ps, d_stat.numel(), out.data_ptr()))
        return out
