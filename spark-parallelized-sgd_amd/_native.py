"""ctypes binding of libpsgd.so -- the C ABI declared in include/psgd.h.

The shared library holds the gfx950 HIP kernels; there is no CPU implementation behind this
module. If the library is missing or no gfx950 device is present, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
# PSGD_LIB: another build of the same library (diagnostics, e.g. `make -C csrc stamps`)
LIB_PATH = os.environ.get("PSGD_LIB") or os.path.join(HERE, "libpsgd.so")
CSRC = os.path.join(HERE, "csrc")

PSGD_OK, PSGD_EINVAL, PSGD_EUNSUPPORTED, PSGD_EDEVICE, PSGD_ENOMEM, PSGD_ESTATE = 0, -1, -2, -3, -4, -5
F64, F32 = 0, 1
SEED_PLUS_INDEX, SEED_PARTITIONWISE = 0, 1   # enum psgd_seeding

# Symbols include/psgd.h declares (checked by tests/test_capi_symbols.py).
EXPORTED = (
    "psgd_abi_version", "psgd_last_error", "psgd_ctx_create", "psgd_ctx_destroy",
    "psgd_register_dense", "psgd_register_csr", "psgd_register_dense_device", "psgd_register_csr_device",
    "psgd_clear_partitions", "psgd_num_partitions", "psgd_run_epoch", "psgd_run_epoch_device",
    "psgd_fold_partials_device", "psgd_run_epoch_device_mirror", "psgd_fold_partials_device_mirror",
    "psgd_convergence_terms_device", "psgd_initial_regval",
    "psgd_ctx_last_kernel", "psgd_ctx_last_ring", "psgd_ctx_last_chain_ms", "psgd_ctx_chain_launches", "psgd_ctx_chain_ms",
    "psgd_vmm_stats", "psgd_reroll_stats", "psgd_libsvm_read", "psgd_libsvm_free",
    "psgd_sample_partition", "psgd_host_alloc", "psgd_host_free", "psgd_register_wait",
    "psgd_evaluate", "psgd_evaluate_device", "psgd_predict", "psgd_predict_device",
    "psgd_column_stats", "psgd_column_stats_device", "psgd_transform_columns", "psgd_transform_columns_device",
    "psgd_gradient_sum", "psgd_gradient_sum_device", "psgd_gd_update", "psgd_gd_update_device",
    "psgd_gradient_sum_multinomial", "psgd_gradient_sum_multinomial_device", "psgd_gradient_multinomial_plan",
    "psgd_gradient_sum_multinomial_method", "psgd_gradient_sum_multinomial_method_device",
    "psgd_gradient_multinomial_plan_method",
    "psgd_gramian", "psgd_gramian_device", "psgd_gramian_plan",
    "psgd_gramian_weighted", "psgd_gramian_weighted_device", "psgd_local_rows",
    "psgd_tsqr", "psgd_tsqr_device", "psgd_tsqr_rows_device", "psgd_tsqr_plan",
    "psgd_row_curvature", "psgd_row_curvature_device",
    "psgd_project", "psgd_project_device", "psgd_project_plan",
    "psgd_kmeans_assign", "psgd_kmeans_assign_device", "psgd_kmeans_step", "psgd_kmeans_step_device",
    "psgd_kmeans_update_device", "psgd_kmeans_plan",
    "psgd_tree_bin_device", "psgd_tree_histogram_device", "psgd_tree_best_split_device", "psgd_tree_route_device",
    "psgd_tree_predict", "psgd_tree_predict_device", "psgd_tree_plan",
    "psgd_tree_label_range_device", "psgd_tree_targets_device", "psgd_tree_moments_device",
    "psgd_tree_histogram_reg_device", "psgd_tree_best_split_reg_device",
    "psgd_forest_bag_device", "psgd_forest_histogram_device", "psgd_forest_best_split_device", "psgd_forest_route_device",
    "psgd_forest_predict", "psgd_forest_predict_device", "psgd_forest_plan",
    "psgd_gmm_responsibilities", "psgd_gmm_responsibilities_device", "psgd_gmm_moments_device",
    "psgd_gmm_step", "psgd_gmm_step_device", "psgd_gmm_plan",
    "psgd_binary_counts", "psgd_binary_counts_device", "psgd_binary_counts_model", "psgd_binary_counts_model_device",
    "psgd_metrics_sort_tile",
    "psgd_evaluate_multinomial", "psgd_evaluate_multinomial_device",
    "psgd_predict_multinomial", "psgd_predict_multinomial_device",
    "psgd_confusion", "psgd_confusion_device", "psgd_confusion_model", "psgd_confusion_model_device",
    "psgd_multiclass_switches",
    "psgd_cell_select", "psgd_cell_select_device", "psgd_gather_dense_device", "psgd_gather_csr_device",
)


class psgd_libsvm(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("d", C.c_int32), ("n_parts", C.c_int32),
                ("part_offsets", C.POINTER(C.c_int64)), ("labels", C.POINTER(C.c_double)),
                ("row_ptr", C.POINTER(C.c_int64)), ("col", C.POINTER(C.c_int32)),
                ("val", C.POINTER(C.c_double))]


class IllegalArgumentException(ValueError):
    """The reference's `require` failures (java.lang.IllegalArgumentException)."""


class UnsupportedOperationException(NotImplementedError):
    """Valid in the reference but not built here yet."""


class DeviceError(RuntimeError):
    """HIP runtime failure inside libpsgd."""


class psgd_params(C.Structure):
    _fields_ = [
        ("gradient", C.c_int32), ("updater", C.c_int32), ("compute_dtype", C.c_int32),
        ("iteration", C.c_int32), ("step_size", C.c_double), ("reg_param", C.c_double),
        ("mini_batch_fraction", C.c_double), ("convergence_tol", C.c_double),
        ("adam_beta", C.c_double), ("adam_gamma", C.c_double), ("adam_eps", C.c_double),
        ("num_classes", C.c_int32),
    ]


def build(force: bool = False) -> str:
    """Compile libpsgd.so in-tree (hipcc --offload-arch=gfx950)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-s", "-C", CSRC, "-j2"], check=True)
    return LIB_PATH


_lib = None
_lock = threading.Lock()


def lib():
    """Load libpsgd.so (after torch, so both share one HIP runtime)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        try:  # torch bundles libamdhip64.so.7; load it first so there is one HIP runtime
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise DeviceError(
                f"{LIB_PATH} is missing: build it with `make -C {CSRC}` (hipcc, gfx950)")
        L = C.CDLL(LIB_PATH)
        vp, dp, i64p, i32p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        P = C.POINTER(psgd_params)
        sig = {
            "psgd_abi_version": ([], C.c_int32),
            "psgd_last_error": ([], C.c_char_p),
            "psgd_ctx_create": ([C.c_int32, C.POINTER(vp)], C.c_int32),
            "psgd_ctx_destroy": ([vp], C.c_int32),
            "psgd_register_dense": ([vp, C.c_int64, C.c_int64, C.c_int32, vp, vp, C.c_int32], C.c_int32),
            "psgd_register_csr": ([vp, C.c_int64, C.c_int64, C.c_int32, vp, vp, vp, vp, C.c_int32], C.c_int32),
            "psgd_register_dense_device": ([vp, C.c_int64, C.c_int64, C.c_int32, C.c_int64, vp, vp, C.c_int32], C.c_int32),
            "psgd_register_csr_device": ([vp, C.c_int64, C.c_int64, C.c_int32, vp, vp, vp, vp, C.c_int32], C.c_int32),
            "psgd_clear_partitions": ([vp], C.c_int32),
            "psgd_num_partitions": ([vp, i64p, i64p], C.c_int32),
            "psgd_run_epoch": ([vp, P, vp, vp, dp, dp, i64p, vp], C.c_int32),
            "psgd_run_epoch_device": ([vp, P, vp, vp, vp, vp], C.c_int32),
            "psgd_fold_partials_device": ([vp, C.c_int32, C.c_int32, vp, vp, vp], C.c_int32),
            "psgd_run_epoch_device_mirror": ([vp, P, vp, vp, vp, vp, vp], C.c_int32),
            "psgd_fold_partials_device_mirror": ([vp, C.c_int32, C.c_int32, vp, vp, vp, vp], C.c_int32),
            "psgd_convergence_terms_device": ([vp, C.c_int32, vp, vp, dp, vp], C.c_int32),
            "psgd_initial_regval": ([vp, P, C.c_int32, vp, dp], C.c_int32),
            "psgd_ctx_last_kernel": ([vp], C.c_int32),
            "psgd_ctx_last_ring": ([vp, i32p], C.c_int32),
            "psgd_ctx_last_chain_ms": ([vp, dp], C.c_int32),
            "psgd_ctx_chain_launches": ([vp], C.c_int64),
            "psgd_ctx_chain_ms": ([vp, C.c_int64, dp], C.c_int32),
            "psgd_vmm_stats": ([i64p], C.c_int32),
            "psgd_reroll_stats": ([i64p], C.c_int32),
            "psgd_libsvm_read": ([C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.POINTER(psgd_libsvm))], C.c_int32),
            "psgd_libsvm_free": ([C.POINTER(psgd_libsvm)], None),
            "psgd_sample_partition": ([C.c_int32, C.c_int64, C.c_int64, C.c_double, vp, i64p], C.c_int32),
            "psgd_host_alloc": ([vp, C.c_int64, C.POINTER(vp)], C.c_int32),
            "psgd_host_free": ([vp, vp], C.c_int32),
            "psgd_register_wait": ([vp], C.c_int32),
            "psgd_evaluate": ([vp, C.c_int32, vp, vp, vp], C.c_int32),
            "psgd_evaluate_device": ([vp, C.c_int32, vp, vp, vp, vp], C.c_int32),
            "psgd_predict": ([vp, C.c_int64, vp, vp], C.c_int32),
            "psgd_predict_device": ([vp, C.c_int64, vp, vp, vp], C.c_int32),
            "psgd_column_stats": ([vp, vp], C.c_int32),
            "psgd_column_stats_device": ([vp, vp, vp], C.c_int32),
            "psgd_transform_columns": ([vp, vp, vp], C.c_int32),
            "psgd_transform_columns_device": ([vp, vp, vp, vp], C.c_int32),
            "psgd_gradient_sum": ([vp, C.c_int32, vp, C.c_double, C.c_int32, vp], C.c_int32),
            "psgd_gradient_sum_device": ([vp, C.c_int32, vp, C.c_double, C.c_int32, vp, vp], C.c_int32),
            "psgd_gradient_sum_multinomial": ([vp, C.c_int32, vp, C.c_double, C.c_int32, vp], C.c_int32),
            "psgd_gradient_sum_multinomial_device": ([vp, C.c_int32, vp, C.c_double, C.c_int32, vp, vp], C.c_int32),
            "psgd_gradient_multinomial_plan": ([C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, vp], C.c_int32),
            "psgd_gradient_sum_multinomial_method": ([vp, C.c_int32, vp, C.c_double, C.c_int32, C.c_int32, vp], C.c_int32),
            "psgd_gradient_sum_multinomial_method_device": ([vp, C.c_int32, vp, C.c_double, C.c_int32, C.c_int32, vp, vp],
                                                            C.c_int32),
            "psgd_gradient_multinomial_plan_method": ([C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32,
                                                       vp], C.c_int32),
            "psgd_gramian": ([vp, vp], C.c_int32),
            "psgd_gramian_device": ([vp, vp, vp], C.c_int32),
            "psgd_gramian_plan": ([C.c_int32, C.c_int32, C.c_int32, C.c_int64, vp], C.c_int32),
            "psgd_gramian_weighted": ([vp, vp, vp], C.c_int32),
            "psgd_gramian_weighted_device": ([vp, vp, vp, vp], C.c_int32),
            "psgd_tsqr": ([vp, vp], C.c_int32),
            "psgd_tsqr_device": ([vp, vp, vp], C.c_int32),
            "psgd_tsqr_rows_device": ([vp, vp, C.c_int64, C.c_int32, vp, vp], C.c_int32),
            "psgd_tsqr_plan": ([C.c_int32, C.c_int32, C.c_int64, vp], C.c_int32),
            "psgd_local_rows": ([vp, vp], C.c_int32),
            "psgd_row_curvature": ([vp, C.c_int32, vp, vp], C.c_int32),
            "psgd_row_curvature_device": ([vp, C.c_int32, vp, vp, vp], C.c_int32),
            "psgd_project": ([vp, C.c_int64, C.c_int32, vp, vp], C.c_int32),
            "psgd_project_device": ([vp, C.c_int32, vp, C.c_int32, C.c_int64, vp, vp, vp], C.c_int32),
            "psgd_project_plan": ([C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, vp], C.c_int32),
            "psgd_kmeans_assign": ([vp, C.c_int32, vp, vp, vp], C.c_int32),
            "psgd_kmeans_assign_device": ([vp, C.c_int32, vp, vp, vp, vp], C.c_int32),
            "psgd_kmeans_step": ([vp, C.c_int32, vp, vp], C.c_int32),
            "psgd_kmeans_step_device": ([vp, C.c_int32, vp, vp, vp], C.c_int32),
            "psgd_kmeans_update_device": ([vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp], C.c_int32),
            "psgd_kmeans_plan": ([C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, vp], C.c_int32),
            "psgd_tree_bin_device": ([vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp], C.c_int32),
            "psgd_tree_histogram_device": ([vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp,
                                            vp], C.c_int32),
            "psgd_tree_best_split_device": ([vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int64, C.c_double, vp, vp], C.c_int32),
            "psgd_tree_route_device": ([vp, vp, vp, C.c_int32, vp, vp], C.c_int32),
            "psgd_tree_predict": ([vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int32),
            "psgd_tree_predict_device": ([vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int32),
            "psgd_tree_plan": ([C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, vp], C.c_int32),
            "psgd_tree_label_range_device": ([vp, vp, vp, vp], C.c_int32),
            "psgd_tree_targets_device": ([vp, vp, C.c_double, C.c_int32, vp, vp], C.c_int32),
            "psgd_tree_moments_device": ([vp, vp, vp, C.c_int32, C.c_int32, vp, vp], C.c_int32),
            "psgd_tree_histogram_reg_device": ([vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp], C.c_int32),
            "psgd_tree_best_split_reg_device": ([vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                                 C.c_double, vp, vp], C.c_int32),
            "psgd_forest_bag_device": ([vp, C.c_uint64, vp, C.c_int64, C.c_int32, C.c_int32, vp, vp], C.c_int32),
            "psgd_forest_histogram_device": ([vp, vp, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_int32, C.c_int32, C.c_uint64, vp, C.c_int64, C.c_int32, vp, vp,
                                              vp], C.c_int32),
            "psgd_forest_best_split_device": ([vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_int64, C.c_double, vp, vp], C.c_int32),
            "psgd_forest_route_device": ([vp, vp, vp, vp, C.c_int32, vp, vp], C.c_int32),
            "psgd_forest_predict": ([vp, C.c_int32, vp, vp, vp, vp, vp, vp, C.c_int32, vp, vp], C.c_int32),
            "psgd_forest_predict_device": ([vp, C.c_int32, vp, vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp], C.c_int32),
            "psgd_forest_plan": ([C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                  C.c_int64, C.c_int64, vp], C.c_int32),
            "psgd_gmm_responsibilities": ([vp, C.c_int32, vp, vp, vp, vp, vp, vp], C.c_int32),
            "psgd_gmm_responsibilities_device": ([vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp], C.c_int32),
            "psgd_gmm_moments_device": ([vp, C.c_int32, vp, vp, vp], C.c_int32),
            "psgd_gmm_step": ([vp, C.c_int32, vp, vp, vp, vp], C.c_int32),
            "psgd_gmm_step_device": ([vp, C.c_int32, vp, vp, vp, vp, vp], C.c_int32),
            "psgd_gmm_plan": ([C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, vp], C.c_int32),
            "psgd_gd_update": ([vp, C.c_int32, C.c_int32, vp, vp, C.c_double, C.c_int32, C.c_double, vp, dp],
                               C.c_int32),
            "psgd_gd_update_device": ([vp, C.c_int32, C.c_int32, vp, vp, C.c_double, C.c_int32, C.c_double, vp, vp,
                                       vp], C.c_int32),
            "psgd_binary_counts": ([vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp], C.c_int32),
            "psgd_binary_counts_device": ([vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp], C.c_int32),
            "psgd_binary_counts_model": ([vp, vp, vp, vp, vp, vp, vp], C.c_int32),
            "psgd_binary_counts_model_device": ([vp, vp, vp, vp, vp, vp, vp, vp], C.c_int32),
            "psgd_metrics_sort_tile": ([], C.c_int32),
            "psgd_evaluate_multinomial": ([vp, C.c_int32, vp, vp, vp], C.c_int32),
            "psgd_evaluate_multinomial_device": ([vp, C.c_int32, vp, vp, vp, vp], C.c_int32),
            "psgd_predict_multinomial": ([vp, C.c_int64, C.c_int32, vp, vp, vp], C.c_int32),
            "psgd_predict_multinomial_device": ([vp, C.c_int64, C.c_int32, vp, vp, vp, vp], C.c_int32),
            "psgd_confusion": ([vp, vp, vp, C.c_int64, C.c_int32, vp, vp], C.c_int32),
            "psgd_confusion_device": ([vp, vp, vp, C.c_int64, C.c_int32, vp, vp, vp], C.c_int32),
            "psgd_confusion_model": ([vp, C.c_int32, vp, vp, vp], C.c_int32),
            "psgd_confusion_model_device": ([vp, C.c_int32, vp, vp, vp, vp], C.c_int32),
            "psgd_multiclass_switches": ([i32p], C.c_int32),
            "psgd_cell_select": ([vp, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_int32, vp, vp, vp], C.c_int32),
            "psgd_cell_select_device": ([vp, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_int32, vp, vp, vp, vp],
                                        C.c_int32),
            "psgd_gather_dense_device": ([vp, vp, vp, C.c_int64, vp, vp, vp], C.c_int32),
            "psgd_gather_csr_device": ([vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int32),
        }
        for name, (args, res) in sig.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
        _lib = L
        return L


def check(rc: int) -> None:
    if rc == PSGD_OK:
        return
    msg = lib().psgd_last_error().decode(errors="replace")
    if rc == PSGD_EINVAL:
        raise IllegalArgumentException(msg)
    if rc == PSGD_EUNSUPPORTED:
        raise UnsupportedOperationException(msg)
    raise DeviceError(f"libpsgd error {rc}: {msg}")


def vmm_stats() -> dict:
    """Process-wide counters of the CSR weight vectors' virtual-memory mappings (psgd_vmm_stats)."""
    out = (C.c_int64 * 4)()
    check(lib().psgd_vmm_stats(out))
    return {"mapped": out[0], "unmapped": out[1], "live_bytes": out[2], "failures": out[3]}


def reroll_stats() -> dict:
    """Process-wide counters of the CSR vector sets' placement re-roll (psgd_reroll_stats)."""
    out = (C.c_int64 * 2)()
    check(lib().psgd_reroll_stats(out))
    return {"sets": out[0], "swaps": out[1]}


def sample_partition(seed: int, n: int, fraction: float, device: int = 0):
    """Row indices RDD.sample(false, fraction, .) keeps from an n-row partition whose sampler
    seed is `seed`, selected on the device (psgd_sample_partition)."""
    import numpy as np
    rows = np.empty(max(int(n), 1), dtype=np.int32)
    m = C.c_int64()
    check(lib().psgd_sample_partition(device, int(seed), int(n), float(fraction), rows.ctypes.data,
                                      C.byref(m)))
    return rows[: m.value].copy()


def metrics_sort_tile() -> int:
    """The pairs one workgroup of the metrics kernels takes (psgd_metrics_sort_tile)."""
    return int(lib().psgd_metrics_sort_tile())


def multiclass_switches() -> dict:
    """The sizes at which the multiclass kernels change path (psgd_multiclass_switches): the doubles
    of class blocks kept in LDS, the largest K - 1 whose softmax one lane takes, the largest K * K of
    the confusion table kept in LDS."""
    out = (C.c_int32 * 3)()
    check(lib().psgd_multiclass_switches(out))
    return {"lds_weights": int(out[0]), "lane_classes": int(out[1]), "confusion_lds_cells": int(out[2])}


MN_GRAD_PATHS = ("fused", "general", "csr_lds", "csr_global", "mfma")   # psgd_gradient_multinomial_plan's out[0]
MN_METHODS = {"auto": 0, "mfma": 1}   # PSGD_MN_METHOD_*


def mn_method(method: str) -> int:
    """"auto" (the plan's own choice of the fused, general and CSR kernels) or "mfma" (the fp64
    matrix-core path: dense rows, numClasses <= 65, d <= 4,096) -> PSGD_MN_METHOD_*."""
    if method not in MN_METHODS:
        raise IllegalArgumentException(f"unknown multinomial gradient method {method!r}: 'auto' or 'mfma'")
    return MN_METHODS[method]


def gradient_multinomial_plan(layout: str, storage: str, d: int, num_classes: int, max_nnz: int = 0,
                              method: str = "auto") -> dict:
    """Which kernels psgd_gradient_sum_multinomial_method runs for rows of `layout` ("dense" / "csr")
    stored as `storage` ("f32" / "f64"), with the environment switches as they are now
    (psgd_gradient_multinomial_plan_method: host code, no device). The "mfma" plan has keys of its own:
    the class blocks of 16, the packed W's features, the accumulation pass's rectangle."""
    out = (C.c_int32 * 12)()
    check(lib().psgd_gradient_multinomial_plan_method({"dense": 0, "csr": 1}[layout], {"f64": 0, "f32": 1}[storage],
                                                      int(d), int(num_classes), int(max_nnz), mn_method(method), out))
    keys = ("path", "group", "weights_in_lds", "wide_softmax", "tile_rows", "nvl", "class_accumulators",
            "acc_group", "col_chunks", "class_chunks", "span", "range")
    if MN_GRAD_PATHS[out[0]] == "mfma":
        keys = ("path", "class_blocks", "weights_in_lds", "wide_softmax", "tile_rows", "dpad", "rect_class_blocks",
                "rect_feature_blocks", "col_chunks", "class_chunks", "span", "range")
    plan = {k: int(v) for k, v in zip(keys, out)}
    plan["path"] = MN_GRAD_PATHS[plan["path"]]
    return plan


GRAMIAN_MAX_D = 4096   # PSGD_GRAMIAN_MAX_D
PROJECT_MAX_K = 256    # PSGD_PROJECT_MAX_K
PROJECT_PATHS = ("dense_lds", "dense_l2", "csr_lds", "csr_l2")


def project_plan(layout: str, storage: str, d: int, k: int, max_nnz: int = 0) -> dict:
    """How psgd_project runs rows of `layout` ("dense" / "csr") stored as `storage` ("f32" / "f64")
    with d features against k components (psgd_project_plan: host code, no device)."""
    out = (C.c_int64 * 8)()
    check(lib().psgd_project_plan({"dense": 0, "csr": 1}[layout], {"f64": 0, "f32": 1}[storage], int(d), int(k),
                                  int(max_nnz), out))
    keys = ("path", "kpad", "rows_wave", "comp_blocks", "feature_chunk", "lds_bytes", "scratch_bytes", "row_lanes")
    plan = {k_: int(v) for k_, v in zip(keys, out)}
    plan["path"] = PROJECT_PATHS[plan["path"]]
    return plan


KMEANS_MAX_K = 256     # PSGD_KMEANS_MAX_K
KMEANS_PATHS = ("dense_lds", "dense_l2", "csr_lds_sums", "csr_global_sums")


def kmeans_plan(layout: str, storage: str, d: int, k: int, total_tiles: int) -> dict:
    """How the k-means passes run rows of `layout` ("dense" / "csr") stored as `storage` ("f32" / "f64")
    with d features against k centres, cut into total_tiles tiles (psgd_kmeans_plan: host code, no device)."""
    out = (C.c_int64 * 12)()
    check(lib().psgd_kmeans_plan({"dense": 0, "csr": 1}[layout], {"f64": 0, "f32": 1}[storage], int(d), int(k),
                                 int(total_tiles), out))
    keys = ("path", "centre_blocks", "gr", "gc", "span_tiles", "spans", "items", "scratch_bytes", "lds_bytes",
            "tile_rows", "kpad", "row_lanes")
    plan = {k_: int(v) for k_, v in zip(keys, out)}
    plan["path"] = KMEANS_PATHS[plan["path"]]
    return plan


TREE_MAX_BINS = 256       # PSGD_TREE_MAX_BINS
TREE_MAX_CLASSES = 32     # PSGD_TREE_MAX_CLASSES
TREE_IMPURITIES = {"gini": 0, "entropy": 1}   # PSGD_TREE_GINI / PSGD_TREE_ENTROPY


def tree_plan(storage: str, d: int, maxBins: int, K: int, slots: int, total_tiles: int, budget: int = 0) -> dict:
    """How a level's histogram pass runs a frontier of `slots` slots over rows of d features cut into
    total_tiles tiles of 256 rows, the 64-bit table of a launch within `budget` bytes (0: 256 MiB)
    (psgd_tree_plan: host code, no device)."""
    out = (C.c_int64 * 10)()
    check(lib().psgd_tree_plan({"f64": 0, "f32": 1}[storage], int(d), int(maxBins), int(K), int(slots), int(total_tiles),
                               int(budget), out))
    keys = ("feature_chunk", "slot_subgroup", "replication", "lds_bytes", "groups", "scratch_bytes", "group_slots",
            "items", "span_rows", "pitch")
    return {k_: int(v) for k_, v in zip(keys, out)}


def forest_plan(d: int, maxBins: int, K: int, m: int, nodes: int, numTrees: int, total_tiles: int, n_rows: int,
                scratchBudget: int = 0, slotBudget: int = 0) -> dict:
    """How a level's forest histogram pass runs a frontier of `nodes` nodes with m subset features each, and how
    many of numTrees trees train together over n_rows local rows (psgd_forest_plan: host code, no device)."""
    out = (C.c_int64 * 11)()
    check(lib().psgd_forest_plan(int(d), int(maxBins), int(K), int(m), int(nodes), int(numTrees), int(total_tiles),
                                 int(n_rows), int(scratchBudget), int(slotBudget), out))
    keys = ("subset_chunk", "node_subgroup", "lds_bytes", "groups", "scratch_bytes", "group_nodes", "items", "span_rows",
            "group_trees", "tile_rows", "pitch")
    return {k_: int(v) for k_, v in zip(keys, out)}


GMM_MAX_K = 256     # PSGD_GMM_MAX_K
GMM_MAX_D = 256     # PSGD_GMM_MAX_D
GMM_PATHS = ("dense_lds", "dense_l2")


def gmm_plan(layout: str, storage: str, d: int, k: int, total_tiles: int) -> dict:
    """How the Gaussian mixture's passes run rows of `layout` ("dense"; "csr" is refused) stored as `storage`
    ("f32" / "f64") with d features against k components, cut into total_tiles tiles (psgd_gmm_plan: host
    code, no device)."""
    out = (C.c_int64 * 13)()
    check(lib().psgd_gmm_plan({"dense": 0, "csr": 1}[layout], {"f64": 0, "f32": 1}[storage], int(d), int(k),
                              int(total_tiles), out))
    keys = ("path", "chunk_blocks", "component_blocks", "gr", "gc", "span_tiles", "spans", "items", "scratch_bytes",
            "scratch_bytes_with_resp", "lds_bytes", "tile_rows", "waves")
    plan = {k_: int(v) for k_, v in zip(keys, out)}
    plan["path"] = GMM_PATHS[plan["path"]]
    return plan


def gramian_plan(layout: str, storage: str, d: int, total_tiles: int) -> dict:
    """How psgd_gramian runs rows of `layout` ("dense" / "csr") stored as `storage` ("f32" / "f64")
    with d features cut into total_tiles tiles (psgd_gramian_plan: host code, no device)."""
    out = (C.c_int64 * 10)()
    check(lib().psgd_gramian_plan({"dense": 0, "csr": 1}[layout], {"f64": 0, "f32": 1}[storage], int(d),
                                  int(total_tiles), out))
    keys = ("path", "a", "blocks", "gr", "gc", "groups", "span_tiles", "spans", "scratch_bytes", "tile_rows")
    plan = {k: int(v) for k, v in zip(keys, out)}
    plan["path"] = ("dense_mfma", "csr")[plan["path"]]
    return plan


TSQR_MAX_D = 127   # PSGD_TSQR_MAX_D


def tsqr_plan(storage: str, d: int, total_tiles: int) -> dict:
    """How psgd_tsqr runs dense rows stored as `storage` ("f32" / "f64") with d features cut into
    total_tiles tiles (psgd_tsqr_plan: host code, no device)."""
    out = (C.c_int64 * 10)()
    check(lib().psgd_tsqr_plan({"f64": 0, "f32": 1}[storage], int(d), int(total_tiles), out))
    keys = ("a", "a_pad", "items", "span_tiles", "panel_rows", "fan_in", "levels", "lds_bytes", "scratch_bytes",
            "tile_rows")
    return {k: int(v) for k, v in zip(keys, out)}


class _PinnedBuffer:
    """Page-locked host memory from psgd_host_alloc; freed when the last numpy view of it goes
    (the context must outlive it)."""

    def __init__(self, ctx, addr, nbytes):
        self._ctx, self._addr = ctx, addr
        self.view = (C.c_char * nbytes).from_address(addr)
        self.view.owner = self      # numpy views keep the ctypes array, which keeps this

    def __del__(self):
        try:
            if self._ctx.handle and self._addr:
                self._ctx._L.psgd_host_free(self._ctx.handle, self._addr)
        except Exception:
            pass
        self._addr = None


class Context:
    """Owns one psgd_ctx (one device, its stream, registry and buffers)."""

    def __init__(self, device: int = 0):
        self._L = lib()
        h = C.c_void_p()
        check(self._L.psgd_ctx_create(device, C.byref(h)))
        self.handle = h
        self.device = device

    def close(self):
        if self.handle:
            self._L.psgd_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # registry -------------------------------------------------------------------------------
    def register_dense(self, part, labels, x):
        import numpy as np
        labels = np.ascontiguousarray(labels, dtype=np.float64)
        if x.dtype not in (np.float32, np.float64):
            x = x.astype(np.float64)
        x = np.ascontiguousarray(x)
        n, d = x.shape
        dt = F32 if x.dtype == np.float32 else F64
        check(self._L.psgd_register_dense(self.handle, part, n, d, labels.ctypes.data,
                                          x.ctypes.data, dt))

    def register_csr(self, part, labels, row_ptr, col, val, d):
        import numpy as np
        labels = np.ascontiguousarray(labels, dtype=np.float64)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=np.int32)
        if val.dtype not in (np.float32, np.float64):
            val = val.astype(np.float64)
        val = np.ascontiguousarray(val)
        dt = F32 if val.dtype == np.float32 else F64
        check(self._L.psgd_register_csr(self.handle, part, len(labels), d, labels.ctypes.data,
                                        row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data, dt))

    def register_dense_device(self, part, n_rows, d, ld, labels_ptr, x_ptr, dtype):
        check(self._L.psgd_register_dense_device(self.handle, part, n_rows, d, ld, labels_ptr,
                                                 x_ptr, dtype))

    def register_csr_device(self, part, n_rows, d, labels_ptr, row_ptr_ptr, col_ptr, val_ptr, dtype):
        check(self._L.psgd_register_csr_device(self.handle, part, n_rows, d, labels_ptr, row_ptr_ptr,
                                               col_ptr, val_ptr, dtype))

    def register_wait(self):
        """Block until every registration copy has landed in HBM (psgd_register_wait)."""
        check(self._L.psgd_register_wait(self.handle))

    def host_array(self, shape, dtype):
        """A numpy array over page-locked host memory (psgd_host_alloc): registration from it is
        one direct DMA, no staging copy. Freed with the returned array's owner (`.base`)."""
        import numpy as np
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        p = C.c_void_p()
        check(self._L.psgd_host_alloc(self.handle, max(n, 1), C.byref(p)))
        buf = _PinnedBuffer(self, p.value, max(n, 1))
        return np.frombuffer(buf.view, dtype=dt, count=int(np.prod(shape))).reshape(shape)

    def clear(self):
        check(self._L.psgd_clear_partitions(self.handle))

    def num_partitions(self):
        a, b = C.c_int64(), C.c_int64()
        check(self._L.psgd_num_partitions(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_kernel(self) -> int:
        return int(self._L.psgd_ctx_last_kernel(self.handle))

    def last_ring(self):
        """(R, MB, D, GS) of the LDS row ring of the last chain launch: row slots, meta blocks,
        loader depth, Gram slots; zeros when the last kernel has no ring."""
        out = (C.c_int32 * 4)()
        check(self._L.psgd_ctx_last_ring(self.handle, out))
        return tuple(int(v) for v in out)

    def last_chain_ms(self) -> float:
        """Device time of the last chain-kernel launch (HIP events on its stream)."""
        ms = C.c_double()
        check(self._L.psgd_ctx_last_chain_ms(self.handle, C.byref(ms)))
        return ms.value

    def chain_launches(self) -> int:
        """Chain-kernel launches this context has made (the index of the next one)."""
        return int(self._L.psgd_ctx_chain_launches(self.handle))

    def chain_ms(self, launch: int) -> float:
        """Device time of chain-kernel launch `launch` (0-based; one of the last 64)."""
        ms = C.c_double()
        check(self._L.psgd_ctx_chain_ms(self.handle, C.c_int64(launch), C.byref(ms)))
        return ms.value

    # epochs ---------------------------------------------------------------------------------
    def run_epoch_device(self, params, w_ptr, partial_ptr, counts_ptr=None, stream=None):
        check(self._L.psgd_run_epoch_device(self.handle, C.byref(params), w_ptr, partial_ptr,
                                            counts_ptr, stream))

    def fold_partials_device(self, n, d, partials_ptr, out_ptr, stream=None):
        check(self._L.psgd_fold_partials_device(self.handle, n, d, partials_ptr, out_ptr, stream))

    def run_epoch_device_mirror(self, params, w_ptr, partial_ptr, counts_ptr, stream, h_ptr):
        """run_epoch_device whose fold also writes {regVal, lossSum, count} to h_ptr[3]
        (page-locked host memory, host_array)."""
        check(self._L.psgd_run_epoch_device_mirror(self.handle, C.byref(params), w_ptr, partial_ptr,
                                                   counts_ptr, stream, h_ptr))

    def fold_partials_device_mirror(self, n, d, partials_ptr, out_ptr, stream, h_ptr):
        check(self._L.psgd_fold_partials_device_mirror(self.handle, n, d, partials_ptr, out_ptr, stream,
                                                       h_ptr))

    def convergence_terms_device(self, d, prev_ptr, cur_ptr, stream=None):
        out = (C.c_double * 2)()
        check(self._L.psgd_convergence_terms_device(self.handle, d, prev_ptr, cur_ptr, out, stream))
        return out[0], out[1]

    def initial_regval(self, params, w):
        import numpy as np
        w = np.ascontiguousarray(w, dtype=np.float64)
        out = C.c_double()
        check(self._L.psgd_initial_regval(self.handle, C.byref(params), len(w), w.ctypes.data,
                                          C.byref(out)))
        return out.value

    def run_epoch(self, params, w_in):
        """Host-pointer form (the JNI-shaped call): returns (w, regVal, lossSum, count, counts)."""
        import numpy as np
        w_in = np.ascontiguousarray(w_in, dtype=np.float64)
        nparts, _ = self.num_partitions()
        w_out = np.zeros_like(w_in)
        rv, loss = C.c_double(), C.c_double()
        cnt = C.c_int64()
        counts = np.zeros(max(nparts, 1), dtype=np.int64)
        check(self._L.psgd_run_epoch(self.handle, C.byref(params), w_in.ctypes.data,
                                     w_out.ctypes.data, C.byref(rv), C.byref(loss), C.byref(cnt),
                                     counts.ctypes.data))
        return w_out, rv.value, loss.value, cnt.value, counts[:nparts]

    # scoring at fixed weights -----------------------------------------------------------------
    def evaluate(self, gradient: int, w):
        """Host-pointer form (psgd_evaluate): (lossSum, count, nCorrect, partLoss, partCorrect)
        of host weights w over every registered partition."""
        import numpy as np
        w = np.ascontiguousarray(w, dtype=np.float64)
        nparts, _ = self.num_partitions()
        out3 = np.zeros(3, dtype=np.float64)
        part = np.zeros((max(nparts, 1), 2), dtype=np.float64)
        check(self._L.psgd_evaluate(self.handle, int(gradient), w.ctypes.data, out3.ctypes.data,
                                    part.ctypes.data))
        return float(out3[0]), int(out3[1]), int(out3[2]), part[:nparts, 0].copy(), part[:nparts, 1].copy()

    def evaluate_device(self, gradient: int, w_ptr, out3_ptr, part_ptr=None, stream=None):
        """psgd_evaluate_device: enqueued on `stream`; out3[3] and part[n_parts * 2] on the device."""
        check(self._L.psgd_evaluate_device(self.handle, int(gradient), w_ptr, out3_ptr, part_ptr, stream))

    def predict(self, part: int, n_rows: int, w):
        """Host-pointer form (psgd_predict): the dots x_r . w of partition `part`'s n_rows rows."""
        import numpy as np
        w = np.ascontiguousarray(w, dtype=np.float64)
        out = np.zeros(int(n_rows), dtype=np.float64)
        check(self._L.psgd_predict(self.handle, C.c_int64(part), w.ctypes.data, out.ctypes.data))
        return out

    def predict_device(self, part: int, w_ptr, margins_ptr, stream=None):
        check(self._L.psgd_predict_device(self.handle, C.c_int64(part), w_ptr, margins_ptr, stream))

    # scoring a multinomial logistic model ----------------------------------------------------------
    def evaluate_multinomial(self, num_classes: int, w):
        """Host-pointer form (psgd_evaluate_multinomial): (lossSum, count, nCorrect, partLoss,
        partCorrect) of the (K - 1) d host weights w over every registered partition."""
        import numpy as np
        w = np.ascontiguousarray(w, dtype=np.float64)
        nparts, _ = self.num_partitions()
        out3 = np.zeros(3, dtype=np.float64)
        part = np.zeros((max(nparts, 1), 2), dtype=np.float64)
        check(self._L.psgd_evaluate_multinomial(self.handle, int(num_classes), w.ctypes.data, out3.ctypes.data,
                                                part.ctypes.data))
        return float(out3[0]), int(out3[1]), int(out3[2]), part[:nparts, 0].copy(), part[:nparts, 1].copy()

    def evaluate_multinomial_device(self, num_classes: int, w_ptr, out3_ptr, part_ptr=None, stream=None):
        check(self._L.psgd_evaluate_multinomial_device(self.handle, int(num_classes), w_ptr, out3_ptr, part_ptr,
                                                       stream))

    def predict_multinomial(self, part: int, n_rows: int, num_classes: int, w):
        """Host-pointer form (psgd_predict_multinomial): (classes[n_rows], margins[n_rows, K - 1])."""
        import numpy as np
        w = np.ascontiguousarray(w, dtype=np.float64)
        classes = np.zeros(int(n_rows), dtype=np.float64)
        margins = np.zeros((int(n_rows), int(num_classes) - 1), dtype=np.float64)
        check(self._L.psgd_predict_multinomial(self.handle, C.c_int64(part), int(num_classes), w.ctypes.data,
                                               classes.ctypes.data, margins.ctypes.data))
        return classes, margins

    def predict_multinomial_device(self, part: int, num_classes: int, w_ptr, classes_ptr, margins_ptr=None,
                                   stream=None):
        check(self._L.psgd_predict_multinomial_device(self.handle, C.c_int64(part), int(num_classes), w_ptr,
                                                      classes_ptr, margins_ptr, stream))

    def confusion(self, predictions, labels, num_classes: int):
        """Host-pointer form (psgd_confusion): (counts[K, K] int64, n_bad)."""
        import numpy as np
        predictions = np.ascontiguousarray(predictions, dtype=np.float64)
        labels = np.ascontiguousarray(labels, dtype=np.float64)
        K = int(num_classes)
        counts = np.zeros((max(K, 1), max(K, 1)), dtype=np.int64)
        bad = C.c_int64()
        check(self._L.psgd_confusion(self.handle, predictions.ctypes.data, labels.ctypes.data,
                                     C.c_int64(predictions.shape[0]), K, counts.ctypes.data, C.byref(bad)))
        return counts, int(bad.value)

    def confusion_device(self, predictions_ptr, labels_ptr, n: int, num_classes: int, counts_ptr, n_bad_ptr,
                         stream=None):
        check(self._L.psgd_confusion_device(self.handle, predictions_ptr, labels_ptr, C.c_int64(n), int(num_classes),
                                            counts_ptr, n_bad_ptr, stream))

    def confusion_model(self, num_classes: int, w):
        """Host-pointer form (psgd_confusion_model): (counts[K, K] int64, n_bad) of every registered row."""
        import numpy as np
        w = np.ascontiguousarray(w, dtype=np.float64)
        K = int(num_classes)
        counts = np.zeros((max(K, 1), max(K, 1)), dtype=np.int64)
        bad = C.c_int64()
        check(self._L.psgd_confusion_model(self.handle, K, w.ctypes.data, counts.ctypes.data, C.byref(bad)))
        return counts, int(bad.value)

    def confusion_model_device(self, num_classes: int, w_ptr, counts_ptr, n_bad_ptr, stream=None):
        check(self._L.psgd_confusion_model_device(self.handle, int(num_classes), w_ptr, counts_ptr, n_bad_ptr, stream))

    # column statistics and the column transform -------------------------------------------------
    def column_stats(self, d: int):
        """Host-pointer form (psgd_column_stats): the 1 + 5 d doubles
        {count, mean[d], m2[d], numNonzeros[d], max[d], min[d]} over every registered row."""
        import numpy as np
        out = np.zeros(1 + 5 * int(d), dtype=np.float64)
        check(self._L.psgd_column_stats(self.handle, out.ctypes.data))
        return out

    def column_stats_device(self, out_ptr, stream=None):
        """psgd_column_stats_device: enqueued on `stream`; out[1 + 5 d] on the device."""
        check(self._L.psgd_column_stats_device(self.handle, out_ptr, stream))

    # the augmented Gramian ----------------------------------------------------------------------
    def gramian(self, d: int):
        """Host-pointer form (psgd_gramian): M = sum z z^T, z = [x, y, 1], as a (d + 2, d + 2) array."""
        import numpy as np
        a = int(d) + 2
        out = np.zeros((a, a), dtype=np.float64)
        check(self._L.psgd_gramian(self.handle, out.ctypes.data))
        return out

    def gramian_device(self, out_ptr, stream=None):
        """psgd_gramian_device: enqueued on `stream`; out[(d + 2)^2] on the device."""
        check(self._L.psgd_gramian_device(self.handle, out_ptr, stream))

    def local_rows(self) -> int:
        """psgd_local_rows: the registered rows, the length of the per-row arrays below."""
        n = C.c_int64()
        check(self._L.psgd_local_rows(self.handle, C.byref(n)))
        return int(n.value)

    # the tall-skinny QR ---------------------------------------------------------------------------
    def tsqr(self, d: int):
        """Host-pointer form (psgd_tsqr): the upper-triangular R of Z = [x, y] as a (d + 1, d + 1) array."""
        import numpy as np
        a = int(d) + 1
        out = np.empty((a, a), dtype=np.float64)
        check(self._L.psgd_tsqr(self.handle, out.ctypes.data))
        return out

    def tsqr_device(self, out_ptr, stream=None):
        """psgd_tsqr_device: enqueued on `stream`; out[(d + 1)^2] on the device."""
        check(self._L.psgd_tsqr_device(self.handle, out_ptr, stream))

    def tsqr_rows_device(self, rows_ptr, n: int, a: int, out_ptr, stream=None):
        """psgd_tsqr_rows_device: the R of rows[n, a] (f64, on the device) into out[a^2]."""
        check(self._L.psgd_tsqr_rows_device(self.handle, rows_ptr, int(n), int(a), out_ptr, stream))

    def gramian_weighted(self, d: int, omega):
        """Host-pointer form (psgd_gramian_weighted): M_w = sum omega_i z_i z_i^T, omega one double per
        registered row in local row order."""
        import numpy as np
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        if omega.ndim != 1 or omega.shape[0] != self.local_rows():
            raise IllegalArgumentException(
                f"requirement failed: the weighted Gramian takes one weight per registered row "
                f"({self.local_rows()}; got shape {omega.shape})")
        a = int(d) + 2
        out = np.zeros((a, a), dtype=np.float64)
        check(self._L.psgd_gramian_weighted(self.handle, omega.ctypes.data, out.ctypes.data))
        return out

    def gramian_weighted_device(self, omega_ptr, out_ptr, stream=None):
        """psgd_gramian_weighted_device: enqueued on `stream`; omega[local rows], out[(d + 2)^2] on the device."""
        check(self._L.psgd_gramian_weighted_device(self.handle, omega_ptr, out_ptr, stream))

    # the rows' curvature ------------------------------------------------------------------------
    def row_curvature(self, gradient: int, w):
        """Host-pointer form (psgd_row_curvature): d^2 loss / d(x . w)^2 of every registered row."""
        import numpy as np
        w = np.ascontiguousarray(w, dtype=np.float64)
        out = np.zeros(max(self.local_rows(), 1), dtype=np.float64)
        check(self._L.psgd_row_curvature(self.handle, int(gradient), w.ctypes.data, out.ctypes.data))
        return out[: self.local_rows()]

    def row_curvature_device(self, gradient: int, w_ptr, out_ptr, stream=None):
        """psgd_row_curvature_device: enqueued on `stream`; out[local rows] on the device."""
        check(self._L.psgd_row_curvature_device(self.handle, int(gradient), w_ptr, out_ptr, stream))

    # the row projection -------------------------------------------------------------------------
    def project(self, part: int, n_rows: int, B):
        """Host-pointer form (psgd_project): partition `part`'s rows times B [d, k] as an (n_rows, k)
        float64 array."""
        import numpy as np
        B = np.ascontiguousarray(B, dtype=np.float64)
        out = np.zeros((int(n_rows), B.shape[1]), dtype=np.float64)
        check(self._L.psgd_project(self.handle, int(part), int(B.shape[1]), B.ctypes.data, out.ctypes.data))
        return out

    def project_device(self, k: int, b_ptr, out_storage: int, ld_out: int, y_ptrs, label_ptrs, stream=None):
        """psgd_project_device: y_ptrs / label_ptrs the per-partition device addresses (0 where a
        partition is empty), in partition-index order."""
        import numpy as np
        ys = np.ascontiguousarray(y_ptrs, dtype=np.uint64)
        ls = np.ascontiguousarray(label_ptrs, dtype=np.uint64)
        check(self._L.psgd_project_device(self.handle, int(k), b_ptr, int(out_storage), int(ld_out), ys.ctypes.data,
                                          ls.ctypes.data, stream))

    # k-means ------------------------------------------------------------------------------------
    def kmeans_assign(self, centres, distances: bool = False):
        """Host-pointer form (psgd_kmeans_assign): (assign int32 [local rows], dist2 or None)."""
        import numpy as np
        c = np.ascontiguousarray(centres, dtype=np.float64)
        n = self.local_rows()
        assign = np.zeros(max(n, 1), dtype=np.int32)
        dist2 = np.zeros(max(n, 1), dtype=np.float64) if distances else None
        check(self._L.psgd_kmeans_assign(self.handle, int(c.shape[0]), c.ctypes.data, assign.ctypes.data,
                                         None if dist2 is None else dist2.ctypes.data))
        return assign[:n], None if dist2 is None else dist2[:n]

    def kmeans_assign_device(self, k: int, c_ptr, assign_ptr, dist2_ptr, stream=None):
        """psgd_kmeans_assign_device: enqueued on `stream`; assign / dist2 (0: none) [local rows] on the device."""
        check(self._L.psgd_kmeans_assign_device(self.handle, int(k), c_ptr, assign_ptr, dist2_ptr or None, stream))

    def kmeans_step(self, centres):
        """Host-pointer form (psgd_kmeans_step): {sums[k][d], counts[k], cost, n} as k (d + 1) + 2 doubles."""
        import numpy as np
        c = np.ascontiguousarray(centres, dtype=np.float64)
        out = np.zeros(c.shape[0] * (c.shape[1] + 1) + 2, dtype=np.float64)
        check(self._L.psgd_kmeans_step(self.handle, int(c.shape[0]), c.ctypes.data, out.ctypes.data))
        return out

    def kmeans_step_device(self, k: int, c_ptr, out_ptr, stream=None):
        """psgd_kmeans_step_device: enqueued on `stream`; out[k (d + 1) + 2] on the device."""
        check(self._L.psgd_kmeans_step_device(self.handle, int(k), c_ptr, out_ptr, stream))

    def kmeans_update_device(self, k: int, d: int, c_ptr, step_ptr, new_ptr, moved_ptr, stream=None):
        """psgd_kmeans_update_device: the next centres [k d] and moved [k] from a step's output."""
        check(self._L.psgd_kmeans_update_device(self.handle, int(k), int(d), c_ptr, step_ptr, new_ptr, moved_ptr, stream))

    # decision tree --------------------------------------------------------------------------------
    def tree_bin_device(self, thresholds, nbins, max_bins: int, thr_ptr, nb_ptr, bins_ptr, labels_ptr, stream=None):
        """psgd_tree_bin_device: host thresholds [d, max_bins - 1] / nbins [d] copied to thr_ptr / nb_ptr, the
        binned rows and label bytes written on `stream`."""
        check(self._L.psgd_tree_bin_device(self.handle, thresholds.ctypes.data, nbins.ctypes.data, int(max_bins), thr_ptr,
                                           nb_ptr, bins_ptr, labels_ptr, stream))

    def tree_histogram_device(self, bins_ptr, labels_ptr, slot_ptr, K: int, max_bins: int, slot0: int, n_slots: int,
                              replication: int, hist_ptr, nbad_ptr, stream=None):
        """psgd_tree_histogram_device: hist [n_slots, d, max_bins, K] int64 of slots slot0 .. on the device."""
        check(self._L.psgd_tree_histogram_device(self.handle, bins_ptr, labels_ptr, slot_ptr, int(K), int(max_bins),
                                                 int(slot0), int(n_slots), int(replication), hist_ptr, nbad_ptr, stream))

    def tree_best_split_device(self, hist_ptr, thr_ptr, nb_ptr, d: int, max_bins: int, K: int, n_slots: int, impurity: int,
                               min_instances: int, min_info_gain: float, rec_ptr, stream=None):
        """psgd_tree_best_split_device: rec [n_slots, 6 + 2 K] doubles on the device."""
        check(self._L.psgd_tree_best_split_device(self.handle, hist_ptr, thr_ptr, nb_ptr, int(d), int(max_bins), int(K),
                                                  int(n_slots), int(impurity), int(min_instances), float(min_info_gain),
                                                  rec_ptr, stream))

    def tree_route_device(self, bins_ptr, table_ptr, n_table: int, slot_ptr, stream=None):
        """psgd_tree_route_device: slot[r] rewritten from table [n_table, 4] int32."""
        check(self._L.psgd_tree_route_device(self.handle, bins_ptr, table_ptr, int(n_table), slot_ptr, stream))

    @staticmethod
    def _tree_nodes(nodes):
        import numpy as np
        kinds = (("feature", np.int32), ("threshold", np.float64), ("left", np.int32), ("right", np.int32),
                 ("prediction", np.int32), ("probability", np.float64))
        return [np.ascontiguousarray(nodes[k], dtype=t) for k, t in kinds]

    def tree_predict(self, nodes, probability: bool = False):
        """Host-pointer form (psgd_tree_predict): (classes int32 [local rows], probabilities or None) of the
        tree `nodes` (a mapping of the arrays feature, threshold, left, right, prediction, probability)."""
        import numpy as np
        arr = self._tree_nodes(nodes)
        n = self.local_rows()
        cls = np.zeros(max(n, 1), dtype=np.int32)
        prob = np.zeros(max(n, 1), dtype=np.float64) if probability else None
        check(self._L.psgd_tree_predict(self.handle, len(arr[0]), *[a.ctypes.data for a in arr], cls.ctypes.data,
                                        None if prob is None else prob.ctypes.data))
        return cls[:n], None if prob is None else prob[:n]

    def tree_predict_device(self, nodes, cls_ptr, prob_ptr, stream=None):
        """psgd_tree_predict_device: classes / probabilities (0: none) [local rows] on the device."""
        arr = self._tree_nodes(nodes)
        check(self._L.psgd_tree_predict_device(self.handle, len(arr[0]), *[a.ctypes.data for a in arr], cls_ptr,
                                               prob_ptr or None, stream))

    # regression tree ------------------------------------------------------------------------------
    def tree_label_range_device(self, y_ptr, range_ptr, stream=None):
        """psgd_tree_label_range_device: range uint64 [3] = {min key, max key, bad labels} (y_ptr 0: the registered labels)."""
        check(self._L.psgd_tree_label_range_device(self.handle, y_ptr or None, range_ptr, stream))

    def tree_targets_device(self, y_ptr, ymin: float, s: int, q_ptr, stream=None):
        """psgd_tree_targets_device: q uint32 [local rows] = rint((y - ymin) 2^s)."""
        check(self._L.psgd_tree_targets_device(self.handle, y_ptr or None, float(ymin), int(s), q_ptr, stream))

    def tree_moments_device(self, q_ptr, slot_ptr, slot0: int, n_slots: int, mom_ptr, stream=None):
        """psgd_tree_moments_device: mom int64 [n_slots, 4] of slots slot0 .. on the device."""
        check(self._L.psgd_tree_moments_device(self.handle, q_ptr, slot_ptr, int(slot0), int(n_slots), mom_ptr, stream))

    def tree_histogram_reg_device(self, bins_ptr, q_ptr, slot_ptr, max_bins: int, slot0: int, n_slots: int, replication: int,
                                  hist_ptr, stream=None):
        """psgd_tree_histogram_reg_device: hist [n_slots, d, max_bins, 2] int64 {rows, sum q} of slots slot0 .. ."""
        check(self._L.psgd_tree_histogram_reg_device(self.handle, bins_ptr, q_ptr, slot_ptr, int(max_bins), int(slot0),
                                                     int(n_slots), int(replication), hist_ptr, stream))

    def tree_best_split_reg_device(self, hist_ptr, mom_ptr, thr_ptr, nb_ptr, d: int, max_bins: int, n_slots: int, s: int,
                                   min_instances: int, min_info_gain: float, rec_ptr, stream=None):
        """psgd_tree_best_split_reg_device: rec [n_slots, 4] doubles on the device."""
        check(self._L.psgd_tree_best_split_reg_device(self.handle, hist_ptr, mom_ptr, thr_ptr, nb_ptr, int(d), int(max_bins),
                                                      int(n_slots), int(s), int(min_instances), float(min_info_gain),
                                                      rec_ptr, stream))

    # random forest --------------------------------------------------------------------------------
    def forest_bag_device(self, seed: int, cut, row0: int, tree0: int, n_trees: int, w_ptr, stream=None):
        """psgd_forest_bag_device: the bag weights [n_trees, local rows] uint8 of trees tree0 .. (cut: 15 uint64)."""
        check(self._L.psgd_forest_bag_device(self.handle, int(seed), cut.ctypes.data, int(row0), int(tree0), int(n_trees),
                                             w_ptr, stream))

    def forest_histogram_device(self, bins_ptr, labels_ptr, slot_ptr, n_trees: int, node_tree_ptr, tree_base_ptr, sub_ptr,
                                n_frontier: int, m: int, K: int, max_bins: int, node0: int, n_nodes: int, seed: int, cut,
                                row0: int, tree0: int, hist_ptr, nbad_ptr, stream=None):
        """psgd_forest_histogram_device: hist [n_nodes, m, max_bins, K] int64 of frontier nodes node0 .. ."""
        check(self._L.psgd_forest_histogram_device(self.handle, bins_ptr, labels_ptr, slot_ptr, int(n_trees), node_tree_ptr,
                                                   tree_base_ptr, sub_ptr, int(n_frontier), int(m), int(K), int(max_bins),
                                                   int(node0), int(n_nodes), int(seed), cut.ctypes.data, int(row0),
                                                   int(tree0), hist_ptr, nbad_ptr, stream))

    def forest_best_split_device(self, hist_ptr, thr_ptr, nb_ptr, sub_ptr, m: int, max_bins: int, K: int, n_nodes: int,
                                 impurity: int, min_instances: int, min_info_gain: float, rec_ptr, stream=None):
        """psgd_forest_best_split_device: rec [n_nodes, 6 + 2 K] doubles on the device."""
        check(self._L.psgd_forest_best_split_device(self.handle, hist_ptr, thr_ptr, nb_ptr, sub_ptr, int(m), int(max_bins),
                                                    int(K), int(n_nodes), int(impurity), int(min_instances),
                                                    float(min_info_gain), rec_ptr, stream))

    def forest_route_device(self, bins_ptr, table_ptr, tree_base_ptr, n_trees: int, slot_ptr, stream=None):
        """psgd_forest_route_device: slot[t][r] rewritten from table [A, 4] int32."""
        check(self._L.psgd_forest_route_device(self.handle, bins_ptr, table_ptr, tree_base_ptr, int(n_trees), slot_ptr, stream))

    @staticmethod
    def _forest_nodes(trees):
        """(tree_off [T + 1], the concatenated feature, threshold, left, right, prediction arrays) of node mappings."""
        import numpy as np
        off = np.concatenate([[0], np.cumsum([len(t["feature"]) for t in trees])]).astype(np.int32)
        kinds = (("feature", np.int32), ("threshold", np.float64), ("left", np.int32), ("right", np.int32),
                 ("prediction", np.int32))
        return [off] + [np.ascontiguousarray(np.concatenate([np.asarray(t[k]) for t in trees]), dtype=ty) for k, ty in kinds]

    def forest_predict(self, trees, K: int, votes: bool = False):
        """Host-pointer form (psgd_forest_predict): (classes int32 [local rows], votes [local rows, K] or None)."""
        import numpy as np
        arr = self._forest_nodes(trees)
        n = self.local_rows()
        cls = np.zeros(max(n, 1), dtype=np.int32)
        vt = np.zeros((max(n, 1), int(K)), dtype=np.int32) if votes else None
        check(self._L.psgd_forest_predict(self.handle, len(trees), *[a.ctypes.data for a in arr], int(K), cls.ctypes.data,
                                          None if vt is None else vt.ctypes.data))
        return cls[:n], None if vt is None else vt[:n]

    def forest_predict_device(self, trees, K: int, cls_ptr, votes_ptr, stream=None):
        """psgd_forest_predict_device: classes / votes (0: none) of the local rows on the device."""
        arr = self._forest_nodes(trees)
        check(self._L.psgd_forest_predict_device(self.handle, len(trees), *[a.ctypes.data for a in arr], int(K), cls_ptr,
                                                 votes_ptr or None, stream))

    # Gaussian mixture ---------------------------------------------------------------------------
    def gmm_responsibilities(self, A, b, c, mahalanobis: bool = False):
        """Host-pointer form (psgd_gmm_responsibilities) at A [k, d, d], b [k, d], c [k]:
        (resp [local rows, k], loglik, q or None)."""
        import numpy as np
        A, b, c = (np.ascontiguousarray(v, dtype=np.float64) for v in (A, b, c))
        k, n = int(c.shape[0]), self.local_rows()
        resp = np.zeros((max(n, 1), k), dtype=np.float64)
        q = np.zeros((max(n, 1), k), dtype=np.float64) if mahalanobis else None
        ll = np.zeros(1, dtype=np.float64)
        check(self._L.psgd_gmm_responsibilities(self.handle, k, A.ctypes.data, b.ctypes.data, c.ctypes.data,
                                                resp.ctypes.data, None if q is None else q.ctypes.data, ll.ctypes.data))
        return resp[:n], float(ll[0]), None if q is None else q[:n]

    def gmm_responsibilities_device(self, k: int, a_ptr, b_ptr, c_ptr, resp_ptr, q_ptr, ll_ptr, stream=None):
        """psgd_gmm_responsibilities_device: enqueued on `stream`; resp / q (0: none) [local rows, k] and
        loglik [1] on the device."""
        check(self._L.psgd_gmm_responsibilities_device(self.handle, int(k), a_ptr, b_ptr, c_ptr, resp_ptr, q_ptr or None,
                                                       ll_ptr, stream))

    def gmm_moments_device(self, k: int, resp_ptr, out_ptr, stream=None):
        """psgd_gmm_moments_device: out[k (d + 1)^2] from resp [local rows, k], both on the device."""
        check(self._L.psgd_gmm_moments_device(self.handle, int(k), resp_ptr, out_ptr, stream))

    def gmm_step(self, A, b, c):
        """Host-pointer form (psgd_gmm_step): {S[k][d + 1][d + 1], loglik, n} as k (d + 1)^2 + 2 doubles."""
        import numpy as np
        A, b, c = (np.ascontiguousarray(v, dtype=np.float64) for v in (A, b, c))
        k, d = int(b.shape[0]), int(b.shape[1])
        out = np.zeros(k * (d + 1) * (d + 1) + 2, dtype=np.float64)
        check(self._L.psgd_gmm_step(self.handle, k, A.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data))
        return out

    def gmm_step_device(self, k: int, a_ptr, b_ptr, c_ptr, out_ptr, stream=None):
        """psgd_gmm_step_device: enqueued on `stream`; out[k (d + 1)^2 + 2] on the device."""
        check(self._L.psgd_gmm_step_device(self.handle, int(k), a_ptr, b_ptr, c_ptr, out_ptr, stream))

    def transform_columns(self, shift, factor):
        """Host-pointer form (psgd_transform_columns): x = ((double)x - shift) * factor in place on
        the context's own rows; shift may be None. Calling it twice scales twice."""
        import numpy as np
        factor = np.ascontiguousarray(factor, dtype=np.float64)
        shift = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
        check(self._L.psgd_transform_columns(self.handle, None if shift is None else shift.ctypes.data,
                                             factor.ctypes.data))

    def transform_columns_device(self, shift_ptr, factor_ptr, stream=None):
        check(self._L.psgd_transform_columns_device(self.handle, shift_ptr, factor_ptr, stream))

    # the batch gradient and the batch update ----------------------------------------------------
    def gradient_sum(self, gradient: int, w, fraction: float = 1.0, iteration: int = 0):
        """Host-pointer form (psgd_gradient_sum): the d + 2 doubles {gradientSum[d], lossSum, count}
        of host weights w over the batch (every row, or RDD.sample(false, fraction, 42 + iteration))."""
        import numpy as np
        w = np.ascontiguousarray(w, dtype=np.float64)
        out = np.zeros(w.shape[0] + 2, dtype=np.float64)
        check(self._L.psgd_gradient_sum(self.handle, int(gradient), w.ctypes.data, float(fraction), int(iteration),
                                        out.ctypes.data))
        return out

    def gradient_sum_device(self, gradient: int, w_ptr, fraction, iteration, out_ptr, stream=None):
        """psgd_gradient_sum_device: enqueued on `stream`; out[d + 2] on the device."""
        check(self._L.psgd_gradient_sum_device(self.handle, int(gradient), w_ptr, float(fraction), int(iteration),
                                               out_ptr, stream))

    def gradient_sum_multinomial(self, num_classes: int, w, fraction: float = 1.0, iteration: int = 0,
                                 method: str = "auto"):
        """Host-pointer form (psgd_gradient_sum_multinomial_method): the (K - 1) d + 2 doubles
        {gradientSum, lossSum, count} of the (K - 1) d host weights w over the batch; method as mn_method."""
        import numpy as np
        w = np.ascontiguousarray(w, dtype=np.float64)
        out = np.zeros(w.shape[0] + 2, dtype=np.float64)
        check(self._L.psgd_gradient_sum_multinomial_method(self.handle, int(num_classes), w.ctypes.data,
                                                           float(fraction), int(iteration), mn_method(method),
                                                           out.ctypes.data))
        return out

    def gradient_sum_multinomial_device(self, num_classes: int, w_ptr, fraction, iteration, out_ptr, stream=None,
                                        method: str = "auto"):
        """psgd_gradient_sum_multinomial_method_device: enqueued on `stream`; out[(K - 1) d + 2] on the device."""
        check(self._L.psgd_gradient_sum_multinomial_method_device(self.handle, int(num_classes), w_ptr, float(fraction),
                                                                  int(iteration), mn_method(method), out_ptr, stream))

    def gd_update(self, updater: int, w, gsum, step: float, iteration: int, reg: float):
        """Host-pointer form (psgd_gd_update): (w', regVal) of one GradientDescent update."""
        import numpy as np
        w = np.ascontiguousarray(w, dtype=np.float64)
        gsum = np.ascontiguousarray(gsum, dtype=np.float64)
        out = np.zeros_like(w)
        rv = C.c_double()
        check(self._L.psgd_gd_update(self.handle, int(updater), int(w.shape[0]), w.ctypes.data, gsum.ctypes.data,
                                     float(step), int(iteration), float(reg), out.ctypes.data, C.byref(rv)))
        return out, rv.value

    def gd_update_device(self, updater: int, d: int, w_ptr, sum_ptr, step, iteration, reg, w_out_ptr, regval_ptr,
                         stream=None):
        check(self._L.psgd_gd_update_device(self.handle, int(updater), int(d), w_ptr, sum_ptr, float(step),
                                            int(iteration), float(reg), w_out_ptr, regval_ptr, stream))

    # binary classification metrics ------------------------------------------------------------------
    def binary_counts(self, scores, labels, table: bool = True):
        """Host-pointer form (psgd_binary_counts): (thresholds, cumPos, cumNeg, summary, areas) of host
        scores and labels; the three table arrays hold G rows, or are None with table=False.
        summary = [G, P, N, rocNumerator], areas = [areaUnderROC, areaUnderPR]."""
        import numpy as np
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        labels = np.ascontiguousarray(labels, dtype=np.float64)
        n = int(scores.shape[0])
        summary, areas = np.zeros(4, dtype=np.int64), np.zeros(2, dtype=np.float64)
        thr = np.zeros(max(n, 1), dtype=np.float64) if table else None
        cp = np.zeros(max(n, 1), dtype=np.int64) if table else None
        cn = np.zeros(max(n, 1), dtype=np.int64) if table else None
        ptr = lambda a: None if a is None else a.ctypes.data
        check(self._L.psgd_binary_counts(self.handle, scores.ctypes.data, labels.ctypes.data, n, ptr(thr), ptr(cp),
                                         ptr(cn), summary.ctypes.data, areas.ctypes.data))
        G = int(summary[0])
        if not table:
            return None, None, None, summary, areas
        return thr[:G].copy(), cp[:G].copy(), cn[:G].copy(), summary, areas

    def binary_counts_device(self, scores_ptr, labels_ptr, n, thr_ptr, cp_ptr, cn_ptr, summary_ptr, areas_ptr,
                             stream=None):
        """psgd_binary_counts_device: enqueued on `stream`; every pointer on the device."""
        check(self._L.psgd_binary_counts_device(self.handle, scores_ptr, labels_ptr, C.c_int64(n), thr_ptr, cp_ptr,
                                                cn_ptr, summary_ptr, areas_ptr, stream))

    def binary_counts_model_device(self, w_ptr, thr_ptr, cp_ptr, cn_ptr, summary_ptr, areas_ptr, stream=None):
        """psgd_binary_counts_model_device: every registered row scored at w; enqueued on `stream`."""
        check(self._L.psgd_binary_counts_model_device(self.handle, w_ptr, thr_ptr, cp_ptr, cn_ptr, summary_ptr,
                                                      areas_ptr, stream))

    # train/test splits ------------------------------------------------------------------------------
    def cell_select(self, seed: int, seeding: int, lb: float, ub: float, complement: bool, rows_ptr):
        """Host-pointer form (psgd_cell_select): (counts, nnz) per registered partition of
        cell(lb, ub, complement); the kept row indices go to the device int32 array at rows_ptr."""
        import numpy as np
        nparts, _ = self.num_partitions()
        counts = np.zeros(max(nparts, 1), dtype=np.int64)
        nnz = np.zeros(max(nparts, 1), dtype=np.int64)
        check(self._L.psgd_cell_select(self.handle, _java_long(seed), int(seeding), float(lb), float(ub),
                                       1 if complement else 0, rows_ptr, counts.ctypes.data, nnz.ctypes.data))
        return counts[:nparts], nnz[:nparts]

    def cell_select_device(self, seed: int, seeding: int, lb: float, ub: float, complement: bool, rows_ptr,
                           counts_ptr, nnz_ptr=None, stream=None):
        """psgd_cell_select_device: enqueued on `stream`; counts[n_parts] and nnz[n_parts] on the device."""
        check(self._L.psgd_cell_select_device(self.handle, _java_long(seed), int(seeding), float(lb), float(ub),
                                              1 if complement else 0, rows_ptr, counts_ptr, nnz_ptr, stream))

    def gather_dense_device(self, rows_ptr, counts, ld_out: int, x_ptrs, label_ptrs, stream=None):
        """psgd_gather_dense_device: counts a host int64 array, x_ptrs / label_ptrs the per-partition
        device addresses (0 where nothing is kept)."""
        import numpy as np
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        xs = np.ascontiguousarray(x_ptrs, dtype=np.uint64)
        ys = np.ascontiguousarray(label_ptrs, dtype=np.uint64)
        check(self._L.psgd_gather_dense_device(self.handle, rows_ptr, counts.ctypes.data, int(ld_out), xs.ctypes.data,
                                               ys.ctypes.data, stream))

    def gather_csr_device(self, rows_ptr, counts, nnz, label_ptrs, row_ptr_ptrs, col_ptrs, val_ptrs, stream=None):
        """psgd_gather_csr_device: counts / nnz host int64 arrays, the rest per-partition device addresses."""
        import numpy as np
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        nnz = np.ascontiguousarray(nnz, dtype=np.int64)
        a = [np.ascontiguousarray(v, dtype=np.uint64) for v in (label_ptrs, row_ptr_ptrs, col_ptrs, val_ptrs)]
        check(self._L.psgd_gather_csr_device(self.handle, rows_ptr, counts.ctypes.data, nnz.ctypes.data,
                                             a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data,
                                             stream))


def _java_long(v: int) -> int:
    """v wrapped to a Java Long (two's complement, 64 bits)."""
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= 1 << 63 else v
