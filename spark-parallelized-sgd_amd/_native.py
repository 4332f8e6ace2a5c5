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
    "psgd_gramian", "psgd_gramian_device", "psgd_gramian_plan",
    "psgd_gramian_weighted", "psgd_gramian_weighted_device", "psgd_local_rows",
    "psgd_row_curvature", "psgd_row_curvature_device",
    "psgd_project", "psgd_project_device", "psgd_project_plan",
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
            "psgd_gramian": ([vp, vp], C.c_int32),
            "psgd_gramian_device": ([vp, vp, vp], C.c_int32),
            "psgd_gramian_plan": ([C.c_int32, C.c_int32, C.c_int32, C.c_int64, vp], C.c_int32),
            "psgd_gramian_weighted": ([vp, vp, vp], C.c_int32),
            "psgd_gramian_weighted_device": ([vp, vp, vp, vp], C.c_int32),
            "psgd_local_rows": ([vp, vp], C.c_int32),
            "psgd_row_curvature": ([vp, C.c_int32, vp, vp], C.c_int32),
            "psgd_row_curvature_device": ([vp, C.c_int32, vp, vp, vp], C.c_int32),
            "psgd_project": ([vp, C.c_int64, C.c_int32, vp, vp], C.c_int32),
            "psgd_project_device": ([vp, C.c_int32, vp, C.c_int32, C.c_int64, vp, vp, vp], C.c_int32),
            "psgd_project_plan": ([C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, vp], C.c_int32),
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


MN_GRAD_PATHS = ("fused", "general", "csr_lds", "csr_global")   # psgd_gradient_multinomial_plan's out[0]


def gradient_multinomial_plan(layout: str, storage: str, d: int, num_classes: int, max_nnz: int = 0) -> dict:
    """Which kernels psgd_gradient_sum_multinomial runs for rows of `layout` ("dense" / "csr") stored
    as `storage` ("f32" / "f64"), with the environment switches as they are now
    (psgd_gradient_multinomial_plan: host code, no device)."""
    out = (C.c_int32 * 12)()
    check(lib().psgd_gradient_multinomial_plan({"dense": 0, "csr": 1}[layout], {"f64": 0, "f32": 1}[storage],
                                               int(d), int(num_classes), int(max_nnz), out))
    keys = ("path", "group", "weights_in_lds", "wide_softmax", "tile_rows", "nvl", "class_accumulators",
            "acc_group", "col_chunks", "class_chunks", "span", "range")
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

    def gradient_sum_multinomial(self, num_classes: int, w, fraction: float = 1.0, iteration: int = 0):
        """Host-pointer form (psgd_gradient_sum_multinomial): the (K - 1) d + 2 doubles {gradientSum,
        lossSum, count} of the (K - 1) d host weights w over the batch."""
        import numpy as np
        w = np.ascontiguousarray(w, dtype=np.float64)
        out = np.zeros(w.shape[0] + 2, dtype=np.float64)
        check(self._L.psgd_gradient_sum_multinomial(self.handle, int(num_classes), w.ctypes.data, float(fraction),
                                                    int(iteration), out.ctypes.data))
        return out

    def gradient_sum_multinomial_device(self, num_classes: int, w_ptr, fraction, iteration, out_ptr, stream=None):
        """psgd_gradient_sum_multinomial_device: enqueued on `stream`; out[(K - 1) d + 2] on the device."""
        check(self._L.psgd_gradient_sum_multinomial_device(self.handle, int(num_classes), w_ptr, float(fraction),
                                                           int(iteration), out_ptr, stream))

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
