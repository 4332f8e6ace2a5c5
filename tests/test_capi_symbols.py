"""The C-ABI library loads and exports every symbol include/psgd.h declares (no compute calls
without a GPU); error paths that need no device behave."""
import ctypes
import os
import re

import pytest

from conftest import ROOT, has_gpu


def header_functions():
    src = open(os.path.join(ROOT, "include", "psgd.h")).read()
    return sorted(set(re.findall(r"^\s*(?:int32_t|int64_t|void|const char\*)\s+(psgd_\w+)\s*\(", src, re.M)))


def test_header_matches_binding_table(pkg):
    assert header_functions() == sorted(pkg._native.EXPORTED)


def test_library_exports_every_declared_symbol(pkg):
    path = pkg._native.LIB_PATH
    assert os.path.exists(path), "libpsgd.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(path)
    for name in header_functions():
        assert hasattr(lib, name), name


def test_abi_version_and_no_device_error(pkg):
    L = pkg._native.lib()
    assert L.psgd_abi_version() == 1
    if has_gpu():
        pytest.skip("device present")
    h = ctypes.c_void_p()
    rc = L.psgd_ctx_create(0, ctypes.byref(h))
    assert rc == pkg._native.PSGD_EDEVICE
    assert b"no HIP device" in L.psgd_last_error()
    assert L.psgd_ctx_destroy(None) == 0
    # null-context calls fail cleanly
    assert L.psgd_clear_partitions(None) == pkg._native.PSGD_EINVAL


def test_kernels_are_gfx950_code_objects(pkg):
    data = open(pkg._native.LIB_PATH, "rb").read()
    assert b"gfx950" in data
    assert b"chain_dense" in data and b"chain_general" in data and b"fold_kernel" in data


def test_kernel_selection_limits_on_the_host(pkg, monkeypatch):
    """The selection is host code (plan_chains; no device needed). chain_sparse_lds (fp32 and fp64)
    counts a chain's rows in 32 bits, so a partition of more than INT32_MAX rows must not select
    it (such partitions fit in HBM as 16-byte CSR rows); chain_sparse64 takes fp64 CSR
    with Simple, or SquaredL2 while alpha stays in range, with or without the per-sample break
    (variants 420/421, 460/461)."""
    from test_chain_plan import ADAGRAD, CSR, DENSE, F32, F64, L1, L2, SIMPLE, SWITCHES, chain_plan
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)

    def plan(compute, updater=SIMPLE, tol=False, alpha_ok=True, layout=CSR, d=47236, nnz=94, n_max=1000, storage=F32):
        p = chain_plan(pkg, layout=layout, storage=storage, compute=compute, updater=updater, tol=tol, d=d,
                       max_ld=d, max_nnz=nnz, n_max=n_max, alpha_ok=alpha_ok)
        return p["family"], p["variant"]

    big = 2**31 - 1
    assert plan(F32, n_max=big) == ("sparse_lds", 601) and plan(F32, n_max=big + 1)[0] != "sparse_lds"
    assert plan(F64, alpha_ok=True, n_max=big) == ("sparse_lds", 621)
    assert plan(F64, alpha_ok=True, n_max=big + 1)[0] != "sparse_lds"
    assert plan(F32, nnz=129, n_max=100)[0] != "sparse_lds"   # rows of more than 128 entries
    assert plan(F64, tol=True) == ("sparse_lds", 661)          # the per-sample break runs in chain_sparse_lds
    # chain_sparse64: where the LDS kernel cannot apply (d = 2^22), and where it is switched off
    for kw in ({"d": 2**22}, {}):
        monkeypatch.setenv("PSGD_SPARSE_KERNEL", "" if kw else "hbm64")
        assert plan(F64, SIMPLE, alpha_ok=False, **kw) == ("sparse64", 421)
        assert plan(F64, L2, alpha_ok=True, **kw) == ("sparse64", 421)
        assert plan(F64, SIMPLE, alpha_ok=False, storage=F64, **kw) == ("sparse64", 420)
        # alpha out of range: chain_general renormalises
        assert plan(F64, L2, alpha_ok=False, **kw) == ("general", 201)
        # ... and the per-sample break runs in chain_sparse64 too
        assert plan(F64, SIMPLE, tol=True, **kw) == ("sparse64", 461)
        assert plan(F64, L2, tol=True, **kw) == ("sparse64", 461)
        assert plan(F64, L2, tol=True, alpha_ok=False, **kw) == ("general", 201)
        # never for fp32 compute, dense rows or L1
        for upd in (SIMPLE, L2, L1, ADAGRAD):
            for tol in (False, True):
                assert plan(F32, upd, tol=tol, **kw)[0] != "sparse64"
                for compute in (F64, F32):
                    assert plan(compute, upd, tol=tol, layout=DENSE, d=512)[0] != "sparse64"
                    assert plan(compute, upd, tol=tol, layout=DENSE, d=4096)[0] != "sparse64"
        assert plan(F64, L1, **kw) == ("general", 201) and plan(F64, L1, tol=True, **kw) == ("general", 201)
