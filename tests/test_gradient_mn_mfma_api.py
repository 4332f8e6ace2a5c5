"""The multinomial batch gradient's method argument without a device: the host plan of method "mfma"
(psgd_gradient_multinomial_plan_method) at its boundaries, its refusals, and "auto" unchanged."""
import ctypes

import pytest


def plan(pkg, *a, **k):
    return pkg._native.gradient_multinomial_plan(*a, **k)


def test_mfma_plan_geometry(pkg):
    p = plan(pkg, "dense", "f32", 100, 10, method="mfma")
    assert p["path"] == "mfma" and p["class_blocks"] == 1 and p["tile_rows"] == 1024 and p["dpad"] == 112
    assert p["rect_class_blocks"] == 1 and p["rect_feature_blocks"] == 8 and p["col_chunks"] == 1 and p["span"] == 1
    assert plan(pkg, "dense", "f64", 100, 10, method="mfma")["dpad"] == 104
    # the class blocks go up at K - 1 = 17, and the rectangle and the record's span with them
    assert [plan(pkg, "dense", "f32", 3, K, method="mfma")["class_blocks"] for K in (3, 17, 18, 33, 34, 49, 50, 65)] \
        == [1, 1, 2, 2, 3, 3, 4, 4]
    assert [plan(pkg, "dense", "f32", 3, K, method="mfma")["span"] for K in (17, 18, 34, 65)] == [1, 2, 4, 4]
    # 130 features: 9 blocks of 16, past the 8 of one rectangle
    assert plan(pkg, "dense", "f32", 130, 3, method="mfma")["col_chunks"] == 2
    assert plan(pkg, "dense", "f32", 32, 3, method="mfma")["rect_feature_blocks"] == 2


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_mfma_packed_w_in_lds_while_it_fits(pkg, storage):
    """dpad * 16 nb * 8 <= 163,840 bytes."""
    for K, d_in, d_out in ((65, 320, 324), (17, 1280, 1281), (3, 1280, 1281), (33, 640, 641)):
        assert plan(pkg, "dense", storage, d_in, K, method="mfma")["weights_in_lds"] == 1
        assert plan(pkg, "dense", storage, d_out, K, method="mfma")["weights_in_lds"] == 0


def test_mfma_plan_refusals(pkg):
    L, N = pkg._native.lib(), pkg._native
    out = (ctypes.c_int32 * 12)()
    call = L.psgd_gradient_multinomial_plan_method
    assert call(0, 1, 4096, 65, 0, N.MN_METHODS["mfma"], out) == N.PSGD_OK and out[0] == 4
    for args, word in (((1, 1, 100, 3, 8), b"CSR"), ((0, 1, 100, 66, 0), b"65"), ((0, 1, 4097, 3, 0), b"4096")):
        assert call(*args, N.MN_METHODS["mfma"], out) == N.PSGD_EUNSUPPORTED
        assert word in L.psgd_last_error()
    for method in (2, -1):
        assert call(0, 1, 100, 3, 0, method, out) == N.PSGD_EINVAL
        assert b"method" in L.psgd_last_error()
        assert L.psgd_gradient_sum_multinomial_method(None, 3, None, 1.0, 1, method, None) == N.PSGD_EINVAL
    with pytest.raises(pkg.UnsupportedOperationException, match="d <= 4096"):
        plan(pkg, "dense", "f32", 5000, 3, method="mfma")
    with pytest.raises(pkg.IllegalArgumentException, match="unknown multinomial gradient method"):
        plan(pkg, "dense", "f32", 100, 3, method="tensor")
    with pytest.raises(pkg.IllegalArgumentException, match="unknown multinomial gradient method"):
        pkg.GradientDescent(pkg.LogisticGradient(3), pkg.SimpleSGDUpdater()).setMultinomialMethod("tensor")


@pytest.mark.parametrize("shape", [("dense", "f32", 100, 3, 0), ("dense", "f32", 512, 10, 0), ("dense", "f64", 20, 66, 0),
                                   ("csr", "f32", 1000, 3, 300), ("csr", "f64", 200000, 5, 40)])
def test_auto_is_the_old_plan(pkg, shape, monkeypatch):
    for name in ("PSGD_GRAD_MN_TWO_PASS", "PSGD_GRAD_MN_FUSE_ALL", "PSGD_GRAD_CSR_GLOBAL", "PSGD_GRAD_MN_RANGE"):
        monkeypatch.delenv(name, raising=False)
    old = (ctypes.c_int32 * 12)()
    layout, storage, d, K, nnz = shape
    L = pkg._native.lib()
    assert L.psgd_gradient_multinomial_plan({"dense": 0, "csr": 1}[layout], {"f64": 0, "f32": 1}[storage], d, K, nnz, old) == 0
    new = plan(pkg, *shape, method="auto")
    assert new == plan(pkg, *shape) and new["path"] != "mfma"
    assert [pkg._native.MN_GRAD_PATHS.index(new["path"])] + list(new.values())[1:] == list(old)
