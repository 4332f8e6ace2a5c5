"""numpy truth for the row projection Y = X B (psgd_project) and for PCA.

project_truth widens the stored values to np.longdouble and returns (Y, A): the product and the
magnitude product A = |X| |B| the fp64 bar is taken against. project_truth_int is the int64 form for
whole-number data, exact. pca_truth is PCA from the SVD of the centred rows, never from a covariance
matrix: the eigenvalues s^2 / (n - 1), descending, and the right singular vectors as columns.

The bars: |Y - truth| <= BAR * A for f64 output; f32 output adds its one rounding, 2^-24 |truth|."""
import numpy as np

BAR = 1e-9
F32_ROUND = 2.0 ** -24


def project_truth(X, B):
    Xl = np.asarray(X).astype(np.longdouble)
    Bl = np.asarray(B).astype(np.longdouble)
    return Xl @ Bl, np.abs(Xl) @ np.abs(Bl)


def project_truth_int(X, B):
    Xi, Bi = np.asarray(X).astype(np.int64), np.asarray(B).astype(np.int64)
    assert (Xi == np.asarray(X)).all() and (Bi == np.asarray(B)).all(), "whole numbers only"
    return Xi @ Bi


def check_projection(Y, T, A, out_storage, what=""):
    """Y (the device's rows, any float dtype) against the long-double truth T under the bars above."""
    Yl = np.asarray(Y).astype(np.longdouble)
    assert Yl.shape == T.shape, f"{what}: shape {Yl.shape} != {T.shape}"
    bar = BAR * A + (F32_ROUND * np.abs(T) if out_storage == "f32" else 0.0)
    err = np.abs(Yl - T)
    bad = ~(err <= bar)   # (NaN fails)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries miss the bar, first at {i}: "
                             f"got {Y[i]!r}, truth {float(T[i])!r}, bar {float(bar[i]):.3g}")
    ref = np.where(bar > 0, bar, 1.0)
    return float((err / ref).max()) if err.size else 0.0


def csr_to_dense(rows, d, dtype):
    X = np.zeros((len(rows), d), dtype=dtype)
    for k, (idx, val) in enumerate(rows):
        X[k, idx] = val
    return X


def pca_truth(X):
    """(eigenvalues of the covariance, descending; components as columns) from the SVD of the centred
    rows in float64 (longdouble centring)."""
    Xl = np.asarray(X).astype(np.longdouble)
    Z = (Xl - Xl.mean(axis=0)).astype(np.float64)
    _, s, Vt = np.linalg.svd(Z, full_matrices=False)
    return s * s / (Z.shape[0] - 1.0), Vt.T


def scaled_rows(n, d, seed):
    """Rows with column scales 1.5^-j under a random rotation, plus offsets in [-1, 1], rounded through
    f32 (exactly representable in either storage): well separated principal directions."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    Z = rng.standard_normal((n, d)) * (1.5 ** -np.arange(d))
    return (Z @ Q.T + rng.uniform(-1.0, 1.0, size=d)).astype(np.float32).astype(np.float64)


# ---- the shapes tests/test_gpu_project.py runs (test_pca_api.py checks the plan over the same) ----
DENSE_D = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 300)
DENSE_K = (1, 2, 15, 16, 17, 33)
DENSE_DK = tuple((d, k) for d in DENSE_D for k in DENSE_K if k <= d) + ((256, 256),)
DENSE_OFF_LDS = (4096, 48)         # 4,096 x 48 doubles do not fit a CU's LDS
CSR_D = (70, 1300)                 # 1,300 x 16 doubles do not fit a CU's LDS
CSR_K = (1, 16, 17)
COMBOS = (("f32", "f32"), ("f64", "f64"), ("f32", "f64"), ("f64", "f32"))   # (storage, output)


def combo_of(d, k):
    """The pruned grid: each (d, k) runs two of the four (storage, output) pairs, the four in turn."""
    i = (DENSE_DK.index((d, k)) if (d, k) in DENSE_DK else d + k) % 4
    return COMBOS[i], COMBOS[(i + 1) % 4]
