"""The truth the Gramian tests compare against: with z_i = [x_i, y_i, 1] from the stored values widened
to float64, M = Z^T Z and the magnitudes A = |Z|^T |Z| (the fp64 bar is 1e-9 A_jk per entry)."""
import numpy as np

BAR = 1e-9


def augment(X, y):
    """Z (n x (d + 2)) in float64: the stored features, the label, a column of ones."""
    X = np.asarray(X)
    n = X.shape[0]
    Z = np.empty((n, X.shape[1] + 2), dtype=np.float64)
    Z[:, :-2] = X
    Z[:, -2] = np.asarray(y, dtype=np.float64)
    Z[:, -1] = 1.0
    return Z


def gram_truth(X, y):
    """(M, A): Z^T Z and |Z|^T |Z| in float64."""
    Z = augment(X, y)
    return Z.T @ Z, np.abs(Z).T @ np.abs(Z)


def gram_truth_int(X, y):
    """Z^T Z in int64 for whole-number data: exact."""
    Z = augment(X, y)
    Zi = Z.astype(np.int64)
    assert (Zi == Z).all()
    return Zi.T @ Zi


def csr_to_dense(rows, d, dtype=np.float64):
    """rows: (indices, values) pairs -> a dense array of the stored values (absent entries zero)."""
    X = np.zeros((len(rows), d), dtype=dtype)
    for i, (idx, val) in enumerate(rows):
        X[i, idx] = val
    return X


def check_gramian(M, T, A, what=""):
    """Every entry within the bar, exact symmetry, the exact count."""
    M = np.asarray(M)
    assert M.shape == T.shape, what
    assert not np.isnan(M).any(), what
    err = np.abs(M - T)
    bad = err > BAR * A
    assert not bad.any(), f"{what}: {int(bad.sum())} entries off, first at {tuple(np.argwhere(bad)[0])}, worst {err.max():.3g}"
    assert (M == M.T).all(), f"{what}: not symmetric"
    assert M[-1, -1] == T[-1, -1], f"{what}: count {M[-1, -1]} != {T[-1, -1]}"
