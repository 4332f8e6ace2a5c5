"""The yardsticks of the tall-skinny QR tests: how far R^T R is from Z^T Z, and LAPACK's R."""
import numpy as np


def colres(R, Z):
    """max_jk |R^T R - Z^T Z|_jk / (||z_j|| ||z_k||) in long double, zero columns skipped."""
    Rl, Zl = np.asarray(R, dtype=np.longdouble), np.asarray(Z, dtype=np.longdouble)
    nrm = np.sqrt((Zl * Zl).sum(axis=0))
    keep = nrm > 0
    diff = np.abs(Rl.T @ Rl - Zl.T @ Zl)[np.ix_(keep, keep)]
    return float((diff / np.outer(nrm[keep], nrm[keep])).max())


def lapack_r(Z):
    """numpy.linalg.qr(Z, mode="r") with the diagonal made non-negative, padded to a square."""
    Z = np.asarray(Z, dtype=np.float64)
    R = np.linalg.qr(Z, mode="r")
    R = np.where(np.diag(R) < 0, -1.0, 1.0)[:, None] * R
    out = np.zeros((Z.shape[1], Z.shape[1]))
    out[: R.shape[0]] = R
    return out
