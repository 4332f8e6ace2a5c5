"""The truth the second-order tests compare against, in numpy float64: the rows' curvature, the
row-weighted Gramian with its magnitudes, and a Newton iteration with the product's line search that
records how far every Armijo decision was from flipping.

The losses are MLlib's (Gradient.scala), y in {0, 1} for Logistic:
  logistic        loss = log(1 + exp(-z)) + (1 - y) z,  dloss/dz = sigma(z) - y,  d2loss/dz2 = sigma(z)(1 - sigma(z))
  least_squares   loss = (z - y)^2 / 2,                 dloss/dz = z - y,         d2loss/dz2 = 1
with z = x . w."""
import numpy as np

from gram_truth import augment

ARMIJO_C = 1e-4
MAX_HALVINGS = 30


def curvature(X, w, kind):
    """d2loss/dz2 per row. Logistic: e / (1 + e)^2 with e = exp(-|z|), which is sigma(z)(1 - sigma(z))
    without cancellation: 0.25 at z = 0, 0.0 once e underflows."""
    z = np.asarray(X, dtype=np.float64) @ np.asarray(w, dtype=np.float64)
    if kind == "least_squares":
        return np.ones_like(z)
    assert kind == "logistic"
    with np.errstate(under="ignore"):
        e = np.exp(-np.abs(z))
    return e / ((1.0 + e) * (1.0 + e))


def weighted_gram(X, y, omega):
    """(M_w, A_w): Z^T diag(omega) Z and the magnitudes |Z|^T diag|omega| |Z| (the fp64 bar is 1e-9 A_w
    per entry)."""
    Z = augment(X, y)
    om = np.asarray(omega, dtype=np.float64)
    return Z.T @ (Z * om[:, None]), np.abs(Z).T @ (np.abs(Z) * np.abs(om)[:, None])


def weighted_gram_int2(X, y, omega):
    """2 M_w in int64 for whole-number rows and weights that are multiples of 0.5: exact."""
    Z = augment(X, y)
    Zi = Z.astype(np.int64)
    o2 = np.asarray(omega, dtype=np.float64) * 2.0
    oi = o2.astype(np.int64)
    assert (Zi == Z).all() and (oi == o2).all()
    return Zi.T @ (Zi * oi[:, None])


def loss_sum(X, y, w, kind):
    z = np.asarray(X, dtype=np.float64) @ w
    if kind == "least_squares":
        return float(np.sum((z - y) ** 2) / 2.0)
    return float(np.sum(np.log1p(np.exp(-np.abs(z))) + np.maximum(-z, 0.0) + (1.0 - y) * z))


def gradient_sum(X, y, w, kind):
    X = np.asarray(X, dtype=np.float64)
    z = X @ w
    if kind == "least_squares":
        return X.T @ (z - y)
    e = np.exp(-np.abs(z))
    sig = np.where(z >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))
    return X.T @ (sig - y)


def hessian_sum(X, w, kind):
    X = np.asarray(X, dtype=np.float64)
    return X.T @ (X * curvature(X, w, kind)[:, None])


def newton(X, y, w0, lam, kind="logistic", num_iterations=25, tol=1e-6):
    """The product's iteration (newton.py) in numpy. Returns a dict: weights, history (f at the weights
    each iteration started from), gnorm (||g|| there), halvings (per iteration) and margins: per
    iteration, for every Armijo test made, |a - b| / max(|a|, |b|) with a = f(w) - f(cand) the decrease
    found and b = c t g.delta the decrease asked for (the test passes when a >= b): how far, relatively,
    the decision was from flipping."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    w = np.array(w0, dtype=np.float64)

    def f(v):
        return loss_sum(X, y, v, kind) / n + 0.5 * lam * float(v @ v)

    out = {"history": [], "gnorm": [], "halvings": [], "margins": []}
    f0 = f(w)
    for _ in range(num_iterations):
        g = gradient_sum(X, y, w, kind) / n + lam * w
        out["history"].append(f0)
        out["gnorm"].append(float(np.linalg.norm(g)))
        H = hessian_sum(X, w, kind) / n + lam * np.eye(d)
        L = np.linalg.cholesky(H)
        delta = np.linalg.solve(L.T, np.linalg.solve(L, g))
        slope = float(g @ delta)
        t, w_new, margins = 1.0, None, []
        for k in range(MAX_HALVINGS + 1):
            cand = w - t * delta
            f1 = f(cand)
            a, b = f0 - f1, ARMIJO_C * t * slope
            margins.append(abs(a - b) / max(abs(a), abs(b)))
            if f1 <= f0 - b:
                w_new = cand
                break
            t *= 0.5
        out["margins"].append(margins)
        if w_new is None:
            out["halvings"].append(MAX_HALVINGS)
            break
        out["halvings"].append(len(margins) - 1)
        diff = float(np.linalg.norm(w_new - w))
        w, f0 = w_new, f1
        if diff < tol * max(float(np.linalg.norm(w)), 1.0):
            break
    out["weights"] = w
    return out


def planted_logistic(n, d, seed, stretch=1.0):
    """Rows and {0, 1} labels drawn from a planted logistic model, so the data is not separable; the
    rows are then stretched (a start away from the optimum saturates more margins, and Newton's full
    step overshoots there)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)) * rng.uniform(0.5, 1.5, size=d)
    w_true = rng.standard_normal(d) / np.sqrt(d)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(X @ w_true)))).astype(np.float64)
    return X * stretch, y
