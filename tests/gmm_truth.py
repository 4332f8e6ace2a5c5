"""A Gaussian mixture's EM step in numpy long double: the restatement the GPU tests compare against
(include/psgd.h has the definitions), with the shapes, the inputs and the fp64 bars of
tests/test_gpu_gmm.py. case() checks once, on the CPU, that a float64 evaluation in another summation
order stays inside every bar for the inputs it makes."""
import functools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52

# d around the 4-, 8- and 16-feature steps and one column block, k around one chunk of four blocks;
# (17, 3): two blocks a component, the second component straddles the first chunk's end; (20, 17): 34 blocks
DENSE_DKS = ((1, 2, "f64"), (3, 1, "f32"), (4, 16, "f32"), (13, 5, "f64"), (16, 4, "f32"), (17, 3, "f64"),
             (33, 3, "f32"), (20, 17, "f64"), (8, 256, "f32"), (256, 2, "f64"))
DENSE_OFF_LDS = (32, 24)
SIZES = (1, 3, 0, 15, 16, 17, 65, 53)


def expected_path(d, k, storage):
    """The rule of psgd_gmm_plan: the packed operands (d rounded up to whole steps of four 16-byte vectors
    x 16 k ceil(d / 16) doubles) and eight waves' staging (16 k + 16 doubles each) fit 160 KiB."""
    step = 16 if storage == "f32" else 8
    dpad = -(-d // step) * step
    return "dense_lds" if 8 * (dpad * 16 * k * -(-d // 16) + 8 * (16 * k + 16)) <= 160 * 1024 else "dense_l2"


def constants(mu, sigma):
    """(R, u) of MultivariateGaussian: float64 eigh as the host does it, the rest in long double."""
    d = len(mu)
    s, U = np.linalg.eigh(0.5 * (np.asarray(sigma, dtype=np.float64) + np.asarray(sigma, dtype=np.float64).T))
    keep = s > EPS * d * s.max()
    assert keep.any(), "covariance matrix has no non-zero singular values"
    root = np.where(keep, 1 / np.sqrt(np.where(keep, s, 1.0).astype(LD)), LD(0))
    return root[:, None] * U.T.astype(LD), -(d * np.log(2 * LD(np.pi)) + np.log(s[keep].astype(LD)).sum()) / 2


def operands(weights, mus, sigmas):
    """(A [k, d, d], b [k, d], c [k]) in float64: what the device receives."""
    Ru = [constants(m, s) for m, s in zip(mus, sigmas)]
    A = np.stack([R.T for R, _ in Ru]).astype(np.float64)
    b = np.stack([R.astype(np.float64) @ np.asarray(m, dtype=np.float64) for (R, _), m in zip(Ru, mus)])
    c = np.log(np.asarray(weights, dtype=np.float64)) + np.array([float(u) for _, u in Ru])
    return A, b, c


def estep(X, A, b, c, dtype=LD):
    """(q [n, k], r [n, k], ln P [n]) in `dtype`."""
    X, A, b, c = (np.asarray(v, dtype=dtype) for v in (X, A, b, c))
    v = np.einsum("ni,kic->nkc", X, A) - b[None]
    q = (v * v).sum(axis=2)
    p = dtype(EPS) + np.exp(c[None] - q / 2)
    P = p.sum(axis=1)
    return q, p / P[:, None], np.log(P)


def moments(X, r, dtype=LD):
    """S [k, d + 1, d + 1] = sum_rows r_j z z^T, z = [x, 1]."""
    Z = np.concatenate([np.asarray(X, dtype=dtype), np.ones((len(X), 1), dtype=dtype)], axis=1)
    return np.einsum("nk,na,nb->kab", np.asarray(r, dtype=dtype), Z, Z)


def m_step(S):
    """(weights, mus, sigmas) from the moments, in their dtype."""
    d = S.shape[1] - 1
    W = S[:, d, d]
    mus = S[:, :d, d] / W[:, None]
    return W / W.sum(), mus, S[:, :d, :d] / W[:, None, None] - mus[:, :, None] * mus[:, None, :]


def em(X, weights, mus, sigmas, convergenceTol, maxIterations):
    """GaussianMixture.run: (weights, mus, sigmas, log-likelihood, iterations); a model is handed on in float64."""
    llh, prev, it = -np.finfo(np.float64).max, 0.0, 0
    while it < maxIterations and abs(llh - prev) > convergenceTol:
        _, r, lnp = estep(X, *operands(weights, mus, sigmas))
        weights, mus, sigmas = (v.astype(np.float64) for v in m_step(moments(X, r)))
        prev, llh, it = llh, float(lnp.sum()), it + 1
    return weights, mus, sigmas, llh, it


def bars(X, A, b, c, r):
    """The fp64 bars on the sums of magnitudes: (q [n, k], r [n, k], ln P [n]). q: 1e-9 sum_c (|b_c| + sum_i
    |x_i A[i][c]|)^2; p_j is then off by bar_q / 2 + 1e-9 relative (rel_j), so ln P by sum_i r_i rel_i and r_j
    by r_j (rel_j + sum_i r_i rel_i)."""
    X, A, b, r = (np.abs(np.asarray(v, dtype=np.float64)) for v in (X, A, b, r))
    bq = 1e-9 * ((np.einsum("ni,kic->nkc", X, A) + b[None]) ** 2).sum(axis=2)
    rel = bq / 2 + 1e-9
    mean = (r * rel).sum(axis=1)
    return bq, r * (rel + mean[:, None]), mean


def moment_bars(X, r):
    """1e-9 sum |r| |z_a z_b|."""
    return 1e-9 * moments(np.abs(np.asarray(X, dtype=np.float64)), np.abs(np.asarray(r, dtype=np.float64)), np.float64)


def inside(got, want, bar):
    return bool((np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want).astype(np.float64)) <= bar).all())


@functools.lru_cache(maxsize=None)
def case(n, d, k, storage, whole):
    """The inputs of a test and their truth: X (rows in the storage type), A, b, c, whole-number
    responsibilities R0, and q, r, lnp, S (of r), S0 (of R0) with the bars of the real case."""
    rng = np.random.default_rng(8200 + 13 * d + k + (3 if storage == "f32" else 0) + (100000 if whole else 0))
    dt = np.float32 if storage == "f32" else np.float64
    if whole:
        X = rng.integers(-3, 4, size=(n, d)).astype(dt)
        A = rng.integers(-3, 4, size=(k, d, d)).astype(np.float64)
        b = rng.integers(-3, 4, size=(k, d)).astype(np.float64)
        c = -0.25 * np.arange(k)
        X[n // 2] = 0.0
        b[0] = 0.0                                        # a row on a mean: q = 0
        A[k - 1], b[k - 1], c[k - 1] = A[0], b[0], c[0]   # two bitwise-equal components
    else:
        mus = rng.uniform(-2.0, 2.0, size=(k, d))
        sigmas, roots = [], []
        for _ in range(k):
            Q = np.linalg.qr(rng.standard_normal((d, d)))[0]
            s = rng.uniform(0.5, 2.0, size=d)
            sigmas.append((Q * s) @ Q.T)
            roots.append(Q * np.sqrt(s))
        w = rng.uniform(0.5, 1.5, size=k)
        A, b, c = operands(w / w.sum(), mus, sigmas)
        j = rng.integers(0, k, size=n)
        X = (mus[j] + np.einsum("nab,nb->na", np.stack(roots)[j], rng.standard_normal((n, d)))).astype(dt)
        X[n - 1] = 1e3   # a far row: r = 1 / k
    R0 = rng.integers(0, 4, size=(n, k)).astype(np.float64)
    q, r, lnp = estep(X, A, b, c)
    out = {"X": X, "y": np.zeros(n), "A": A, "b": b, "c": c, "R0": R0, "q": q, "r": r, "lnp": lnp,
           "S": moments(X, r), "S0": moments(X, R0)}
    if not whole:
        out["bq"], out["br"], out["bl"] = bars(X, A, b, c, r)
        out["bS"] = moment_bars(X, r)
        # float64 in numpy's (pairwise, BLAS) orders stays inside every bar: the bars are not too tight
        q64, r64, l64 = estep(X, A, b, c, np.float64)
        assert inside(q64, q, out["bq"]) and inside(r64, r, out["br"]) and inside(l64, lnp, out["bl"])
        assert inside(moments(X, r64, np.float64), out["S"], out["bS"])
    return out
