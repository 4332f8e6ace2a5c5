"""High-precision truths of the per-sample scalar functions (psgd_device.h), in np.longdouble
(x86 extended: 64-bit mantissa, eps 1.08e-19), each in a form without cancellation, and the input
sets that put the device functions at the ends of their ranges. A plain helper module:
tests/test_math_truth.py checks the truths against mpmath, tests/test_gpu_math_edges.py holds the
device functions to them."""
import numpy as np

LD = np.longdouble
LN2 = np.log(LD(2))


def sigmoid_neg(m):
    """1 / (1 + exp(m))  (the reference's Logistic multiplier + y, m = margin = -z)."""
    m = np.asarray(m, LD)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.where(m > 0, np.exp(-np.abs(m)) / (1 + np.exp(-np.abs(m))), 1 / (1 + np.exp(-np.abs(m))))


def logistic_mult(z, y):
    """sigmoid(z) - y without cancellation: y = 1: -1 / (1 + e^z); y = 0: 1 / (1 + e^-z)."""
    z = np.asarray(z, LD)
    y = np.asarray(y, LD)
    return np.where(y > 0, -sigmoid_neg(z), sigmoid_neg(-z))


def softplus(t):
    """log(1 + exp(t)) = max(t, 0) + log1p(exp(-|t|))."""
    t = np.asarray(t, LD)
    with np.errstate(under="ignore", invalid="ignore"):
        return np.where(t > 0, t, 0) + np.log1p(np.exp(-np.abs(t)))


def logistic_loss(z, y):
    """MLlib's LogisticGradient loss: log1pExp(margin) for label 1, log1pExp(margin) - margin for
    label 0, margin = -z; the latter is log1pExp(-margin)."""
    z = np.asarray(z, LD)
    return softplus(np.where(np.asarray(y) > 0, -z, z))


def pow_ld(a, b):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.power(np.asarray(a, LD), np.asarray(b, LD))


# ---------------------------------------------------------------------------------------------
# Input sets
# ---------------------------------------------------------------------------------------------
def neighbours(x, dtype, k=2):
    """x (rounded to dtype) and its k neighbours on either side."""
    out = [dtype(x)]
    lo = hi = dtype(x)
    for _ in range(k):
        lo = np.nextafter(lo, dtype(-np.inf))
        hi = np.nextafter(hi, dtype(np.inf))
        out += [lo, hi]
    return np.array(out, dtype)


def margin_inputs(dtype, seed=0):
    """Margins for the sigmoid / loss functions: every binade of the type from its smallest
    denormal to 2^10 (both signs, the power of two, its neighbours and random mantissas), a
    dense sample of the range around the clamps, the neighbours of the clamp / overflow /
    underflow edges, and the points k ln2 +- ln2/2 where rint(m log2 e) flips."""
    rng = np.random.default_rng(seed)
    f64 = dtype == np.float64
    emin = -1074 if f64 else -149
    span = 760.0 if f64 else 130.0
    parts = []
    e = np.arange(emin, 11)
    p2 = np.ldexp(1.0, e).astype(dtype)
    parts += [p2, np.nextafter(p2, dtype(0)), np.nextafter(p2, dtype(np.inf))]
    mant = rng.uniform(1.0, 2.0, size=(16, e.size))
    parts.append(np.ldexp(mant, e[None, :]).astype(dtype).ravel())
    parts.append(rng.uniform(-span, span, size=150000).astype(dtype))
    parts.append(rng.uniform(-40.0, 40.0, size=20000).astype(dtype))
    edges = [-746.0, -745.13, -708.4, 0.0, 709.0, 709.78, 710.0, 745.13, 746.0, 708.4, -709.0, -709.78, -710.0]
    if not f64:
        edges = [0.0, 87.3, -87.3, 88.7, -88.7, 103.9, -103.9, 16.6, -16.6, 17.3, -17.3]
    for x in edges:
        parts.append(neighbours(x, dtype, 3))
    kmax = 1100 if f64 else 190
    k = np.arange(-kmax, kmax + 1)
    half = (k[None, :] + np.array([-0.5, 0.5])[:, None]) * float(LN2)
    for d in (-2, -1, 0, 1, 2):
        h = half.astype(dtype).ravel()
        for _ in range(abs(d)):
            h = np.nextafter(h, dtype(np.inf if d > 0 else -np.inf))
        parts.append(h)
    x = np.concatenate([np.asarray(p, dtype).ravel() for p in parts])
    x = np.concatenate([x, -x])
    return np.ascontiguousarray(x)


NONFINITE = (np.inf, -np.inf, np.nan)


def normal_binades(dtype, lo_exp, hi_exp, per=48, seed=1):
    """Every binade 2^lo_exp .. 2^hi_exp: the power of two, its upper neighbour, the last value of
    the binade and `per` random mantissas."""
    rng = np.random.default_rng(seed)
    e = np.arange(lo_exp, hi_exp + 1)
    p2 = np.ldexp(1.0, e).astype(dtype)
    top = np.nextafter(np.ldexp(1.0, e[:-1] + 1).astype(dtype), dtype(0))
    mant = rng.uniform(1.0, 2.0, size=(per, e.size))
    r = np.ldexp(mant, e[None, :]).astype(dtype).ravel()
    return np.concatenate([p2, np.nextafter(p2, dtype(np.inf)), top, r])
