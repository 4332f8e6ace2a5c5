"""The multinomial batch gradient on the fp64 matrix cores (method="mfma": grad_mn_rowmult_mfma and
grad_mn_wsum_mfma) against tests/multinomial_grad_truth.py.

The data is test_gpu_gradient_mn.py's dense_case, and so are the bars: every (c, j): |G - ref| <= 1e-9
A[c, j] with A = sum_i |mult_ic x_ij|; lossSum within 1e-9 relative; count exact; on the truth, before
each comparison, the precondition pre <= 1e-10 A (margins summed in another order cannot move a
multiplier far enough to reach the bar). Every case also asks a second call and the host-pointer form
for the same bytes."""
import functools

import numpy as np
import pytest

from conftest import has_gpu

import multinomial_grad_truth as GT
import psgd_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    for name in ("PSGD_GRAD_MN_TWO_PASS", "PSGD_GRAD_MN_FUSE_ALL", "PSGD_GRAD_MN_RANGE"):
        monkeypatch.delenv(name, raising=False)


def plan(pkg, storage, d, K):
    return pkg._native.gradient_multinomial_plan("dense", storage, d, K, method="mfma")


def truth_of(rows, ys, w, K, d):
    t = GT.gradient(rows, ys, w, K, d)
    assert np.all(t.pre <= 1e-10 * t.A), "the multipliers' error could reach the bar"
    return t


def check_sums(got, t, what, bar=1e-9):
    n = t.G.size
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (n + 2,) and np.isfinite(got).all(), what
    assert got[n + 1] == t.count, (what, got[n + 1], t.count)
    err, A = np.abs(got[:n] - t.G.ravel()), t.A.ravel()
    worst = float(np.max(err / np.where(A > 0, A, 1.0)))
    lrel = abs(got[n] - t.lossSum) / abs(t.lossSum)
    print(f"{what}: worst |G - ref| / A {worst:.3g}, lossSum rel {lrel:.3g}, count {t.count}")
    assert np.all(err <= bar * A), (what, int(np.argmax(err - bar * A)), worst)
    assert lrel <= 1e-9, (what, got[n], t.lossSum)


@functools.lru_cache(maxsize=None)
def dense_case(d, storage, K, sizes, labels=None, tie=False):
    rng = np.random.default_rng(5200 + 7 * d + K + (9 if storage == "f32" else 0))
    n = sum(sizes)
    X = rng.standard_normal((n, d)).astype(np.float32 if storage == "f32" else np.float64)
    X[rng.random((n, d)) < 0.05] = 0.0
    W = 0.5 * rng.standard_normal((K - 1, d)) / np.sqrt(d)
    y = rng.integers(0, K, size=n).astype(np.float64)
    if labels is not None:
        y = np.array([labels[k % len(labels)] for k in range(n)], dtype=np.float64)
    if tie:
        # class blocks 1, 2 and 17 are one block: equal margins in two lanes of one MFMA block and in the
        # same lane of two blocks. Every block lies near a positive multiple of one direction u, theirs the
        # largest: where x . u > 0 the tied margin is the maximum and positive (the shifted branch), where
        # x . u < 0 every margin is negative; the rows are scaled so that both happen at several sizes
        u = W[1].copy()
        W[:] = (0.2 + 0.05 * np.arange(K - 1))[:, None] * u + 0.01 * W
        W[2] = W[17] = W[1] = 8.0 * u
        X *= np.array([1.0, -1.0, 4.0, -4.0, 0.25], dtype=X.dtype)[np.arange(n) % 5][:, None]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    rows = X.astype(np.float64)
    return {"X": X, "y": y, "w": W.ravel(), "offs": offs, "rows": rows, "truth": truth_of(rows, y, W.ravel(), K, d)}


def dense_data(pkg, c):
    return pkg.PartitionedData([pkg.DensePartition(np.ascontiguousarray(c["y"][a:b]), np.ascontiguousarray(c["X"][a:b]))
                                for a, b in zip(c["offs"][:-1], c["offs"][1:])])


def run_mfma(pkg, c, K, what, data=None):
    engine = pkg.HipEngine(data or dense_data(pkg, c))
    got = engine.gradient_sum_multinomial(K, c["w"], method="mfma").cpu().numpy()
    check_sums(got, c["truth"], what)
    assert got.tobytes() == engine.gradient_sum_multinomial(K, c["w"], method="mfma").cpu().numpy().tobytes()
    assert got.tobytes() == engine.ctx.gradient_sum_multinomial(K, c["w"], method="mfma").tobytes()
    return engine, got


def sizes_of(pkg, d, storage):
    tile = plan(pkg, storage, d, 3)["tile_rows"]
    return (0, 1, 15, 16, 17, 65) + ((3 * tile + 37,) if d <= 100 else ())


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [1, 3, 100, 130])
@pytest.mark.parametrize("K", [3, 17, 18, 65])
def test_class_and_feature_geometry(pkg, K, d, storage):
    p = plan(pkg, storage, d, K)
    assert p["path"] == "mfma" and p["weights_in_lds"] == 1 and p["class_blocks"] == (K + 14) // 16
    run_mfma(pkg, dense_case(d, storage, K, sizes_of(pkg, d, storage)), K, f"mfma d={d} {storage} K={K}")


def test_packed_w_through_l2(pkg):
    K, d = 65, 324
    assert plan(pkg, "f32", d, K)["weights_in_lds"] == 0
    run_mfma(pkg, dense_case(d, "f32", K, (1, 65, 257)), K, "mfma W through L2")


def test_labels_that_are_no_class(pkg):
    K = 4
    labels = (0.0, 1.0, float(K - 1), float(K), -1.0, 2.5)
    run_mfma(pkg, dense_case(7, "f64", K, (150,), labels=labels), K, "mfma labels")


def test_ties_and_the_shifted_branch(pkg):
    K, d = 19, 3
    c = dense_case(d, "f32", K, (0, 1, 65, 257), tie=True)
    Mg = c["rows"] @ c["w"].reshape(K - 1, d).T
    top = Mg.max(axis=1)
    tied = (Mg[:, 1] == top) & (Mg[:, 2] == top) & (Mg[:, 17] == top)
    assert np.array_equal(Mg[:, 1], Mg[:, 2]) and np.array_equal(Mg[:, 1], Mg[:, 17])
    assert (tied & (top > 0)).sum() >= 10 and (~tied & (top < 0)).sum() >= 10
    run_mfma(pkg, c, K, "mfma ties")


@pytest.mark.parametrize("d,ld", [(3, 8), (100, 104)])
def test_zero_copy_pad_columns(pkg, d, ld):
    """Device-registered rows at a pitch ld > d with NaN in the pad: it reaches no MFMA."""
    import torch
    K = 10
    c = dense_case(d, "f32", K, (1, 65, 70))
    dev = torch.device("cuda", 0)
    parts = []
    for a, b in zip(c["offs"][:-1], c["offs"][1:]):
        X = torch.full((b - a, ld), float("nan"), dtype=torch.float32, device=dev)
        X[:, :d] = torch.from_numpy(c["X"][a:b]).to(dev)
        parts.append(pkg.DevicePartition(torch.from_numpy(c["y"][a:b]).to(dev), X, d))
    run_mfma(pkg, c, K, f"mfma zero-copy d={d} ld={ld}", data=pkg.PartitionedData(parts))


def test_sampled_batch(pkg):
    K, d, fraction, iteration = 10, 100, 0.5, 3
    c = dense_case(d, "f32", K, sizes_of(pkg, d, "f32"))
    engine = pkg.HipEngine(dense_data(pkg, c))
    mfma = engine.gradient_sum_multinomial(K, c["w"], fraction, iteration, method="mfma").cpu().numpy()
    auto = engine.gradient_sum_multinomial(K, c["w"], fraction, iteration, method="auto").cpu().numpy()
    assert 0 < auto[-1] < c["truth"].count and mfma[-1:].tobytes() == auto[-1:].tobytes()
    A = c["truth"].A.ravel()          # sums of absolute terms over every row: they bound the batch's
    assert np.all(np.abs(mfma[:-2] - auto[:-2]) <= 2e-9 * A)
    assert abs(mfma[-2] - auto[-2]) <= 2e-9 * abs(auto[-2])
    # and against the truth on the sampled rows themselves
    seeds = R.partition_seeds(42 + iteration, len(c["offs"]) - 1)
    keep = [a + t for p, (a, b) in enumerate(zip(c["offs"][:-1], c["offs"][1:]))
            for t in R.bernoulli_sample(seeds[p], b - a, fraction)]
    check_sums(mfma, truth_of(c["rows"][keep], c["y"][keep], c["w"], K, d), "mfma sampled")


@pytest.mark.parametrize("K", [10, 40])
def test_row_ranges_do_not_change_a_bit(pkg, K, monkeypatch):
    """K = 40: a record covers 4 tiles, so ranges of 2 and 1 tiles continue from the span's record."""
    d = 20
    p = plan(pkg, "f32", d, K)
    assert p["span"] == (4 if K == 40 else 1) and p["range"] > 16
    c = dense_case(d, "f32", K, (5 * p["tile_rows"] + 37, 0, 2 * p["tile_rows"] + 1, 3))
    engine, whole = run_mfma(pkg, c, K, f"mfma ranges K={K}")
    for r in (8, 2, 1):
        monkeypatch.setenv("PSGD_GRAD_MN_RANGE", str(r))
        assert plan(pkg, "f32", d, K)["range"] == r
        assert engine.gradient_sum_multinomial(K, c["w"], method="mfma").cpu().numpy().tobytes() == whole.tobytes(), r


def test_unserved_shape_names_the_limit(pkg):
    c = dense_case(3, "f32", 3, (5,))
    engine = pkg.HipEngine(dense_data(pkg, c))
    with pytest.raises(pkg.UnsupportedOperationException, match="numClasses <= 65"):
        engine.gradient_sum_multinomial(66, np.zeros(65 * 3), method="mfma")


def test_gradient_descent_with_mfma(pkg):
    """Three iterations against a numpy loop over the truth's gradient (SimpleSGDUpdater: w -= step /
    sqrt(i) G / count), at the bar test_gpu_gradient_mn.py's GradientDescent test holds: 1e-9 relative
    with a floor of 1e-12."""
    K, d, step = 10, 100, 0.5
    c = dense_case(d, "f64", K, (0, 1, 65, 150))
    w = np.linspace(-0.2, 0.2, (K - 1) * d)
    w_ref, h_ref = w.copy(), []
    for i in range(1, 4):
        t = GT.gradient(c["rows"], c["y"], w_ref, K, d)
        h_ref.append(t.lossSum / t.count)
        w_ref = w_ref - step / np.sqrt(i) * t.G.ravel() / t.count
    gd = pkg.GradientDescent(pkg.LogisticGradient(K), pkg.SimpleSGDUpdater()).setStepSize(step).setNumIterations(3) \
        .setConvergenceTol(0.0).setMultinomialMethod("mfma")
    data = dense_data(pkg, c)
    got, h = pkg.GradientDescent.runMiniBatchSGDMultinomial(data, gd.gradient, gd.updater, step, 3, 0.0, 1.0, w, 0.0,
                                                            method="mfma")
    for a, b, what in ((h, h_ref, "history"), (got, w_ref, "weights"), (gd.optimize(data, w), w_ref, "optimize")):
        diff = np.abs(np.asarray(a) - np.asarray(b))
        assert np.all((diff <= 1e-9 * np.maximum(np.abs(a), np.abs(b))) | (diff <= 1e-12)), what
