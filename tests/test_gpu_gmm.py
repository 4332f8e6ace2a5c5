"""The Gaussian mixture's passes on the GPU against numpy's long-double restatement (tests/gmm_truth.py,
which has the shapes, the inputs and the bars). Whole numbers in -3 .. 3 make q and the moments of
whole-number responsibilities exact: bit for bit. Real data meets the fp64 bars. A second call and the host
forms return the same bytes."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu

import gmm_truth as GT
from test_gpu_kmeans import blobs
from test_gpu_project import _free_port, dense_data, np_dtype, offsets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")


def check_all(pkg, engine, c, whole, what):
    """Everything the passes promise, on one engine, against the truth of case c."""
    import torch
    X, ops = c["X"], (c["A"], c["b"], c["c"])
    n, d, k = len(X), X.shape[1], len(c["c"])
    a = d + 1
    resp, ll, q = engine.gmm_responsibilities(None, ops, mahalanobis=True)
    resp, q = resp.cpu().numpy(), q.cpu().numpy()
    step = engine.gmm_step(None, ops).cpu().numpy()
    S = step[:-2].reshape(k, a, a)
    S0 = engine.gmm_moments(torch.from_numpy(c["R0"]).to(engine.dev)).cpu().numpy().reshape(k, a, a)
    assert resp.shape == q.shape == (n, k) and step[-1] == n
    assert all(np.isfinite(v).all() for v in (resp, q, step, S0)) and np.isfinite(ll)
    assert (np.abs(resp.sum(axis=1) - 1.0) <= 1e-15 * k).all()
    assert (S == S.transpose(0, 2, 1)).all() and (S0 == S0.transpose(0, 2, 1)).all()
    assert step[-2] == ll
    if whole:
        assert (q == c["q"].astype(np.float64)).all(), f"{what}: q differs at {np.argwhere(q != c['q'].astype(np.float64))[0]}"
        assert (S0 == c["S0"].astype(np.float64)).all()
        assert q[n // 2, 0] == 0.0
        assert (resp[:, k - 1] == resp[:, 0]).all()   # the duplicated component
    else:
        worst = [np.max(np.abs(g - t.astype(np.float64)) / np.maximum(b, 1e-300)) for g, t, b in
                 ((q, c["q"], c["bq"]), (resp, c["r"], c["br"]), (S, c["S"], c["bS"]))]
        print(f"{what}: worst error / bar: q {worst[0]:.3g}, r {worst[1]:.3g}, moments {worst[2]:.3g}, "
              f"loglik {abs(ll - float(c['lnp'].sum())) / c['bl'].sum():.3g}")
        assert GT.inside(q, c["q"], c["bq"]) and GT.inside(resp, c["r"], c["br"]) and GT.inside(S, c["S"], c["bS"])
        assert abs(ll - float(c["lnp"].sum())) <= c["bl"].sum()
        assert GT.inside(S0, c["S0"], GT.moment_bars(X, c["R0"]))
        # the far row: r = 1 / k, ln P = ln(k EPS)
        assert (np.abs(resp[n - 1] - 1.0 / k) <= c["br"][n - 1]).all()
    # the same bytes from call to call, and from the host forms
    resp2, ll2, q2 = engine.gmm_responsibilities(None, ops, mahalanobis=True)
    h_resp, h_ll, h_q = engine.ctx.gmm_responsibilities(*ops, mahalanobis=True)
    for got in ((resp2.cpu().numpy(), q2.cpu().numpy(), ll2, engine.gmm_step(None, ops).cpu().numpy()),
                (h_resp, h_q, h_ll, engine.ctx.gmm_step(*ops))):
        assert got[0].tobytes() == resp.tobytes() and got[1].tobytes() == q.tobytes() and got[2] == ll
        assert got[3].tobytes() == step.tobytes()
    assert engine.gmm_responsibilities(None, ops)[2] is None
    return resp, ll


@pytest.mark.parametrize("whole", [True, False], ids=["whole", "real"])
@pytest.mark.parametrize("d,k,storage", GT.DENSE_DKS, ids=[f"d{d}-k{k}-{s}" for d, k, s in GT.DENSE_DKS])
def test_dense(pkg, d, k, storage, whole):
    """The path is asserted from the plan: dense_lds wherever the packed operands fit a CU's LDS (all but
    the two shapes of 256, whose operands are 512 KiB and 1 MiB)."""
    plan = pkg._native.gmm_plan("dense", storage, d, k, 15)
    assert plan["path"] == GT.expected_path(d, k, storage) == ("dense_l2" if 256 in (d, k) else "dense_lds")
    if (d, k) == (17, 3):   # two blocks a component over chunks of four: component 1 straddles a chunk's end
        assert plan["component_blocks"] == 2 and plan["chunk_blocks"] == 4
    c = GT.case(sum(GT.SIZES), d, k, storage, whole)
    check_all(pkg, pkg.HipEngine(dense_data(pkg, c, GT.SIZES)), c, whole, f"dense d={d} k={k} {storage}")


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_dense_off_lds(pkg, storage):
    """Packed operands too large for LDS (asserted from the plan): the MFMA operands come through L2."""
    d, k = GT.DENSE_OFF_LDS
    assert pkg._native.gmm_plan("dense", storage, d, k, 7)["path"] == "dense_l2"
    sizes = (37, 0, 63)
    for whole in (True, False):
        c = GT.case(sum(sizes), d, k, storage, whole)
        check_all(pkg, pkg.HipEngine(dense_data(pkg, c, sizes)), c, whole, f"off-LDS {storage} whole={whole}")


def test_moments_span_many_tiles(pkg):
    """More tiles than the moments' plan has items: a span is a run of tiles that crosses partitions."""
    d, k, sizes = 3, 2, (50001, 0, 7, 89990, 13)
    n_tiles = sum(-(-s // 16) for s in sizes)
    plan = pkg._native.gmm_plan("dense", "f32", d, k, n_tiles)
    assert n_tiles > plan["items"] and plan["span_tiles"] > 1 and plan["spans"] * plan["span_tiles"] >= n_tiles
    c = GT.case(sum(sizes), d, k, "f32", True)
    check_all(pkg, pkg.HipEngine(dense_data(pkg, c, sizes)), c, True, "many tiles")


@pytest.mark.parametrize("d,storage,ld", [(13, "f32", 16), (30, "f64", 32)])
def test_zero_copy_pitch(pkg, d, storage, ld):
    """Rows with ld > d and NaN in the pad: nothing non-finite comes out of either pass."""
    import torch
    c = GT.case(sum(GT.SIZES), d, 5, storage, False)
    dev = torch.device("cuda", 0)
    o = offsets(GT.SIZES)
    parts = []
    for a, b in zip(o[:-1], o[1:]):
        X = torch.full((b - a, ld), float("nan"), dtype=torch.float32 if storage == "f32" else torch.float64, device=dev)
        X[:, :d] = torch.from_numpy(np.array(c["X"][a:b])).to(dev)
        parts.append(pkg.DevicePartition(torch.zeros(b - a, dtype=torch.float64, device=dev), X, d))
    check_all(pkg, pkg.HipEngine(pkg.PartitionedData(parts)), c, False, f"zero-copy d={d} ld={ld}")


def test_far_rows_and_tiny_weights(pkg):
    """A row 1e3 sigma from every component: r = 1 / k and ln P = ln(k EPS); a component of weight 1e-300:
    finite everywhere. (A row on a mean has q = 0 exactly: every whole case of test_dense asserts it.)"""
    d, k = 5, 3
    rng = np.random.default_rng(41)
    mus = rng.uniform(-1.0, 1.0, size=(k, d))
    X = np.concatenate([mus[rng.integers(0, k, size=40)] + rng.standard_normal((40, d)), np.full((1, d), 1e3)])
    w = np.array([0.5, 0.5 - 1e-300, 1e-300])
    ops = GT.operands(w, mus, [np.eye(d)] * k)
    engine = pkg.HipEngine(pkg.PartitionedData.parallelize(np.zeros(len(X)), X, 2, dtype=np.float64))
    resp, ll, q = engine.gmm_responsibilities(None, ops, mahalanobis=True)
    resp, q = resp.cpu().numpy(), q.cpu().numpy()
    t_q, t_r, t_lnp = GT.estep(X, *ops)
    bq, br, bl = GT.bars(X, *ops, t_r)
    assert np.isfinite(resp).all() and np.isfinite(q).all() and np.isfinite(engine.gmm_step(None, ops).cpu().numpy()).all()
    assert GT.inside(q, t_q, bq) and GT.inside(resp, t_r, br) and abs(ll - float(t_lnp.sum())) <= bl.sum()
    assert (np.abs(resp[-1] - 1.0 / k) <= br[-1]).all()
    far_only = pkg.HipEngine(pkg.PartitionedData.parallelize(np.zeros(1), X[-1:], 1, dtype=np.float64))
    lnp = far_only.gmm_responsibilities(None, ops)[1]
    assert abs(lnp - np.log(k * GT.EPS)) <= 1e-15 * abs(np.log(k * GT.EPS))


def test_errors_and_empty_registry(pkg):
    import torch
    N = pkg._native
    part = pkg.DensePartition(np.zeros(0), np.zeros((0, 5), dtype=np.float32))
    engine = pkg.HipEngine(pkg.PartitionedData([part, part]))
    k, d = 3, 5
    ops = (np.ones((k, d, d)), np.ones((k, d)), np.zeros(k))
    assert (engine.gmm_step(None, ops).cpu().numpy() == 0.0).all() and (engine.ctx.gmm_step(*ops) == 0.0).all()
    resp, ll, _ = engine.gmm_responsibilities(None, ops)
    assert resp.shape == (0, k) and ll == 0.0
    assert (engine.gmm_moments(torch.zeros((0, k), dtype=torch.float64, device=engine.dev)).cpu().numpy() == 0.0).all()
    L, h = N.lib(), engine.ctx.handle
    A, b, c = (torch.from_numpy(v).to(engine.dev).data_ptr() for v in ops)
    keep = torch.zeros(k * 36 + 2 + 3 * k, dtype=torch.float64, device=engine.dev)
    out = keep.data_ptr()
    assert L.psgd_gmm_step_device(h, k, A, b, c, out, None) == 0
    for args in ((None, b, c, out), (A, None, c, out), (A, b, None, out), (A, b, c, None)):
        assert L.psgd_gmm_step_device(h, k, *args, None) == N.PSGD_EINVAL
    assert L.psgd_gmm_step_device(None, k, A, b, c, out, None) == N.PSGD_EINVAL
    assert L.psgd_gmm_step_device(h, 0, A, b, c, out, None) == N.PSGD_EINVAL
    assert L.psgd_gmm_step_device(h, 257, A, b, c, out, None) == N.PSGD_EUNSUPPORTED
    assert L.psgd_gmm_responsibilities_device(h, k, A, b, c, None, None, out, None) == N.PSGD_EINVAL
    assert L.psgd_gmm_responsibilities_device(h, k, A, b, c, out, None, None, None) == N.PSGD_EINVAL
    assert L.psgd_gmm_moments_device(h, k, None, out, None) == N.PSGD_EINVAL
    assert L.psgd_gmm_moments_device(h, 257, out, out, None) == N.PSGD_EUNSUPPORTED
    wide = pkg.HipEngine(pkg.PartitionedData([pkg.DensePartition(np.zeros(2), np.zeros((2, 257), dtype=np.float32))]))
    wide.column_stats()   # (registers the rows)
    assert L.psgd_gmm_moments_device(wide.ctx.handle, k, out, out, None) == N.PSGD_EUNSUPPORTED
    csr = pkg.HipEngine(pkg.PartitionedData([pkg.CsrPartition(np.zeros(1), np.array([0, 1], dtype=np.int64),
                                                               np.zeros(1, dtype=np.int32), np.ones(1), d)]))
    csr.column_stats()
    assert L.psgd_gmm_step_device(csr.ctx.handle, k, A, b, c, out, None) == N.PSGD_EUNSUPPORTED
    with pytest.raises(pkg.IllegalArgumentException, match="dense rows"):
        csr.gmm_step(None, ops)
    fresh = ctypes.c_void_p()
    assert L.psgd_ctx_create(0, ctypes.byref(fresh)) == 0
    try:
        assert L.psgd_gmm_step_device(fresh, k, A, b, c, out, None) == N.PSGD_ESTATE
        assert L.psgd_gmm_moments_device(fresh, k, out, out, None) == N.PSGD_ESTATE
    finally:
        L.psgd_ctx_destroy(fresh)


# ---- end to end -------------------------------------------------------------------------------------
def check_model(pkg, model, data, X, start, tol, max_it):
    w, mus, sigmas, llh, it = GT.em(X, *start, tol, max_it)
    assert model.numIterations == it and 1 < it < max_it
    np.testing.assert_allclose(model.weights, w, rtol=1e-8, atol=0)
    np.testing.assert_allclose(np.stack([g.mu for g in model.gaussians]), mus, rtol=1e-8, atol=0)
    np.testing.assert_allclose(np.stack([g.sigma for g in model.gaussians]), sigmas, rtol=1e-8, atol=1e-12)
    assert abs(model.logLikelihood - llh) <= 1e-9 * abs(llh)
    # every row's best-to-second gap exceeds twice its bar: predict is decided whatever the order of the sums
    ops = GT.operands(model.weights, [g.mu for g in model.gaussians], [g.sigma for g in model.gaussians])
    _, t_r, _ = GT.estep(X, *ops)
    _, br, _ = GT.bars(X, *ops, t_r)
    top = np.sort(t_r.astype(np.float64), axis=1)
    assert (top[:, -1] - top[:, -2] > 2 * br.max(axis=1)).all()
    pred = np.concatenate([t.cpu().numpy() for t in model.predict(data)])
    soft = np.concatenate([t.cpu().numpy() for t in model.predictSoft(data)])
    assert pred.dtype == np.int32 and (pred == np.argmax(t_r, axis=1)).all() and GT.inside(soft, t_r, br)


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_run_matches_the_restatement(pkg, storage):
    X, means = blobs()
    d = X.shape[1]
    data = pkg.PartitionedData.parallelize(np.zeros(len(X)), X, 4, dtype=np_dtype(storage))
    mus = means + 0.3 * np.random.default_rng(1).standard_normal(means.shape)
    start = (np.full(3, 1.0 / 3), mus, np.stack([np.eye(d)] * 3))
    init = pkg.GaussianMixtureModel(start[0], [pkg.MultivariateGaussian(m, s) for m, s in zip(mus, start[2])])
    model = pkg.GaussianMixture(3, 0.01, 100).setInitialModel(init).run(data)
    check_model(pkg, model, data, X, start, 0.01, 100)
    if storage == "f32":
        return
    # from k-means' centres, and on PCA's projected device partitions as they are
    warm = pkg.GaussianMixtureModel.fromKMeans(pkg.KMeans(3, 20).setInitialModel(pkg.KMeansModel(mus)).run(data), data)
    a = np.concatenate([t.cpu().numpy() for t in pkg.KMeansModel(mus).predict(data)])   # (the blobs are far apart:
    for j in range(3):                                                                   #  the assignment is settled)
        np.testing.assert_allclose(warm.gaussians[j].sigma, np.cov(X[a == j].astype(np.float64).T, bias=True), rtol=1e-8, atol=1e-12)
    start_w = (warm.weights, np.stack([g.mu for g in warm.gaussians]), np.stack([g.sigma for g in warm.gaussians]))
    check_model(pkg, pkg.GaussianMixture(3, 0.01, 100).setInitialModel(warm).run(data), data, X, start_w, 0.01, 100)
    proj = pkg.PCA(2).fit(data).transform(data, "f64")
    rows = np.concatenate([p.x.cpu().numpy()[:, :2] for p in proj.partitions])
    init2 = pkg.GaussianMixtureModel.fromKMeans(pkg.KMeans(3, 20, seed=4).run(proj), proj)
    start2 = (init2.weights, np.stack([g.mu for g in init2.gaussians]), np.stack([g.sigma for g in init2.gaussians]))
    m2 = pkg.GaussianMixture(3, 1e-3, 100).setInitialModel(init2).run(proj)
    w2, mu2, s2, llh2, it2 = GT.em(rows, *start2, 1e-3, 100)
    assert m2.numIterations == it2
    np.testing.assert_allclose(np.stack([g.mu for g in m2.gaussians]), mu2, rtol=1e-8, atol=1e-12)


@pytest.mark.parametrize("P", [5, 1])
def test_two_ranks(tmp_path, pkg, P):
    """Two ranks sharing cuda:0 over gloo, each a fresh child process (tests/two_rank_gmm.py): both hold the
    same step and model bytes, within the one-rank bars of the restatement."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import two_rank_gmm as T
    out = str(tmp_path / "res.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), PSGD_TEST_P=str(P))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "two_rank_gmm.py"), out], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    for key in ("step", "weights", "mus", "sigmas", "llh", "iterations"):   # floats survive JSON exactly: identical bits
        assert res["0"][key] == res["1"][key], key
    got = res["0"]
    X, start = T.make_data()
    k, a = T.K, X.shape[1] + 1
    ops = GT.operands(*start)
    _, t_r, t_lnp = GT.estep(X, *ops)
    step = np.array(got["step"])
    assert GT.inside(step[:-2].reshape(k, a, a), GT.moments(X, t_r), GT.moment_bars(X, t_r))
    assert abs(step[-2] - float(t_lnp.sum())) <= GT.bars(X, *ops, t_r)[2].sum() and step[-1] == len(X)
    w, mus, sigmas, llh, it = GT.em(X, *start, 0.01, 100)
    assert got["iterations"] == it and abs(got["llh"] - llh) <= 1e-9 * abs(llh)
    np.testing.assert_allclose(np.array(got["mus"]).reshape(mus.shape), mus, rtol=1e-8, atol=0)
    np.testing.assert_allclose(np.array(got["sigmas"]).reshape(sigmas.shape), sigmas, rtol=1e-8, atol=1e-12)
    assert sum(sum(res[r_]["rows"]) for r_ in ("0", "1")) == len(X)
