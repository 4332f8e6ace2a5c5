"""GaussianMixture at world size 2: two ranks over gloo on one GPU, each a fresh worker process that picks
HipEngine(rank, world=2) on cuda:0 (run by tests/test_gpu_gmm.py::test_two_ranks as a child process;
usage: python tests/two_rank_gmm.py OUT.json; env: MASTER_ADDR, MASTER_PORT, PSGD_TEST_P)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K = 3


def make_data(n=600, d=5):
    """(X, the initial model (weights, mus, sigmas) near the truth)."""
    rng = np.random.default_rng(313)
    means = rng.uniform(-6.0, 6.0, size=(K, d))
    X = np.concatenate([m + rng.standard_normal((n // K, d)) for m in means]).astype(np.float32)
    start = (np.full(K, 1.0 / K), means + 0.3 * rng.standard_normal(means.shape), np.stack([np.eye(d)] * K))
    return X[rng.permutation(len(X))], start


def worker(rank, world, P, out):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as g
    pkg = g.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        X, (w, mus, sigmas) = make_data()
        data = pkg.PartitionedData.parallelize(np.zeros(len(X)), X, P, dtype=np.float32)
        gaussians = [pkg.MultivariateGaussian(m, s) for m, s in zip(mus, sigmas)]
        step = pkg.gmm_step(data, w, gaussians)
        model = pkg.GaussianMixture(K, 0.01, 100).setInitialModel(pkg.GaussianMixtureModel(w, gaussians)).run(data)
        mine = {"rows": [int(t.shape[0]) for t in model.predictSoft(data)],
                "step": np.concatenate([step.moments.ravel(), [step.logLikelihood, step.count]]).tolist(),
                "weights": model.weights.tolist(), "mus": np.stack([g_.mu for g_ in model.gaussians]).ravel().tolist(),
                "sigmas": np.stack([g_.sigma for g_ in model.gaussians]).ravel().tolist(),
                "llh": model.logLikelihood, "iterations": model.numIterations}
        if rank == 1:
            with open(out + ".r1", "w") as f:
                json.dump(mine, f)
        dist.barrier()
        if rank == 0:
            with open(out + ".r1") as f:
                other = json.load(f)
            with open(out, "w") as f:
                json.dump({"0": mine, "1": other}, f)
    finally:
        dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    out = sys.argv[1]
    P = int(os.environ.get("PSGD_TEST_P", "5"))
    mp.start_processes(worker, args=(2, P, out), nprocs=2, start_method="spawn")


if __name__ == "__main__":
    main()
