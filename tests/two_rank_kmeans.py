"""KMeans at world size 2: two ranks over gloo on one GPU, each a fresh worker process that picks
HipEngine(rank, world=2) on cuda:0 (run by tests/test_gpu_kmeans.py::test_two_ranks as a child process;
usage: python tests/two_rank_kmeans.py OUT.json; env: MASTER_ADDR, MASTER_PORT, PSGD_TEST_P)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K, SEED = 3, 6


def make_data(n=600, d=5):
    rng = np.random.default_rng(311)
    means = rng.uniform(-8.0, 8.0, size=(K, d))
    X = np.concatenate([m + rng.standard_normal((n // K, d)) for m in means]).astype(np.float32)
    return X[rng.permutation(len(X))], means


def worker(rank, world, P, out):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as g
    pkg = g.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        X, means = make_data()
        data = pkg.PartitionedData.parallelize(np.zeros(len(X)), X, P, dtype=np.float32)
        lo, hi = pkg.shard_range(P, rank, world)
        step = pkg.kmeans_step(data, means)
        model = pkg.KMeans(K, 20, 1e-4, seed=SEED).run(data)
        start = pkg.KMeans(K, 0, seed=SEED).run(data).clusterCenters
        pred = model.predict(data)
        mine = {"block": [lo, hi], "rows": [int(t.numel()) for t in pred],
                "pred": [int(v) for t in pred for v in t.cpu().numpy()],
                "step": np.concatenate([step.sums.ravel(), step.counts, [step.cost, step.count]]).tolist(),
                "start": start.ravel().tolist(), "centres": model.clusterCenters.ravel().tolist(),
                "cost": model.trainingCost, "iterations": model.numIterations}
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
