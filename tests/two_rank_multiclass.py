"""HipEngine.evaluate_multinomial and confusion at world size 2: two ranks over gloo on one GPU (run
by tests/test_gpu_multiclass.py::test_two_ranks as a child process).

usage: python tests/two_rank_multiclass.py OUT.json   (env: MASTER_ADDR, MASTER_PORT, PSGD_TEST_P)

Starts two fresh worker processes (torch.multiprocessing spawn); each initialises gloo, builds the
same PartitionedData and scores the same weights through evaluate_multinomial() and
MulticlassMetrics.fromModel() with no engine argument, so the product picks HipEngine(rank, world=2)
on cuda:0: each rank scores its block of partitions and the ranks all-gather their sums and tables.
Rank 0 writes what both ranks got."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def make_data(n=2500, d=64, K=5):
    rng = np.random.default_rng(92)
    X = rng.standard_normal((n, d))
    w = rng.standard_normal((K - 1) * d) / np.sqrt(d)
    y = rng.integers(0, K, size=n).astype(np.float64)
    return X, y, w, K


def worker(rank, world, P, out):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as g
    pkg = g.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        X, y, w, K = make_data()
        data = pkg.PartitionedData.parallelize(y, X, P)
        ev = pkg.evaluate_multinomial(data, pkg.LogisticGradient(K), pkg.SimpleSGDUpdater(), 0.0, w)
        table = pkg.MulticlassMetrics.fromModel(data, w, K).table
        mine = {"lossSum": ev.lossSum, "count": ev.count, "nCorrect": ev.nCorrect,
                "partLoss": [float(v) for v in ev.partLoss], "partCorrect": [int(v) for v in ev.partCorrect],
                "table": table.tolist()}
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
