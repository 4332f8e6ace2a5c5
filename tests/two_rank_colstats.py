"""HipEngine.column_stats at world size 2: two ranks over gloo on one GPU (run by
tests/test_gpu_colstats.py::test_two_ranks as a child process).

usage: python tests/two_rank_colstats.py OUT.json   (env: MASTER_ADDR, MASTER_PORT, PSGD_TEST_P)

Starts two fresh worker processes (torch.multiprocessing spawn); each initialises gloo, builds the
same PartitionedData and calls column_stats() with no engine argument, so the product picks
HipEngine(rank, world=2) on cuda:0: each rank runs its block of partitions, the ranks all-gather
their 1 + 5 d doubles and merge them on the host. Rank 0 writes what both ranks got."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def make_data(n=2500, d=64):
    rng = np.random.default_rng(92)
    X = rng.standard_normal((n, d))
    X[:, 0] = 0.0
    X[:, 1] = 0.1
    X[:, 2] = 1e6 + rng.standard_normal(n)
    X[rng.random((n, d)) < 0.03] = 0.0
    X[:, 1] = 0.1
    y = rng.integers(0, 2, size=n).astype(np.float64)
    return X, y


def worker(rank, world, P, out):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as g
    pkg = g.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        X, y = make_data()
        st = pkg.column_stats(pkg.PartitionedData.parallelize(y, X, P))
        mine = {"count": st.count, "mean": st.mean.tolist(), "variance": st.variance.tolist(),
                "numNonzeros": [int(v) for v in st.numNonzeros], "max": st.max.tolist(), "min": st.min.tolist()}
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
