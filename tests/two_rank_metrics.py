"""BinaryClassificationMetrics.fromModel at world size 2: two ranks over gloo on one GPU (run by
tests/test_gpu_metrics.py::test_two_ranks as a child process).

usage: python tests/two_rank_metrics.py OUT.json   (env: MASTER_ADDR, MASTER_PORT)

Starts two fresh worker processes (torch.multiprocessing spawn); each initialises gloo, builds the
same PartitionedData and asks for the metrics of the same weights with no engine argument, so the
product picks HipEngine(rank, world=2) on cuda:0: each rank scores its block of partitions, the
ranks all-gather their padded scores and labels, and each runs the array form over the whole.
Rank 0 writes what both ranks got."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PARTS = 5   # rank 0 holds three partitions, rank 1 two: the padding of the all-gather is used


def make_data(n=2500, d=48):
    rng = np.random.default_rng(92)
    X = rng.standard_normal((n, d))
    w = rng.standard_normal(d) / np.sqrt(d)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(X @ w)))).astype(np.float64)
    return X, y, w


def summarize(m):
    """Every output, floating-point values as their bit patterns."""
    thr, cp, cn = m.cumulativeCounts()
    bits = lambda v: int(np.float64(v).view(np.uint64))
    return {"G": m.numThresholds, "P": m.numPositives, "N": m.numNegatives, "rocNumerator": m.rocNumerator,
            "thresholds": [int(v) for v in thr.view(np.uint64)], "cumPos": [int(v) for v in cp],
            "cumNeg": [int(v) for v in cn], "areaUnderROC": bits(m.areaUnderROC()),
            "areaUnderPR": bits(m.areaUnderPR())}


def worker(rank, world, out):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as g
    pkg = g.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        X, y, w = make_data()
        data = pkg.PartitionedData.parallelize(y, X, PARTS)
        mine = summarize(pkg.BinaryClassificationMetrics.fromModel(data, w))
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
    mp.start_processes(worker, args=(2, sys.argv[1]), nprocs=2, start_method="spawn")


if __name__ == "__main__":
    main()
