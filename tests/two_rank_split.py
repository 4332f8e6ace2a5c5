"""randomSplit / kFold at world size 2: two ranks over gloo on one GPU (run by
tests/test_gpu_data_split.py::test_two_ranks as a child process).

usage: python tests/two_rank_split.py OUT.json   (env: MASTER_ADDR, MASTER_PORT)

Starts two fresh worker processes (torch.multiprocessing spawn); each initialises gloo, builds the
same PartitionedData of P = 5 tagged partitions and splits it with no engine argument, so the
product picks HipEngine(rank, world=2) on cuda:0: each rank selects and compacts its own block of
partitions, seeded by their global indices, and the ranks all-gather the counts. Rank 0 writes what
both ranks got: per split and partition the kept rows' tags (empty for another rank's partitions)
and partition_counts."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

P, N_ROWS, D = 5, 3001, 6
WEIGHTS, SEED = [0.6, 0.4], 11
FOLDS, FOLD_SEED = 3, 7


def slices():
    return [((i * N_ROWS) // P, ((i + 1) * N_ROWS) // P) for i in range(P)]


def make_data():
    """x[t, 1] is the row's position in its partition."""
    rng = np.random.default_rng(77)
    X = rng.standard_normal((N_ROWS, D))
    for a, b in slices():
        X[a:b, 1] = np.arange(b - a)
    y = rng.integers(0, 2, size=N_ROWS).astype(np.float64)
    return X, y


def tags(data):
    return [[int(v) for v in q.x.detach().cpu().numpy()[:, 1]] for q in data.partitions]


def worker(rank, world, out):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as g
    pkg = g.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        X, y = make_data()
        data = pkg.PartitionedData.parallelize(y, X, P)
        split = pkg.randomSplit(data, WEIGHTS, SEED)
        folds = pkg.kFold(data, FOLDS, FOLD_SEED)
        mine = {"block": list(pkg.shard_range(P, rank, world)),
                "split": [tags(s) for s in split],
                "split_counts": [[int(v) for v in s.partition_counts] for s in split],
                "folds": [[tags(tr), tags(va)] for tr, va in folds],
                "fold_counts": [[[int(v) for v in tr.partition_counts], [int(v) for v in va.partition_counts]]
                                for tr, va in folds]}
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
