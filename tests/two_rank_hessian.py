"""The weighted Gramian and Newton's method at world size 2: two ranks over gloo on one GPU (run by
tests/test_gpu_hessian.py::test_two_ranks as a child process).

usage: python tests/two_rank_hessian.py OUT.json   (env: MASTER_ADDR, MASTER_PORT)

Starts two fresh worker processes (torch.multiprocessing spawn); each initialises gloo, builds the
same PartitionedData -- five partitions, the second of them empty, so one rank holds the empty one --
and calls gramian(weights=) and runNewton with no engine argument, so the product picks
HipEngine(rank, world=2) on cuda:0: each rank takes its slice of the weights and its rows' curvature,
the ranks all-gather their matrices and add them in rank order. Rank 0 writes what both ranks got."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

SIZES = (100, 0, 250, 150, 200)
LAM, START = 0.1, 2.0


def make_data(d=21):
    import hessian_truth as HT
    X, y = HT.planted_logistic(sum(SIZES), d, 97, stretch=2.0)
    om = np.random.default_rng(98).uniform(0.0, 2.0, size=sum(SIZES))
    om[::17] = 0.0
    return X, y, om


def worker(rank, world, out):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as g
    pkg = g.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        X, y, om = make_data()
        offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(int)
        data = pkg.PartitionedData([pkg.DensePartition(np.ascontiguousarray(y[a:b]), np.ascontiguousarray(X[a:b]))
                                    for a, b in zip(offs[:-1], offs[1:])])
        w, hist = pkg.runNewton(data, pkg.LogisticGradient(), pkg.SquaredL2SGDUpdater(), 25, LAM,
                                np.full(X.shape[1], START))
        mine = {"matrix": pkg.gramian(data, weights=om).matrix.ravel().tolist(),
                "weights": w.tolist(), "history": hist.tolist()}
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
    mp.start_processes(worker, args=(2, out), nprocs=2, start_method="spawn")


if __name__ == "__main__":
    main()
