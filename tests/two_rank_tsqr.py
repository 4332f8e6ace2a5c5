"""HipEngine.tsqr at world size 2: two ranks over gloo on one GPU (run by
tests/test_gpu_tsqr.py::test_two_ranks as a child process).

usage: python tests/two_rank_tsqr.py OUT.json   (env: MASTER_ADDR, MASTER_PORT)

Starts two fresh worker processes (torch.multiprocessing spawn); each initialises gloo, builds the
same PartitionedData and calls qr_factor() with no engine argument, so the product picks
HipEngine(rank, world=2) on cuda:0: each rank factors its block of partitions, the ranks all-gather
their R factors and factor the stack in rank order. Rank 0 writes what both ranks got."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def make_data(n=700, d=21):
    rng = np.random.default_rng(98)
    X = rng.standard_normal((n, d)).astype(np.float32)
    y = rng.standard_normal(n)
    return X, y


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
        data = pkg.PartitionedData.parallelize(y, X, 5)
        mine = {"matrix": pkg.qr_factor(data).matrix.ravel().tolist()}
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
