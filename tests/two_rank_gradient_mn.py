"""HipEngine.gradient_sum_multinomial and GradientDescent.runMiniBatchSGDMultinomial at world size 2:
two ranks over gloo on one GPU (run by tests/test_gpu_gradient_mn.py::test_two_ranks as a child
process, as tests/two_rank_gradient.py is).

usage: python tests/two_rank_gradient_mn.py OUT.json   (env: MASTER_ADDR, MASTER_PORT, PSGD_TEST_P)

Each rank builds the same PartitionedData and calls gradient_sum_multinomial() and
runMiniBatchSGDMultinomial() with no engine argument; the ranks all-gather their (K - 1) d + 2
doubles and add them in rank order. Rank 0 writes what both ranks got."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

K = 4
GD_ARGS = (1.0, 5, 0.01, 1.0)   # stepSize, numIterations, regParam, miniBatchFraction


def make_data(n=700, d=24):
    rng = np.random.default_rng(94)
    X = rng.standard_normal((n, d))
    X[rng.random((n, d)) < 0.05] = 0.0
    w = (0.5 * rng.standard_normal((K - 1, d)) / np.sqrt(d)).ravel()
    y = rng.integers(0, K, size=n).astype(np.float64)
    return X, y, w


def worker(rank, world, P, out):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as g
    pkg = g.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        X, y, w = make_data()
        data = pkg.PartitionedData.parallelize(y, X, P)
        gs = pkg.gradient_sum_multinomial(data, pkg.LogisticGradient(K), w)
        wts, hist = pkg.GradientDescent.runMiniBatchSGDMultinomial(data, pkg.LogisticGradient(K),
                                                                   pkg.SquaredL2SGDUpdater(), *GD_ARGS, w, 0.0)
        mine = {"sum": gs.gradient.tolist() + [gs.lossSum, float(gs.count)], "weights": wts.tolist(),
                "history": hist.tolist()}
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
