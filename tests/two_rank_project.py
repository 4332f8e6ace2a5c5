"""HipEngine.project and PCA.fit at world size 2: two ranks over gloo on one GPU (run by
tests/test_gpu_project.py::test_two_ranks as a child process).

usage: python tests/two_rank_project.py OUT.json   (env: MASTER_ADDR, MASTER_PORT, PSGD_TEST_P)

Starts two fresh worker processes (torch.multiprocessing spawn); each initialises gloo, builds the
same PartitionedData and calls multiply() and PCA.fit with no engine argument, so the product picks
HipEngine(rank, world=2) on cuda:0: each rank projects its block of partitions and holds empty
placeholders for the other's. Rank 0 writes what both ranks got."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def make_data(n=700, d=21, k=5):
    rng = np.random.default_rng(197)
    X = (rng.standard_normal((n, d)) * (1.4 ** -np.arange(d))).astype(np.float32)
    y = rng.standard_normal(n)
    B = rng.standard_normal((d, k))
    return X, y, B


def worker(rank, world, P, out):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as g
    pkg = g.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        X, y, B = make_data()
        data = pkg.PartitionedData.parallelize(y, X, P, dtype=np.float32)
        lo, hi = pkg.shard_range(P, rank, world)
        mine = {"block": [lo, hi]}
        for storage in ("f32", "f64"):
            res = pkg.multiply(data, B, storage)
            mine["counts"] = [int(c) for c in res.partition_counts]
            mine["rows"] = [p.n_rows for p in res.partitions]
            mine[storage] = [float(v) for p in res.partitions for v in p.x[:, :B.shape[1]].cpu().numpy().ravel()]
            mine["labels"] = [float(v) for p in res.partitions for v in p.labels.cpu().numpy()]
        mine["pc"] = pkg.PCA(3).fit(data).pc.ravel().tolist()
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
