"""DecisionTree.trainRegressor at world size 2: two ranks over gloo on cuda:0, each a fresh worker process (run by
tests/test_gpu_tree_regression.py::test_two_ranks; usage: python tests/two_rank_tree_reg.py OUT.json; env: MASTER_ADDR,
MASTER_PORT)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P = 5


def worker(rank, world, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as g
    from test_tree_regression_api import waves
    pkg = g.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        X, y = waves()
        data = pkg.PartitionedData.parallelize(y, X, P, dtype=np.float32)
        model = pkg.DecisionTree.trainRegressor(data, maxDepth=4, maxBins=16, minInstancesPerNode=10)
        mine = {"nodes": {k: v.tolist() for k, v in model.nodes.items()}}
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


if __name__ == "__main__":
    import torch.multiprocessing as mp
    mp.start_processes(worker, args=(2, sys.argv[1]), nprocs=2, start_method="spawn")
