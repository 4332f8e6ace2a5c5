"""RandomForest at world size 2: two ranks over gloo on cuda:0, each a fresh worker process (run by
tests/test_gpu_forest.py::test_two_ranks; usage: python tests/two_rank_forest.py OUT.json; env: MASTER_ADDR, MASTER_PORT)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P = 5
ARGS = dict(numTrees=4, featureSubsetStrategy="sqrt", maxDepth=3, maxBins=16, seed=11, minInstancesPerNode=10)


def worker(rank, world, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as g
    from test_tree_api import blobs
    pkg = g.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        X, y = blobs()
        data = pkg.PartitionedData.parallelize(y, X, P, dtype=np.float32)
        model = pkg.RandomForest.trainClassifier(data, 3, **ARGS)
        mine = {"trees": [{k: v.tolist() for k, v in t.nodes.items()} for t in model.trees]}
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
