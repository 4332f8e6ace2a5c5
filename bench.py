"""Benchmark of the parallelized-SGD hot path on MI355X (one process per GPU).

A step = one outer iteration of ParallelizedSGD.runParallelizedSGD (ParallelizedSGD.scala:237-299)
over this GPU's partitions: the chain kernel over every partition (PSGD:243-270), the on-device
fold (PSGD:271-276), with N > 1 the RCCL all-gather of the per-GPU partials and the cross-GPU
fold, and the driver bookkeeping (loss, count, new weights) -- with tol = 0 and full batches as
the driver's pipelined loop runs it (ParallelizedSGD._run_pipelined: epochs enqueued two ahead of
their scalar reads). Inputs are synthetic and resident in HBM before the timed region. Default workload = BASELINE.json configs[1]
("Least-squares linear regression, dense 10M x 512 fp32, 256 chains on 1 MI355X"); per-GPU work
is fixed as N grows (weak scaling: every GPU runs its own 256 chains x 10M rows).

A plain run sets up, warms up, times the steps of that one workload, writes the last step's
results if --dump-outputs is given, and prints its line. --full adds, after the headline, the CPU
baselines, the secondary workloads (the other BASELINE configs, precisions and updaters), c5's
store-mode probe and the detail file.

Prints ONE JSON line (rank 0), kept under LINE_LIMIT bytes; the secondary workloads' full records
go to --detail (a JSON file), their summary onto the line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from collections import deque

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (gradient, rows per GPU, d, chains per GPU, step, storage dtype, BASELINE config)
    # c1 is the reference's own CPU-runnable case (4 chains: latency-bound on a GPU, a parity
    # config); run it with --compute f64, its precision
    "c1": ("logistic", 100_000, 100, 4, 1.0, "f64",
           "Logistic regression, synthetic dense 100k x 100 fp64, 4 partitions (Spark local[4] case)"),
    "c2": ("least_squares", 10_000_000, 512, 256, 1e-3, "f32",
           "Least-squares linear regression, dense 10M x 512 fp32, 256 chains on 1 MI355X"),
    "c3": ("logistic", 12_500_000, 1024, 256, 1.0, "f32",
           "Logistic regression, dense 100M x 1024 (per-GPU shard: 12.5M rows, 256 of 2048 chains)"),
    "c4": ("hinge", 20_000_000, 47_236, 256, 1.0, "f32",
           "Hinge-loss linear SVM, sparse CSR rcv1-like (47,236 features, 94 nnz/row = 0.2%)"),
    "c5": ("logistic", 125_000_000, 1 << 22, 1024, 0.5, "f32",
           "L2 logistic regression, sparse 2^22 features (HBM-resident weights), 1B rows over 8 GPUs: "
           "1024 of 8192 chains per GPU, lambda 1e-6"),
}
CSR_NNZ = {"c4": 94, "c5": 100}  # nonzeros per row (c4: rcv1's mean; c5: SURVEY §8d)
REG = {"c5": 1e-6}                # SquaredL2 regParam (c5); others: Simple updater
# secondary lines: rows per GPU (0 = the workload's own; c5's full 125M-row shard takes minutes)
SECONDARY_ROWS = {"c5": 20_000_000}
# secondary specs are workload[:compute[:updater[:storage]]]; c3 with f64 storage is the
# reference's own Double rows (8,200 B per sample)
# (AdaGrad / Adam on the logistic c3 shard: the reference's Adam, r^iter in fix1 (UPD.scala:262),
# turns NaN once the squared-gradient average r exceeds 1, which least squares at c2 reaches)
DEFAULT_SECONDARY = ("c3:f32,c3:f64::f64,c3:f64,c2:f64,c1:f64,c4:f32,c4:f64,c4:f64::f64,c5:f32,c5:f64,"
                     "c3:f32:adagrad,c3:f32:adam,c3:f64:adagrad,c3:f64:adam")
# N > 1 (the driver's scaling runs): BASELINE's own multi-GPU configs as secondaries, per GPU --
# configs[2] (dense logistic 100M x 1024 over 8 GPUs = c3's 12.5M-row shard per GPU, fp32 and the
# reference's f64 rows) and configs[4] (1B-row L2 logistic over 8 GPUs = c5's full 125M-row shard)
DEFAULT_SECONDARY_MULTI = "c3:f32,c3:f64::f64,c5:f32"
SECONDARY_ROWS_MULTI = {"c5": 125_000_000}
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
DEFAULT_DETAIL = os.path.join("bench_out", "bench_detail.json")   # --full's detail file
DUMP_LIMIT_BYTES = 64_000_000   # --dump-outputs writes at most this much


def pmc_traffic(workload, grad, variant, storage, rows, compute="f32", updater="simple"):
    """HBM bytes per chain-kernel launch from the newest committed rocprofv3 PMC summary of the
    same workload and kernel instance (profiles/r*_<workload>[_<tag>]_pmc.json,
    tools/profile_round.sh + tools/pmc_summary.py; FETCH_SIZE doubled per MI355X_MICROARCH.md
    §HBM), or None. `compute` is part of the kernel instance only through `variant`."""
    import glob
    files = glob.glob(os.path.join(ROOT, "profiles", f"r*_{workload}_pmc.json")) + \
        glob.glob(os.path.join(ROOT, "profiles", f"r*_{workload}_*_pmc.json"))
    if not files or not (100 <= variant < 200 or 300 <= variant < 900):
        return None, None
    g = {"logistic": 0, "least_squares": 1, "hinge": 2}[grad]
    u = {"simple": 0, "squared_l2": 1, "l1": 2, "adagrad": 3, "adam": 4}.get(updater)
    if u is None:
        return None, None
    sname = "float" if storage == "f32" else "double"
    cname = "float" if compute == "f32" else "double"
    nv = variant % 10
    # the launched instance's template arguments (psgd_*.hip); a trailing CONV argument (the
    # per-sample break, round 4) is absent from older summaries and means false there
    if variant >= 800:     # chain_split<S, T, GRAD, UPD, CONV, NV, FULL, H>
        kern, want = "chain_split", {0: sname, 1: cname, 2: g, 3: u, 4: "false", 5: nv}
    elif variant >= 700:   # chain_block64<S, GRAD, UPD, NV, FULL, H[, CONV]>
        kern = "chain_block64"
        want = {0: sname, 1: g, 2: u, 3: nv, 5: 1 + (variant - 700) % 40 // 10,
                6: "true" if variant >= 740 else "false"}
    elif variant >= 600:   # chain_sparse_lds<S, T, GRAD, UPD, SK, TAIL[, CONV]>
        kern = "chain_sparse_lds"
        want = {0: sname, 1: "double" if (variant - 600) % 40 >= 20 else "float", 2: g, 3: u,
                6: "true" if variant >= 640 else "false"}
    elif variant >= 500:
        return None, None
    elif 420 <= variant < 430 or 460 <= variant < 470:   # chain_sparse64<S, GRAD, UPD[, CONV]>
        kern, want = "chain_sparse64", {0: sname, 1: g, 2: u, 3: "true" if variant >= 460 else "false"}
    elif 410 <= variant < 420:   # chain_sparse_spec<S, GRAD, UPD, SK, SR>
        kern, want = "chain_sparse_spec", {0: sname, 1: g, 2: u}
    elif variant >= 400:   # chain_sparse<S, GRAD, UPD[, CONV]>
        kern, want = "chain_sparse", {0: sname, 1: g, 2: u, 3: "true" if variant >= 440 else "false"}
    elif variant >= 300:   # chain_block<S, GRAD, UPD, NV, FULL[, CONV]>
        kern, want = "chain_block", {0: sname, 1: g, 2: u, 3: nv, 5: "true" if variant >= 340 else "false"}
    else:                  # chain_dense<S, T, GRAD, UPD, CONV = false, NV, FULL>
        kern, want = "chain_dense", {0: sname, 1: cname, 2: g, 3: u, 4: "false", 5: variant - 100}
    defaults = {"chain_block64": 7, "chain_sparse_lds": 7, "chain_sparse64": 4, "chain_sparse": 4,
                "chain_block": 6}

    def matches(name):
        if not name.startswith(f"psgd::{kern}<") or not name.endswith(">"):
            return False
        args = name[len(f"psgd::{kern}<"):-1].split(", ")
        full = defaults.get(kern)
        if full and len(args) == full - 1:
            args.append("false")   # the CONV argument of summaries older than it
        return all(i < len(args) and args[i] == str(v) for i, v in want.items())
    # newest round first (r04b before r04 before r03), then the file name
    for path in sorted(files, key=lambda f: os.path.basename(f), reverse=True):
        with open(path) as f:
            summ = json.load(f)
        for name, e in summ.get("kernels", {}).items():
            if matches(name) and "hbm_bytes" in e:
                # the summary's launch may have processed a different row count (--rows): per row
                per_row = e["hbm_bytes"] / max(summ.get("rows_per_launch") or rows, 1)
                return per_row * rows, os.path.relpath(path, ROOT)
    return None, None


def kernel_name(variant):
    if 800 <= variant < 900:
        h = (variant - 800) // 10
        return (f"chain_split (NV={variant % 10}: per-sample chain, features split over {h} compute waves, "
                f"partial dots exchanged through LDS)")
    if 700 <= variant < 800:
        waves = 1 + (variant - 700) % 40 // 10
        brk = ", per-sample isConverged break" if variant >= 740 else ""
        return (f"chain_block64 (NV={variant % 10}: blocked fp64 chain, 8-row Gram blocks, "
                f"{waves} chain wave{'s' if waves > 1 else ''}{brk})")
    if 300 <= variant < 400:
        brk = ", per-sample isConverged break" if variant >= 340 else ""
        return f"chain_block (NV={variant % 10}: blocked fp32 chain, 8-row Gram blocks{brk})"
    if 600 <= variant < 700:
        prec = "fp64" if (variant - 600) % 40 >= 20 else "fp32"
        brk = ", per-sample isConverged break" if variant >= 640 else ""
        return (f"chain_sparse_lds ({prec} CSR chain, weights LDS-resident [tail past ~160 KiB: L2-resident, "
                f"gathered {8 if (variant % 20) >= 10 else 4} samples ahead with an LDS feature-tag correction]{brk})")
    if 420 <= variant < 430 or 460 <= variant < 470:
        brk = ", per-sample isConverged break" if variant >= 460 else ""
        return ("chain_sparse64 (fp64 CSR chain, weights as double vectors in HBM, alpha-scaled SquaredL2, "
                f"one gather round trip per sample{brk})")
    if 410 <= variant < 420:
        return ("chain_sparse_spec (fp32 CSR chain, weights L2/MALL-resident, gathers 8 samples "
                "ahead with an LDS feature-tag correction)")
    if 400 <= variant < 410 or 440 <= variant < 450:
        brk = ", per-sample isConverged break" if variant >= 440 else ""
        return f"chain_sparse (fp32 CSR chain, weights L2/MALL-resident, one gather round trip per sample{brk})"
    if 100 <= variant < 200:
        return f"chain_dense (NV={variant - 100}: per-sample chain)"
    return f"chain_general (variant {variant})"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="c2", choices=sorted(WORKLOADS))
    ap.add_argument("--compute", default="f32", choices=["f32", "f64"])
    ap.add_argument("--rows", type=int, default=0, help="override rows per GPU (testing)")
    ap.add_argument("--features", type=int, default=0, help="override d (experiments; not a BASELINE config)")
    ap.add_argument("--chains", type=int, default=0, help="override chains per GPU (experiments; not a BASELINE config)")
    ap.add_argument("--fraction", type=float, default=1.0,
                    help="miniBatchFraction: batch i = RDD.sample(false, f, 42 + i) per partition")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="CPU baseline budget")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--secondary", default=None,
                    help="comma list of workload[:compute[:updater[:storage]]] measured after the headline "
                         "(default: DEFAULT_SECONDARY on 1 GPU, DEFAULT_SECONDARY_MULTI on N > 1; '' = none)")
    ap.add_argument("--secondary-rows", type=int, default=0,
                    help="rows per GPU of every secondary workload (testing; 0 = each workload's default)")
    ap.add_argument("--updater", default="", help="another SGDUpdater for the headline workload (experiments)")
    ap.add_argument("--storage", default="", choices=["", "f32", "f64"],
                    help="row storage dtype of the headline workload (default: the workload's own)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="process-group backend for --gpus > 1: nccl (RCCL over xGMI, one GPU per rank) or "
                         "gloo (a CPU rehearsal of the multi-rank path; ranks may share one GPU)")
    ap.add_argument("--skew-rows", type=int, default=0,
                    help="dense shards: start partition p's rows p * K rows later in HBM (layout experiments)")
    ap.add_argument("--tol", type=float, default=0.0,
                    help="convergenceTol of the headline workload (PSGD.scala:262 per-sample break; the "
                         "reference's default is 0.001; BASELINE's configs run 0)")
    ap.add_argument("--no-arena", action="store_true",
                    help="allocate each workload's rows separately (A/B of the one-allocation arena)")
    ap.add_argument("--detail", default=None,
                    help="file for the full headline and secondary records ('' = none; default: none in a "
                         f"plain run, {DEFAULT_DETAIL} with --full); stdout carries a summary")
    ap.add_argument("--prewarm-s", type=float, default=1.0,
                    help="untimed epochs for this long before the warmup steps (GPU clock ramp)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline also measure what a plain run leaves out: the CPU baselines, the "
                         "secondary workloads (--secondary), c5's store-mode probe, and the detail file")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step of the headline workload returned to its caller "
                         "(the folded weights, the loss sum and the sample count) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.secondary and not args.full:
        ap.error("--secondary workloads are measured only with --full")
    return args


class Arena:
    """One device allocation, made at the start of the process, that every workload's synthetic
    rows are carved from (the partitions of a persisted RDD are registered once and stay resident;
    the bench does not allocate and free 20-100 GB per workload). Measured round 5: a dense
    workload whose rows were allocated after another workload's 51-102 GB had been freed streamed
    5-7 % slower (profiles/r05_c3_stream_ceiling.log item 4); carved from one arena every workload
    runs on the process's first allocation."""

    def __init__(self, torch, dev, nbytes):
        self.buf = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
        self.off = 0

    def take(self, shape, dtype):
        import math
        n = math.prod(shape) * dtype.itemsize
        if self.off + n > self.buf.numel():
            raise MemoryError(f"arena: {n} bytes past its {self.buf.numel()}")
        t = self.buf[self.off:self.off + n].view(dtype).view(shape)
        self.off += (n + 4095) // 4096 * 4096
        return t

    def reset(self):
        self.off = 0


def shard_bytes(workload, storage="", rows=0, features=0, skew=0, chains=0):
    """Bytes of a workload's synthetic rows and labels in the arena (4 KiB rounding per tensor)."""
    grad, n, d, P, step, sdt = WORKLOADS[workload][:6]
    sdt = storage or sdt
    n = rows or n
    d = features or d
    P = chains or P
    es = 4 if sdt == "f32" else 8
    pad = 3 * 4096
    if workload in CSR_NNZ:
        nnz = CSR_NNZ[workload]
        return n * nnz * (4 + es) + n * 8 + pad
    return (n + P * skew) * d * es + n * 8 + pad


def make_shard(torch, dev, n, d, P, grad, dtype, seed, skew=0, arena=None):
    """Synthetic rows in HBM: X ~ N(0,1); w* ~ N(0, 1/d); LeastSquares y = w*.x + N(0, 0.01);
    Logistic y = 1{w*.x + Logistic(0,1) > 0}. skew > 0: partition p's rows start
    p * skew rows later in the allocation (unused rows in between). X and y from `arena` if given."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    tdt = torch.float32 if dtype == "f32" else torch.float64
    X = arena.take((n + P * skew, d), tdt) if arena else torch.empty((n + P * skew, d), dtype=tdt, device=dev)
    chunk = 1 << 20
    w_star = torch.randn(d, generator=g, device=dev, dtype=torch.float64) / d ** 0.5
    y = arena.take((n,), torch.float64) if arena else torch.empty(n, dtype=torch.float64, device=dev)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        X[a:b].normal_(generator=g)
        z = X[a:b].to(torch.float64) @ w_star
        if grad == "least_squares":
            y[a:b] = z + 0.1 * torch.randn(b - a, generator=g, device=dev, dtype=torch.float64)
        else:
            u = torch.rand(b - a, generator=g, device=dev, dtype=torch.float64).clamp_(1e-12, 1 - 1e-12)
            y[a:b] = ((z + torch.log(u) - torch.log1p(-u)) > 0).to(torch.float64)
    offs = [i * n // P for i in range(P)] + [n]
    if skew:
        # move each partition's rows to its skewed place, last partition first
        for p in range(P - 1, 0, -1):
            a, b = offs[p], offs[p + 1]
            X[a + p * skew:b + p * skew] = X[a:b].clone()
    return X, y, offs


def make_csr_shard(torch, dev, n, d, P, grad, dtype, seed, nnz, arena=None):
    """Synthetic rcv1-like CSR rows in HBM: nnz distinct sorted indices per
    row (one uniform draw in each of nnz equal column buckets), values U(0,1) L2-normalised per
    row, labels y = 1{w*.x + Logistic(0,1) > 0} from a planted w* ~ N(0,1)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    tdt = torch.float32 if dtype == "f32" else torch.float64
    width = d // nnz
    if arena:
        col, val, y = arena.take((n, nnz), torch.int32), arena.take((n, nnz), tdt), arena.take((n,), torch.float64)
    else:
        col = torch.empty((n, nnz), dtype=torch.int32, device=dev)
        val = torch.empty((n, nnz), dtype=tdt, device=dev)
        y = torch.empty(n, dtype=torch.float64, device=dev)
    w_star = torch.randn(d, generator=g, device=dev, dtype=torch.float64)
    base = (torch.arange(nnz, device=dev, dtype=torch.int64) * width)[None, :]
    chunk = 1 << 18
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        c = base + torch.randint(0, width, (b - a, nnz), generator=g, device=dev)
        v = torch.rand((b - a, nnz), generator=g, device=dev, dtype=torch.float64)
        v = v / v.norm(dim=1, keepdim=True)
        col[a:b] = c.to(torch.int32)
        val[a:b] = v.to(tdt)
        z = (val[a:b].to(torch.float64) * w_star[c]).sum(1)
        u = torch.rand(b - a, generator=g, device=dev, dtype=torch.float64).clamp_(1e-12, 1 - 1e-12)
        y[a:b] = ((z + torch.log(u) - torch.log1p(-u)) > 0).to(torch.float64)
    row_ptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * nnz
    offs = [i * n // P for i in range(P)] + [n]
    return row_ptr, col.reshape(-1), val.reshape(-1), y, offs


def host_cpus():
    """CPUs this process may run on: its affinity set, capped by a cgroup-v2 CPU quota when one
    is set (a container's share of the host), so the baseline's threads all run at once."""
    n = len(os.sched_getaffinity(0))
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(grad, d, P, step, budget_s, seed=7, csr_nnz=0, updater="simple", reg=0.0):
    """Time the CPU restatement of the reference (oracle/, one thread per partition, all host
    cores) on a bounded sample of the same workload -- its gradient and SGDUpdater -- the first m
    rows of every partition."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    cores = min(host_cpus(), P)
    rng = np.random.default_rng(seed)

    def sample(m):
        X = rng.standard_normal((P * m, d)).astype(np.float32).astype(np.float64)
        w = rng.standard_normal(d) / np.sqrt(d)
        z = X @ w
        y = z + 0.1 * rng.standard_normal(P * m) if grad == "least_squares" else \
            ((z + rng.logistic(size=P * m)) > 0).astype(float)
        return O.Matrix(y, X)

    def sample_csr(m):
        width = d // csr_nnz
        col = (np.arange(csr_nnz) * width)[None, :] + rng.integers(0, width, (P * m, csr_nnz))
        val = rng.uniform(size=(P * m, csr_nnz))
        val = (val / np.linalg.norm(val, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
        y = (rng.uniform(size=P * m) > 0.5).astype(float)
        rp = np.arange(P * m + 1, dtype=np.int64) * csr_nnz
        return O.Matrix(y, row_ptr=rp, col=col.reshape(-1).astype(np.int32), val=val.reshape(-1), d=d)

    # A sample of m rows per partition (host memory bounded), re-run as successive epochs until
    # the time budget is spent: per-epoch CPU cost does not depend on which rows are used.
    m = 1024 if (csr_nnz or d <= 1024) else 256
    mat = sample_csr(m) if csr_nnz else sample(m)
    offs = [p * m for p in range(P + 1)]
    w = np.zeros(d)
    total, epochs = 0, 0
    t0 = time.perf_counter()
    while True:
        w_out, _, _, cnt = O.run_chains(mat, offs, grad, updater, step, reg, w, tol=0.0,
                                        n_threads=cores)
        total += int(cnt.sum())
        epochs += 1
        w = w_out.mean(axis=0)
        dt = time.perf_counter() - t0
        if dt >= budget_s:
            break
    return {"value": total / dt, "unit": "samples/s", "cores": cores, "kind": "port",
            "host_cpus": host_cpus(), "nproc": os.cpu_count(),
            "sample": f"oracle/psgd_oracle.c (fp64 CPU restatement of ParallelizedSGD.scala:243-270 "
                      f"incl. per-sample isConverged; {grad}, {updater}), {P} partitions x {m} "
                      f"{'CSR (%d nnz) ' % csr_nnz if csr_nnz else ''}rows, d={d}, "
                      f"{epochs} epochs, {cores} threads, {dt:.1f} s"}


def cpu_baseline_c1(budget_s, seed=42):
    """BASELINE configs[0] on the CPU: logistic, dense 100k x 100 fp64, 4 partitions, one thread
    per partition (Spark local[4]); the CPU restatement's whole epochs, repeated for budget_s."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    grad, n, d, P, step = WORKLOADS["c1"][:5]
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    w_star = rng.standard_normal(d) / np.sqrt(d)
    y = ((X @ w_star + rng.logistic(size=n)) > 0).astype(float)
    mat = O.Matrix(y, X)
    offs = [p * n // P for p in range(P + 1)]
    w = np.zeros(d)
    total, epochs = 0, 0
    t0 = time.perf_counter()
    while True:
        w_out, _, _, cnt = O.run_chains(mat, offs, grad, "simple", step, 0.0, w, tol=0.0, n_threads=P)
        total += int(cnt.sum())
        epochs += 1
        w = w_out.mean(axis=0)
        dt = time.perf_counter() - t0
        if dt >= budget_s:
            break
    return {"value": total / dt, "unit": "samples/s", "cores": P, "kind": "port",
            "sample": f"oracle/psgd_oracle.c, the whole c1 epoch ({n} x {d} fp64, {P} partitions, "
                      f"{P} threads = local[{P}]), {epochs} epochs, {dt:.1f} s"}


def run_workload(torch, dist, pkg, dev, rank, world, local, workload, compute, rows, fraction,
                 steps, warmup, prewarm_s, features=0, chains=0, updater="", storage="", backend="nccl",
                 skew=0, tol=0.0, arena=None, store_probe=False, keep_outputs=False):
    """One workload: synthetic shard in HBM, prewarm, W warmup steps, K timed steps (barrier +
    synchronize on both sides, max over ranks). Returns the measurement as a dict. store_probe:
    c5's store-mode probe (launches of its own) after the timed steps; keep_outputs: the last
    timed step's results, copied to the host after the timed region, under "_outputs"."""
    import numpy as np
    # the ranks' scalar agreements (prewarm epoch count, elapsed time): device tensors over RCCL,
    # host tensors over gloo
    red_dev = dev if backend == "nccl" else torch.device("cpu")
    grad, n, d, P, step, sdt, cfg_name = WORKLOADS[workload]
    if storage and storage != sdt:
        sdt = storage
        cfg_name += f" [{sdt} storage" + (": the reference's Double rows]" if sdt == "f64" else "]")
    if rows and rows != n:
        cfg_name += f" [this run: {rows:,} rows per GPU of the {n:,}-row shard]"
    if rows:
        n = rows
    if features:
        d = features
        cfg_name += f" [d overridden: {d}]"
    if chains:
        P = chains
        cfg_name += f" [chains overridden: {P}]"
    csr = workload in CSR_NNZ
    if csr:
        rp, col, val, y, offs = make_csr_shard(torch, dev, n, d, P, grad, sdt, 1000 + rank,
                                               CSR_NNZ[workload], arena)
        torch.cuda.synchronize()
        parts = [pkg.DeviceCsrPartition(y[a:b], rp[a:b + 1], col, val, d) for a, b in zip(offs[:-1], offs[1:])]
        empty = lambda: pkg.DeviceCsrPartition(y[:0], rp[:1], col, val, d)
    else:
        X, y, offs = make_shard(torch, dev, n, d, P, grad, sdt, 1000 + rank, skew, arena)
        torch.cuda.synchronize()
        parts = [pkg.DevicePartition(y[a:b], X[a + p * skew:b + p * skew], d)
                 for p, (a, b) in enumerate(zip(offs[:-1], offs[1:]))]
        empty = lambda: pkg.DevicePartition(y[:0], X[:0], d)
    # global partition list: this rank's block is [rank*P, (rank+1)*P)
    all_parts = [None] * (P * world)
    all_parts[rank * P:(rank + 1) * P] = parts
    for i in range(len(all_parts)):
        if all_parts[i] is None:
            all_parts[i] = empty()  # placeholders for other ranks
    data = pkg.PartitionedData(all_parts)
    engine = pkg.HipEngine(data, rank, world, device=local)
    gcls = {"least_squares": pkg.LeastSquaresGradient, "logistic": pkg.LogisticGradient,
            "hinge": pkg.HingeGradient}[grad]()
    reg = REG.get(workload, 0.0)
    ucls = pkg.SquaredL2SGDUpdater() if reg > 0 else pkg.SimpleSGDUpdater()
    if updater:   # the workload with another SGDUpdater plugin (UPD.scala:120-286)
        ucls = {"l1": pkg.L1SGDUpdater, "adagrad": pkg.AdaGradSGDUpdater, "adam": pkg.AdamSGDUpdater,
                "simple": pkg.SimpleSGDUpdater, "squared_l2": pkg.SquaredL2SGDUpdater}[updater]()
    params = pkg.make_params(gcls, ucls, step, reg, fraction, tol, compute)
    w = engine.weights(np.zeros(d))
    stream = engine.stream  # the engine's kernels and copies all run on this stream

    # tol == 0 with full batches: the driver's pipelined loop (ParallelizedSGD._run_pipelined --
    # every epoch enqueued with the previous epoch's folded weights, its three scalars read back
    # PIPELINE_LAG epochs later); otherwise the loop's synchronous form (scalars after each epoch)
    pipelined = fraction >= 1.0 and tol == 0.0
    lag = pkg.ParallelizedSGD.PIPELINE_LAG if pipelined else 0

    def run_epochs(w, it0, k, events=None):
        """k epochs from iteration it0; events: k + 1 HIP events, one recorded on the engine
        stream before each epoch and one after the last. Returns (w, last count, last loss,
        total count)."""
        pending = deque()
        last = [0, 0.0, 0]

        def settle(scalars):
            _, loss, cnt = scalars   # the 3 driver scalars (PSGD:278-287)
            last[0], last[1] = cnt, loss
            last[2] += cnt
            return cnt

        for j in range(k):
            params.iteration = it0 + j
            if events is not None:
                events[j].record(stream)
            if pipelined:
                folded, token = engine.epoch_async(params, w)
            else:
                folded, _ = engine.epoch(params, w)
            if pipelined:
                pending.append(token)
                w = engine.adopt_view(folded)
                if len(pending) > lag:
                    settle(engine.scalars_wait(pending.popleft()))
            elif settle(engine.scalars(folded)) > 0:
                w = engine.adopt(folded)
        if events is not None:
            events[k].record(stream)
        while pending:
            settle(engine.scalars_wait(pending.popleft()))
        return w, last[0], last[1], last[2]

    def chain_ms_since(first):
        """Device ms of the chain launches from launch `first` on (HIP events around each chain
        launch on the engine stream; the context keeps the last 64)."""
        end = engine.ctx.chain_launches()
        return [engine.ctx.chain_ms(k) for k in range(max(first, end - 64), end)]

    # Device prewarm (part of setup, like data generation): the chain kernel's first launches run
    # below steady-state clocks (rocprof trace: 3.5-3.8 ms for the first c2 epochs, 3.1 ms from
    # the sixth on), so untimed epochs run for --prewarm-s seconds before the W warmup steps.
    # The model they produce is discarded: the warmup and timed steps start from w = 0.
    # Every epoch holds a collective when N > 1, so all ranks run the same count: two epochs
    # time one, and the count for --prewarm-s is the max over ranks.
    w0 = w
    prewarm_epochs = 0
    if prewarm_s > 0:
        wp = w0
        torch.cuda.synchronize()
        t_pw = time.perf_counter()
        wp, _, _, _ = run_epochs(wp, 1, 2)
        prewarm_epochs = 2
        torch.cuda.synchronize()
        per_epoch = (time.perf_counter() - t_pw) / 2
        want = max(2, min(5000, int(prewarm_s / max(per_epoch, 1e-6))))
        if world > 1:
            t = torch.tensor([want], dtype=torch.int64, device=red_dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            want = int(t.item())
        if want > prewarm_epochs:
            wp, _, _, _ = run_epochs(wp, prewarm_epochs + 1, want - prewarm_epochs)
            prewarm_epochs = want
        torch.cuda.synchronize()
    w = w0
    if warmup:
        w, cnt, loss, _ = run_epochs(w, 1, warmup)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    # one HIP event at each step's start and one after the last: each step's device time is the
    # interval to the next start (an event pair per step cost the device ~5 us more per step)
    events = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    if world > 1:
        engine.exchange_events = []   # HIP events around each timed step's all-gather + fold
    first_launch = engine.ctx.chain_launches()
    t0 = time.perf_counter()
    w, cnt, loss, total = run_epochs(w, warmup + 1, steps, events)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # `cnt` is the whole job's sample count of the step (the fold sums counts over all ranks)
    samples_per_step = cnt
    if fraction >= 1.0 and tol == 0.0:
        assert samples_per_step == n * world, (samples_per_step, n * world)
    else:  # sampled batches, or chains that break early (tol > 0): the timed steps' samples
        samples_per_step = total / steps
    value = samples_per_step * steps / elapsed
    assert np.isfinite(loss), loss
    kernel_ms = chain_ms_since(first_launch)
    epoch_ms = [a.elapsed_time(b) for a, b in zip(events[:-1], events[1:])]
    avg_epoch_s = sum(epoch_ms) / len(epoch_ms) / 1e3
    avg_kernel_s = sum(kernel_ms) / len(kernel_ms) / 1e3
    ranks = None
    if world > 1:
        # every rank's chain-kernel ms and all-gather + fold ms (its HIP events), gathered to all
        xchg = [a.elapsed_time(b) for a, b in engine.exchange_events]
        engine.exchange_events = None
        mine = torch.tensor([avg_kernel_s * 1e3, sum(xchg) / max(len(xchg), 1)], dtype=torch.float64,
                            device=red_dev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        ranks = {"kernel_ms": [round(float(t[0]), 3) for t in allr],
                 "xchg_ms": [round(float(t[1]), 4) for t in allr]}
    es = 4 if sdt == "f32" else 8
    variant = engine.ctx.last_kernel()
    offchip = None
    if csr:
        # the row stream -- values + int32 columns + int64 row pointer + f64 label --
        # plus, when the chain's weights are not on chip, their gather and scatter (2 nnz
        # sizeof(T)). chain_sparse_lds keeps them in LDS (its tail in L2): the row stream is its
        # figure; chain_sparse / chain_sparse64 / chain_general keep them in HBM: the sum is theirs.
        # The line carries both.
        rowstream = CSR_NNZ[workload] * (es + 4) + 8 + 8
        offchip = rowstream + 2 * CSR_NNZ[workload] * (4 if compute == "f32" else 8)
        weights_on_chip = 600 <= variant < 700
        bytes_per_sample = rowstream if weights_on_chip else offchip
    else:
        bytes_per_sample = (d + 1) * es  # row + label (weights are on chip)
    local_samples = n if fraction >= 1.0 and tol == 0.0 else samples_per_step / world
    # one chain-kernel launch processes every (sampled) row of this GPU's partitions
    achieved = local_samples * bytes_per_sample / avg_kernel_s / 1e9
    # the step-level figure beside the kernel's: per-GPU samples/s of the driver-timed step x B
    frac_step = value / world * bytes_per_sample / 1e9 / HBM_PEAK_GBS
    upd_name = updater or ("squared_l2" if reg > 0 else "simple")
    traffic, traffic_src = pmc_traffic(workload, grad, variant, sdt, n, compute, upd_name)
    res = {
        "value": value, "ms_per_step": elapsed / steps * 1e3, "dtype": compute, "loss": loss,
        "config": {"workload": f"{workload}: {cfg_name}", "rows_per_gpu": n, "d": d,
                   "chains_per_gpu": P, "storage": sdt, "gradient": grad,
                   "updater": updater or ("squared_l2" if reg > 0 else "simple"), "reg_param": reg,
                   "step_size": step, "convergence_tol": tol, "mini_batch_fraction": fraction,
                   "parallelism": f"dp{world}" + (" (chains sharded, RCCL all-gather + fold per epoch)"
                                                   if backend == "nccl" else
                                                   " (chains sharded, gloo all-gather + fold per epoch: a rehearsal)")},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS, "frac_step": frac_step, "traffic": traffic,
                     "traffic_source": traffic_src,
                     "kernel": kernel_name(variant),
                     "bytes_per_launch": local_samples * bytes_per_sample,
                     "bytes_per_sample": bytes_per_sample,
                     **({"bytes_per_sample_rowstream": rowstream,
                         "frac_rowstream": local_samples * rowstream / avg_kernel_s / 1e9 / HBM_PEAK_GBS,
                         "bytes_per_sample_weights_offchip": offchip,
                         "frac_weights_offchip": local_samples * offchip / avg_kernel_s / 1e9 / HBM_PEAK_GBS}
                        if csr else {}),
                     "avg_kernel_ms": avg_kernel_s * 1e3,
                     "avg_epoch_ms": avg_epoch_s * 1e3,
                     "variant": variant,
                     "timing": "HIP events recorded around each chain-kernel launch on its stream"},
        "prewarm": {"seconds": prewarm_s, "epochs": prewarm_epochs},   # untimed, model discarded
        **({"ranks": ranks} if ranks else {}),
        "_meta": (grad, d, P, step, csr, upd_name, reg),
        # per timed step, the chain kernel's ms (the detail file only; the stdout line drops it)
        "kernel_ms_series": [round(x, 4) for x in kernel_ms],
    }
    if keep_outputs:
        # what the loop's caller holds after the last timed step: the folded weights and the
        # step's loss sum and sample count (the three driver scalars' last two)
        res["_outputs"] = {"weights": engine.to_host(w), "loss_sum": np.array([loss], np.float64),
                           "count": np.array([cnt], np.float64)}
    if store_probe and workload == "c5" and csr:
        res["c5_store_probe"] = c5_store_probe(torch, pkg, engine, params, w0, parts, all_parts, empty,
                                               rank, P, avg_kernel_s * 1e3)
    del engine, data, parts, all_parts
    return res


# c5's kernel time follows the write rate of its scattered stores over the chains' weight vectors,
# which takes one of two levels decided by the physical placement the vectors' allocation received
# (profiles/r05_c5_placement.log). The probe times the same kernel over the first C5_PROBE_ROWS
# rows of every chain, on the same (reused) vector allocation; the per-row rate past the probe,
# (full - probe) / (rows - probe rows), leaves out the epoch's fixed start (the first touch of the
# chains' vectors) and is compared with the gap between the two levels to name the
# mode the run landed in, so box-to-box c5 numbers can be read against it.
C5_PROBE_ROWS = 2000
C5_FAST_NS = {"f32": 4.4, "f64": 4.8}   # marginal ns per row at or below: the fast store mode


def c5_store_probe(torch, pkg, engine, params, w, parts, all_parts, empty, rank, P, full_ms):
    probe = [None] * len(all_parts)
    for p, part in enumerate(parts):
        m = min(C5_PROBE_ROWS, part.n_rows)
        probe[rank * P + p] = pkg.DeviceCsrPartition(part.labels[:m], part.row_ptr[:m + 1], part.col,
                                                     part.val, part.d)
    for i in range(len(probe)):
        if probe[i] is None:
            probe[i] = empty()
    eng = pkg.HipEngine(pkg.PartitionedData(probe), engine.rank, engine.world, device=engine.device)
    ms = []
    for _ in range(3):   # the chains only (no collective): this rank's placement
        with torch.cuda.stream(eng.stream):
            eng.local_partial(params, w, False)
        ms.append(eng.ctx.last_chain_ms())
    prow = sum(min(C5_PROBE_ROWS, part.n_rows) for part in parts)
    rows = sum(part.n_rows for part in parts)
    best = min(ms[1:])
    marginal = (full_ms - best) * 1e6 / max(rows - prow, 1)
    comp = "f32" if params.compute_dtype == pkg._native.F32 else "f64"
    del eng
    return {"rows_per_chain": C5_PROBE_ROWS, "probe_ms": round(best, 4),
            "marginal_ns_per_row": round(marginal, 3),
            "mode": "fast" if marginal <= C5_FAST_NS[comp] else "slow"}


def dump_outputs(path, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: each array as path/<name>.npy in float64, `limit` bytes in all. An array
    past its equal share of the limit is written as a fixed sample: its elements at sorted
    indices drawn without replacement by a generator seeded with the array's length."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    share = (limit // max(len(arrays), 1) - 256) // 8   # (256: room for the .npy header)
    for name, a in arrays.items():
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        if a.size > share:
            a = a[np.sort(np.random.default_rng(a.size).choice(a.size, size=share, replace=False))]
        np.save(os.path.join(path, name + ".npy"), a)


def main():
    args = parse()
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']} "
                 "(the launcher and the flag disagree)")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: start the N ranks as children (torchrun's
        # launcher; it picks the rendezvous port itself on 127.0.0.1) and exit with their
        # status. Under a profiler its preloaded library has already initialised the GPU in
        # this process: launching from here would be a launcher hop under the profiler, so
        # profile one rank instead.
        if "rocprof" in os.environ.get("LD_PRELOAD", "") or any(k.startswith("ROCPROF") for k in os.environ):
            sys.exit("bench.py: --gpus > 1 under rocprofv3 is refused; profile a single rank (--gpus 1)")
        import subprocess
        cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1",
               f"--nproc-per-node={args.gpus}", os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.run(cmd).returncode)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as ge
    pkg = ge.load_package()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.backend == "gloo":
        # a rehearsal of the multi-rank path on fewer GPUs than ranks (ranks share devices)
        local = local % max(torch.cuda.device_count(), 1)
    if world > 1:
        torch.cuda.set_device(local)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    # a plain run measures the headline workload alone; --full adds the secondaries, the CPU
    # baselines, c5's store probe and the detail file
    spec_list = "" if not args.full else args.secondary if args.secondary is not None else \
        (DEFAULT_SECONDARY if world == 1 else DEFAULT_SECONDARY_MULTI)
    secondary = [s for s in spec_list.split(",") if s]
    detail = args.detail if args.detail is not None else (DEFAULT_DETAIL if args.full else "")
    sec_rows = SECONDARY_ROWS if world == 1 else SECONDARY_ROWS_MULTI

    def rows_of(wl):
        return args.secondary_rows or sec_rows.get(wl, 0)
    arena = None
    if not args.no_arena:
        need = shard_bytes(args.workload, args.storage, args.rows, args.features, args.skew_rows, args.chains)
        for spec in secondary:
            wl, _, _, sto = (spec.split(":") + ["", "", ""])[:4]
            need = max(need, shard_bytes(wl, sto, rows_of(wl)))
        arena = Arena(torch, dev, need)
    res = run_workload(torch, dist, pkg, dev, rank, world, local, args.workload, args.compute,
                       args.rows, args.fraction, args.steps, args.warmup, args.prewarm_s, args.features,
                       args.chains, args.updater, args.storage, args.backend, args.skew_rows, args.tol,
                       arena=arena, store_probe=args.full, keep_outputs=bool(args.dump_outputs))
    outputs = res.pop("_outputs", None)
    if outputs is not None and rank == 0:   # (the folded result is the same on every rank)
        dump_outputs(args.dump_outputs, outputs)
    grad, d, P, step, csr, upd_name, reg = res.pop("_meta")
    res.pop("loss")
    series = res.pop("kernel_ms_series")
    out = {
        "metric": "training samples/sec (whole node) + achieved HBM GB/s, logistic SGD 1/2/4/8 GPUs",
        "value": res["value"], "unit": "samples/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": res["ms_per_step"],
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": res["dtype"], "data": "synthetic (device-generated, resident in HBM)",
        "config": res["config"], "roofline": res["roofline"], "prewarm": res["prewarm"],
        **({"ranks": res["ranks"]} if "ranks" in res else {}),
        **({"c5_store_probe": res["c5_store_probe"]} if "c5_store_probe" in res else {}),
    }
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(grad, d, P, step, args.cpu_seconds,
                                           csr_nnz=CSR_NNZ[args.workload] if csr else 0,
                                           updater=upd_name, reg=reg)
        # BASELINE configs[0], the reference's own CPU case (Spark local[4]): its CPU rate in the
        # same run, beside the c1 GPU secondary line
        out["cpu_baseline_c1"] = cpu_baseline_c1(min(args.cpu_seconds, 4.0))
    # Secondary lines (one GPU only): the other BASELINE configs' per-GPU workloads under the
    # same clock, each with its own roofline (VERDICT r01 "let the driver observe" them).
    records = []
    for spec in secondary:
        wl, comp, upd, sto = (spec.split(":") + ["", "", ""])[:4]
        torch.cuda.empty_cache()
        if arena:
            arena.reset()   # the previous workload's rows are dead: the next one reuses the memory
        try:
            r = run_workload(torch, dist, pkg, dev, rank, world, local, wl, comp or "f32",
                             rows_of(wl), 1.0, args.steps, args.warmup,
                             min(args.prewarm_s, 0.5), updater=upd, storage=sto, arena=arena,
                             store_probe=True)
        except Exception as e:   # a secondary line never hides the headline
            records.append({"spec": spec, "error": f"{type(e).__name__}: {e}"})
            continue
        r.pop("_meta")
        r["spec"] = spec
        r["samples_per_s"] = r.pop("value")
        r["loss"] = float(r["loss"])
        records.append(r)
    if rank == 0:
        if records or detail:
            out["detail_file"] = write_detail(detail, dict(out, kernel_ms_series=series), records)
        print(final_line(out, records), flush=True)
    if world > 1:
        dist.destroy_process_group()


# The driver keeps only the tail of stdout (about 8 KB, stderr appended after it) and parses the
# last line: round 4's line carried 14 full secondary records (21.7 KB) and was not parsed.
LINE_LIMIT = 6000


def secondary_summary(records):
    """One compact entry per secondary workload: what the driver's line carries."""
    return [{"spec": r["spec"], "error": r["error"][:200]} if "error" in r else
            {"spec": r["spec"], "samples_per_s": round(r["samples_per_s"]),
             "frac": round(r["roofline"]["frac"], 4),
             **({"frac_step": round(r["roofline"]["frac_step"], 4)} if "frac_step" in r["roofline"] else {}),
             "kernel_ms": round(r["roofline"]["avg_kernel_ms"], 3),
             "B_per_sample": r["roofline"]["bytes_per_sample"],
             "variant": r["roofline"].get("variant"),
             **({"ranks": r["ranks"]} if "ranks" in r else {}),
             **({"c5_store_probe": r["c5_store_probe"]} if "c5_store_probe" in r else {})}
            for r in records]


def write_detail(path, out, records):
    """The full secondary records (config, roofline, prewarm of each) go to a JSON file, not to
    the stdout line. Returns the path written, or None when it could not be written."""
    if not path:
        return None
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump({"headline": out, "secondary": records}, f, indent=1)
        return os.path.relpath(os.path.abspath(path), ROOT)
    except OSError:
        return None


def final_line(out, records):
    """The ONE stdout JSON line: headline fields, roofline, cpu baselines and the compact
    secondary summary. Never longer than LINE_LIMIT bytes: if it would be, the roofline's and
    the cpu baselines' descriptive strings are dropped first, then the summary's extra fields."""
    line = {k: v for k, v in out.items() if k != "kernel_ms_series"}
    if records:
        line["secondary_summary"] = secondary_summary(records)
    s = json.dumps(line, separators=(",", ":"))
    if len(s) > LINE_LIMIT:
        for k in ("cpu_baseline", "cpu_baseline_c1"):
            if k in line:
                line[k] = {kk: v for kk, v in line[k].items() if kk != "sample"}
        line["roofline"] = {k: v for k, v in line["roofline"].items() if k not in ("kernel", "timing")}
        line["config"] = {k: v for k, v in line["config"].items() if k != "parallelism"}
        s = json.dumps(line, separators=(",", ":"))
    for keep in (("spec", "samples_per_s", "frac", "frac_step", "ranks"), ("spec", "samples_per_s", "frac")):
        if len(s) > LINE_LIMIT and records:
            line["secondary_summary"] = [{k: v for k, v in e.items() if k in keep}
                                         for e in line["secondary_summary"]]
            s = json.dumps(line, separators=(",", ":"))
    return s


if __name__ == "__main__":
    main()
