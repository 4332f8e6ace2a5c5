#!/usr/bin/env python3
"""Time the multiclass scoring calls on device-resident data at the flagship shapes (diagnostic tool):

  c2: 10M x 512 f32 dense rows in 256 partitions: psgd_evaluate_multinomial_device at K = 3 and K = 10;
  c4: 20M rcv1-like CSR rows, 47,236 features, 94 non-zeros, f32 values, 256 partitions: K = 3;
  psgd_confusion_device on 10M (prediction, label) pairs at K = 10.

Each multinomial pass is timed in turn with the binary pass over the same registered rows
(psgd_evaluate_device, Logistic: score_dense / score_csr) -- one call of each, alternating, in one
session -- so that the two are compared under the same clocks and neighbours. HIP events around each
call after a warm-up; one JSON line per workload: median and min milliseconds of both, their ratio,
the bytes of the rows over the time, and for the dense shapes the f64 fma count (K - 1) n d over the
time beside the vector f64 ceiling. That ceiling: 256 CUs x 4 SIMDs, a wave64 f64 fma issuing in 4
cycles (16 lanes a clock a SIMD, half the f32 vector rate of 157.3 TFLOP/s), at 2.4 GHz = 39.3 T
fma/s (78.6 TFLOP/s).

usage: python tools/multiclass_bench.py [--what c2|c4|confusion|all] [--rows N] [--partitions P] [--reps K]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_FMA_PER_S = 256 * 4 * 16 * 2.4e9   # vector f64 fma a second at the 2.4 GHz peak clock


def timed(st, torch, calls, warmup, reps):
    """calls: {name: fn}; one call of each per round, in turn. -> {name: [ms]}"""
    ms = {name: [] for name in calls}
    with torch.cuda.stream(st):
        for k in range(warmup + reps):
            for name, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                e1.synchronize()
                if k >= warmup:
                    ms[name].append(e0.elapsed_time(e1))
    return ms


def stats(ms):
    return round(statistics.median(ms), 4), round(min(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="all", choices=["c2", "c4", "confusion", "all"])
    ap.add_argument("--rows", type=int, default=0, help="rows instead of the shape's own (smaller boxes)")
    ap.add_argument("--partitions", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")

    import torch
    import __graft_entry__ as g
    import bench as B
    pkg = g.load_package()
    dev = torch.device("cuda", 0)
    P = a.partitions

    def score(name, parts, n, d, nbytes, classes):
        engine = pkg.HipEngine(pkg.PartitionedData(parts))
        st = engine.stream
        out = torch.zeros(3 + 2 * P, dtype=torch.float64, device=dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(11)
        wb = torch.randn(d, dtype=torch.float64, device=dev, generator=gen) / d ** 0.5
        calls = {"binary": lambda: engine.ctx.evaluate_device(0, wb.data_ptr(), out.data_ptr(), out.data_ptr() + 24,
                                                              st.cuda_stream)}
        ws = {}
        for K in classes:
            ws[K] = torch.randn((K - 1) * d, dtype=torch.float64, device=dev, generator=gen) / d ** 0.5
            calls[f"K={K}"] = (lambda K=K: engine.ctx.evaluate_multinomial_device(
                K, ws[K].data_ptr(), out.data_ptr(), out.data_ptr() + 24, st.cuda_stream))
        torch.cuda.synchronize()
        ms = timed(st, torch, calls, a.warmup, a.reps)
        bmed, bmin = stats(ms["binary"])
        for K in classes:
            med, lo = stats(ms[f"K={K}"])
            rec = {"workload": f"{name} evaluate_multinomial K={K}", "rows": n, "features": d, "partitions": P,
                   "reps": a.reps, "ms_median": med, "ms_min": lo, "binary_ms_median": bmed, "binary_ms_min": bmin,
                   "ratio_median": round(med / bmed, 3), "bytes": nbytes, "GBps_median": round(nbytes / med / 1e6, 1),
                   "binary_GBps_median": round(nbytes / bmed / 1e6, 1)}
            if name == "c2":
                fma = (K - 1) * n * d
                rec["f64_fma"] = fma
                rec["Tfma_per_s_median"] = round(fma / med / 1e9, 2)
                rec["f64_ceiling_ms"] = round(fma / F64_FMA_PER_S * 1e3, 3)
            print(json.dumps(rec), flush=True)
        del engine

    if a.what in ("c2", "all"):
        n, d = a.rows or 10_000_000, 512
        X, _, offs = B.make_shard(torch, dev, n, d, P, "logistic", "f32", 7)
        y = torch.randint(0, 3, (n,), device=dev).to(torch.float64)   # classes of K = 3: valid labels for K = 10 too
        parts = [pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])]
        score("c2", parts, n, d, n * d * 4 + n * 8, (3, 10))
        del parts, X, y
        torch.cuda.empty_cache()
    if a.what in ("c4", "all"):
        n, d, nnz = a.rows or 20_000_000, 47_236, 94
        row_ptr, col, val, _, offs = B.make_csr_shard(torch, dev, n, d, P, "logistic", "f32", 7, nnz)
        y = torch.randint(0, 3, (n,), device=dev).to(torch.float64)
        parts = [pkg.DeviceCsrPartition(y[s:e], row_ptr[s:e + 1], col, val, d) for s, e in zip(offs[:-1], offs[1:])]
        score("c4", parts, n, d, n * nnz * 8 + (n + P) * 8 + n * 8, (3,))
        del parts, row_ptr, col, val, y
        torch.cuda.empty_cache()
    if a.what in ("confusion", "all"):
        from spark_parallelized_sgd_amd.optimization import get_context
        n, K = a.rows or 10_000_000, 10
        ctx = get_context(0)
        st = torch.cuda.Stream(device=dev)
        y = torch.randint(0, K, (n,), device=dev).to(torch.float64)
        p = torch.where(torch.rand(n, device=dev) < 0.7, y, torch.randint(0, K, (n,), device=dev).to(torch.float64))
        buf = torch.zeros(1 + K * K, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ms = timed(st, torch, {"confusion": lambda: ctx.confusion_device(
            p.data_ptr(), y.data_ptr(), n, K, buf.data_ptr() + 8, buf.data_ptr(), st.cuda_stream)}, a.warmup, a.reps)
        med, lo = stats(ms["confusion"])
        h = buf.cpu().numpy()
        print(json.dumps({"workload": f"confusion K={K}", "pairs": n, "reps": a.reps, "ms_median": med, "ms_min": lo,
                          "bytes": 16 * n, "GBps_median": round(16 * n / med / 1e6, 1), "n_bad": int(h[0]),
                          "counted": int(h[1:].sum())}), flush=True)


if __name__ == "__main__":
    main()
