#!/usr/bin/env python3
"""Time psgd_gramian_device on device-resident data, beside its yardsticks in the same process
(diagnostic tool):

  mfma:   back-to-back v_mfma_f64_16x16x4_f64 (no memory): one workgroup (one wave a SIMD of one CU)
          and as many workgroups as CUs (each reserves 96 KiB of LDS, so a CU holds one), 1, 2, 4 and
          8 independent accumulators a wave; the loop body is MFMAs and a counter -- the issue rate
          gram_dense's share is taken of;
  c2:     10M x 512 f32 dense rows in 256 partitions;
  c3:     12.5M x 1,024 f32 dense rows in 256 partitions (skipped when HBM cannot hold it);
  d30:    10M x 30 f32 dense rows;
          each beside torch.mm(X^T, X) of a float64 copy of the same rows (the library's dgemm) and
          psgd_column_stats_device (stats_dense, the row stream);
  csr:    20M CSR rows of 32 non-zeros over 4,096 features beside psgd_gradient_sum_device (grad_csr)
          on the same rows, in atomic bytes per second (8 per add).

HIP events around each call after a warm-up; one JSON line per measurement: median and min ms.

usage: python tools/gram_bench.py [--shape mfma,c2,c3,d30,csr | all] [--rows N] [--reps K]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, st, reps, warmup, call):
    ms = []
    with torch.cuda.stream(st):
        for k in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            if k >= warmup:
                ms.append(e0.elapsed_time(e1))
    return ms


def report(shape, call, ms, extra=None):
    med, lo = statistics.median(ms), min(ms)
    line = {"shape": shape, "call": call, "reps": len(ms), "ms_median": round(med, 4), "ms_min": round(lo, 4)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of each shape's own (smaller boxes)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    shapes = ["mfma", "c2", "c3", "d30", "csr"] if a.shape == "all" else a.shape.split(",")

    import torch
    import __graft_entry__ as g
    import bench as B
    pkg = g.load_package()
    N = pkg._native
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    best = {}

    def mfma():
        L = N.lib()
        L.psgd_gram_mfma_rate.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
        L.psgd_gram_mfma_rate.restype = ctypes.c_int32
        st = torch.cuda.Stream(dev)
        out = torch.zeros(1, dtype=torch.float64, device=dev)
        iters = 20000
        for blocks in (1, cus):
            for chains in (1, 2, 4, 8):
                def call():
                    rc = L.psgd_gram_mfma_rate(blocks, chains, iters, out.data_ptr(), st.cuda_stream)
                    assert rc == 0, rc
                ms = timed(torch, st, a.reps, a.warmup, call)
                lo = min(ms)
                per_wave = iters * chains
                rate = blocks * 4 * per_wave * 1024 / (lo * 1e-3) / 1e12
                report("mfma", "v_mfma_f64_16x16x4_f64", ms,
                       {"workgroups": blocks, "accumulators": chains, "ns_per_mfma_a_simd_best": round(lo * 1e6 / per_wave, 2),
                        "Tfma_per_s_best": round(rate, 2)})
                if blocks == cus:
                    best["mfma"] = max(best.get("mfma", 0.0), rate)

    def dense(shape, n, d, P):
        try:
            # (zero-copy rows have a pitch of whole 16-byte vectors: the columns past d are never read)
            X, y, offs = B.make_shard(torch, dev, n, (d + 3) // 4 * 4, P, "least_squares", "f32", 7)
            parts = [pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])]
            engine = pkg.HipEngine(pkg.PartitionedData(parts))
            a2 = (d + 2) * (d + 2)
            out = torch.zeros(a2, dtype=torch.float64, device=dev)
            st = engine.stream
            engine.gramian()     # registers
            torch.cuda.synchronize()
            tile = 1024
            tiles = sum(-(-(int(e) - int(s)) // tile) for s, e in zip(offs[:-1], offs[1:]))
            plan = N.gramian_plan("dense", "f32", d, tiles)
            ms = timed(torch, st, a.reps, a.warmup, lambda: engine.ctx.gramian_device(out.data_ptr(), st.cuda_stream))
            nb = plan["blocks"]
            fma = n / 4 * (nb * (nb + 1) // 2) * 1024
            extra = {"rows": n, "features": d, "plan": plan, "Tfma_per_s_median": round(fma / statistics.median(ms) / 1e9, 2),
                     "row_GBps_median": round(n * d * 4 / statistics.median(ms) / 1e6, 1)}
            if "mfma" in best:
                extra["share_of_bare_mfma_rate"] = round(fma / statistics.median(ms) / 1e9 / best["mfma"], 3)
            gram = report(shape, "gramian (gram_dense + gram_merge)", ms, extra)
            so = torch.zeros(1 + 5 * d, dtype=torch.float64, device=dev)
            ms = timed(torch, st, a.reps, a.warmup, lambda: engine.ctx.column_stats_device(so.data_ptr(), st.cuda_stream))
            stats = report(shape, "column_stats (stats_dense)", ms, {"row_GBps_median": round(n * d * 4 / statistics.median(ms) / 1e6, 1)})
            print(json.dumps({"shape": shape, "gramian_over_column_stats": round(gram / stats, 2)}), flush=True)
            Xd = X[:, :d].double()
            torch.cuda.synchronize()
            ms = timed(torch, torch.cuda.current_stream(dev), a.reps, a.warmup, lambda: torch.mm(Xd.t(), Xd))
            mm = report(shape, "torch.mm(X^T, X) float64", ms,
                        {"Tfma_per_s_median": round(n * d * d / statistics.median(ms) / 1e9, 2)})
            print(json.dumps({"shape": shape, "gramian_over_torch_mm": round(gram / mm, 2)}), flush=True)
        except torch.cuda.OutOfMemoryError:
            print(json.dumps({"shape": shape, "skipped": "out of memory"}), flush=True)
        torch.cuda.empty_cache()

    def csr(n, d, P, nnz):
        row_ptr, col, val, y, offs = B.make_csr_shard(torch, dev, n, d, P, "logistic", "f32", 7, nnz)
        parts = [pkg.DeviceCsrPartition(y[s:e], row_ptr[s:e + 1], col, val, d) for s, e in zip(offs[:-1], offs[1:])]
        engine = pkg.HipEngine(pkg.PartitionedData(parts))
        st = engine.stream
        out = torch.zeros((d + 2) * (d + 2), dtype=torch.float64, device=dev)
        engine.gramian()
        torch.cuda.synchronize()
        adds = (nnz + 2) * (nnz + 3) // 2 - 3
        ms = timed(torch, st, a.reps, a.warmup, lambda: engine.ctx.gramian_device(out.data_ptr(), st.cuda_stream))
        gram = report("csr", "gramian (gram_csr + gram_mirror)", ms,
                      {"rows": n, "features": d, "nnz": nnz, "adds_a_row": adds,
                       "atomic_GBps_median": round(n * adds * 8 / statistics.median(ms) / 1e6, 1)})
        w = torch.randn(d, device=dev, dtype=torch.float64)
        go = torch.zeros(d + 2, dtype=torch.float64, device=dev)
        ms = timed(torch, st, a.reps, a.warmup,
                   lambda: engine.ctx.gradient_sum_device(0, w.data_ptr(), 1.0, 0, go.data_ptr(), st.cuda_stream))
        grad = report("csr", "gradient_sum (grad_csr, LDS accumulators)", ms,
                      {"atomic_GBps_median": round(n * nnz * 8 / statistics.median(ms) / 1e6, 1)})
        print(json.dumps({"shape": "csr", "gramian_over_gradient_sum": round(gram / grad, 2)}), flush=True)

    for shape in shapes:
        if shape == "mfma":
            mfma()
        elif shape == "c2":
            dense("c2", a.rows or 10_000_000, 512, 256)
        elif shape == "c3":
            dense("c3", a.rows or 12_500_000, 1024, 256)
        elif shape == "d30":
            dense("d30", a.rows or 10_000_000, 30, 256)
        elif shape == "csr":
            csr(a.rows or 20_000_000, 4096, 256, 32)
        else:
            ap.error(f"unknown shape {shape}")


if __name__ == "__main__":
    main()
