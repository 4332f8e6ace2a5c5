#!/usr/bin/env python3
"""Time the train/test split kernels on device-resident data at the flagship shapes (diagnostic tool):

  c2: 10M x 512 f32 dense rows in 256 partitions;
  c4: 20M rcv1-like CSR rows, 47,236 features, 94 non-zeros, f32 values, 256 partitions.

Per shape, after an untimed prewarm (the calls repeated for --prewarm-s seconds, as bench.py warms
its chain kernel) and a warm-up: HIP events around psgd_cell_select_device (the [0, 0.6) cell of
seed 11) and around the gather alone (psgd_gather_dense_device / psgd_gather_csr_device of that
cell into preallocated tensors); wall time of the whole randomSplit([0.6, 0.4], 11), read-backs and
allocations included. One JSON line per measurement with median and min milliseconds and, for the
gathers, the bytes read + written over the time (dense: 2 x kept rows x d x 4; CSR: 2 x kept
non-zeros x 8 + 3 x kept rows x 8 for the row pointers read and written).

In the same session at c2, the yardsticks: torch.index_select of the same rows (the library gather
a torch-built split would use), and --transform adds psgd_transform_columns_device, the project's
read + write stream over the same shape (host-registered rows, as tools/colstats_bench.py does).

usage: python tools/split_bench.py [--shape c2|c4|both] [--rows N] [--partitions P] [--reps K] [--transform]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    # name: (rows, features, partitions, nnz (0: dense))
    "c2": (10_000_000, 512, 256, 0),
    "c4": (20_000_000, 47_236, 256, 94),
}
WEIGHTS, SEED = [0.6, 0.4], 11


def timed(torch, st, reps, warmup, prewarm_s, call):
    ms = []
    with torch.cuda.stream(st):
        t0 = time.perf_counter()
        while prewarm_s > 0 and time.perf_counter() - t0 < prewarm_s:
            call()
            st.synchronize()
        for k in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            if k >= warmup:
                ms.append(e0.elapsed_time(e1))
    return ms


def report(line, ms, nbytes=0):
    med, lo = statistics.median(ms), min(ms)
    line.update({"reps": len(ms), "ms_median": round(med, 4), "ms_min": round(lo, 4)})
    if nbytes:
        line.update({"bytes_moved": int(nbytes), "GBps_median": round(nbytes / med / 1e6, 1),
                     "GBps_best": round(nbytes / lo / 1e6, 1)})
    print(json.dumps(line), flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["c2", "c4", "both"])
    ap.add_argument("--rows", type=int, default=0, help="rows instead of the shape's own (smaller boxes)")
    ap.add_argument("--partitions", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prewarm-s", type=float, default=1.0)
    ap.add_argument("--transform", action="store_true", help="also time the column transform at the c2 shape")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")

    import numpy as np
    import torch
    import __graft_entry__ as g
    import bench as B
    pkg = g.load_package()
    N = pkg._native
    dev = torch.device("cuda", 0)
    gather_ms, gather_bytes = {}, 0

    for name in (["c2", "c4"] if a.shape == "both" else [a.shape]):
        n, d, P, nnz = SHAPES[name]
        n, P = a.rows or n, a.partitions or P
        if nnz:
            row_ptr, col, val, y, offs = B.make_csr_shard(torch, dev, n, d, P, "logistic", "f32", 7, nnz)
            parts = [pkg.DeviceCsrPartition(y[s:e], row_ptr[s:e + 1], col, val, d) for s, e in zip(offs[:-1], offs[1:])]
        else:
            X, y, offs = B.make_shard(torch, dev, n, d, P, "least_squares", "f32", 7)
            parts = [pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])]
        data = pkg.PartitionedData(parts)
        engine = pkg.HipEngine(data)
        ctx, st = engine.ctx, engine.stream
        base = {"shape": name, "rows": n, "features": d, "partitions": P, "nnz": nnz}
        rows = torch.empty(n, dtype=torch.int32, device=dev)
        cn = torch.zeros(2 * P, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ms = timed(torch, st, a.reps, a.warmup, a.prewarm_s,
                   lambda: ctx.cell_select_device(SEED, N.SEED_PLUS_INDEX, 0.0, 0.6, False, rows.data_ptr(), cn.data_ptr(),
                                                  cn.data_ptr() + 8 * P, st.cuda_stream))
        h = cn.cpu().numpy()
        counts, nz = h[:P].copy(), h[P:].copy()
        m0 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        M = int(m0[-1])
        report(dict(base, call="cell_select", kept_rows=M, ns_per_row_median=round(statistics.median(ms) * 1e6 / n, 3)), ms)
        yo = torch.empty(M, dtype=torch.float64, device=dev)
        ys = [yo[int(m0[i]): int(m0[i + 1])].data_ptr() for i in range(P)]
        if nnz:
            z0 = np.concatenate([[0], np.cumsum(nz)]).astype(np.int64)
            Z = int(z0[-1])
            rp = torch.empty(M + P, dtype=torch.int64, device=dev)
            co = torch.empty(Z, dtype=torch.int32, device=dev)
            vo = torch.empty(Z, dtype=torch.float32, device=dev)
            rps = [rp.data_ptr() + 8 * (int(m0[i]) + i) for i in range(P)]
            cos = [co.data_ptr() + 4 * int(z0[i]) for i in range(P)]
            vos = [vo.data_ptr() + 4 * int(z0[i]) for i in range(P)]
            call = lambda: ctx.gather_csr_device(rows.data_ptr(), counts, nz, ys, rps, cos, vos, st.cuda_stream)
            nbytes = 2 * Z * 8 + 3 * M * 8
            what = "gather_csr"
        else:
            Xo = torch.empty((M, d), dtype=torch.float32, device=dev)
            xs = [Xo[int(m0[i]): int(m0[i + 1])].data_ptr() for i in range(P)]
            call = lambda: ctx.gather_dense_device(rows.data_ptr(), counts, d, xs, ys, st.cuda_stream)
            nbytes = 2 * M * d * 4
            what = "gather_dense"
        ms = timed(torch, st, a.reps, a.warmup, a.prewarm_s, call)
        gather_ms[name] = report(dict(base, call=what, kept_rows=M), ms, nbytes)
        gather_bytes = nbytes
        if not nnz:
            # the same rows through the library gather: global indices of the kept rows
            starts = torch.tensor(np.repeat(np.asarray(offs[:-1], dtype=np.int64), counts), device=dev)
            local = torch.cat([rows[int(offs[i]): int(offs[i]) + int(counts[i])] for i in range(P)]).to(torch.int64)
            idx = starts + local
            torch.cuda.synchronize()
            ms = timed(torch, st, a.reps, a.warmup, a.prewarm_s, lambda: torch.index_select(X, 0, idx, out=Xo))
            med = report(dict(base, call="torch.index_select", kept_rows=M), ms, nbytes)
            print(json.dumps({"shape": name, "gather_dense_over_index_select": round(gather_ms[name] / med, 3)}), flush=True)
            del starts, local, idx, Xo
        del yo
        torch.cuda.empty_cache()
        wall = []
        for k in range(3 + 5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pkg.randomSplit(data, WEIGHTS, SEED, engine=engine)
            torch.cuda.synchronize()
            if k >= 3:
                wall.append((time.perf_counter() - t0) * 1e3)
            sizes = [s.count() for s in out]
            del out
        report(dict(base, call="randomSplit([0.6, 0.4]) wall", split_rows=sizes), wall)
        del engine, data, parts
        torch.cuda.empty_cache()

    if a.transform:
        n, d, P, _ = SHAPES["c2"]
        n, P = a.rows or n, a.partitions or P
        per = -(-n // P)
        block = np.zeros((per, d), dtype=np.float32)
        labels = np.zeros(per)
        engine = pkg.HipEngine(pkg.PartitionedData([pkg.DensePartition(labels, block) for _ in range(P)]))
        st = engine.stream
        factor = torch.ones(d, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        nbytes = 2 * per * P * d * 4
        ms = timed(torch, st, a.reps, a.warmup, a.prewarm_s,
                   lambda: engine.ctx.transform_columns_device(None, factor.data_ptr(), st.cuda_stream))
        med = report({"shape": "c2", "call": "transform_dense", "rows": per * P, "features": d, "partitions": P}, ms,
                     nbytes)
        if "c2" in gather_ms and a.shape == "c2":
            # time per byte moved (the gather moved the kept rows only)
            ratio = (gather_ms["c2"] / gather_bytes) / (med / nbytes)
            print(json.dumps({"shape": "c2", "gather_dense_over_transform_per_byte": round(ratio, 3)}), flush=True)


if __name__ == "__main__":
    main()
