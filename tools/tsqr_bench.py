#!/usr/bin/env python3
"""Time psgd_tsqr_device on device-resident f32 dense rows, beside its yardsticks on the same rows
(diagnostic tool). Each shape runs in a process of its own; in it the calls alternate, one launch of
each a round, so that clocks and cache state are shared evenly:

  tsqr:    psgd_tsqr_device (tsqr_dense over the rows, then the merge levels);
  merge:   psgd_tsqr_rows_device over items * a_pad rows of a columns: the merge levels' tree of the
           same kernel over as many rows as the items' R factors have, their share of the time;
  gramian: psgd_gramian_device (gram_dense + gram_merge), the pass the QR stands beside;
  stats:   psgd_column_stats_device (stats_dense), the row stream;
  qr:      torch.linalg.qr(X.double(), mode="r"), the library's QR of a float64 copy.

Shapes: 10M x 30, 10M x 64, 4M x 127. HIP events around each launch, 20 after 3; one JSON line per call:
median and min ms, and T fma/s counted as 2 n a^2 over the median, against the 39.1 T fma/s bare rate
of v_mfma_f64_16x16x4_f64 (tools/gram_bench.py --shape mfma).

usage: python tools/tsqr_bench.py [--shape d30,d64,d127 | all] [--rows N] [--reps K]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"d30": (10_000_000, 30), "d64": (10_000_000, 64), "d127": (4_000_000, 127)}
BARE_TFMA = 39.1


def one_shape(shape, n, d, reps, warmup):
    import torch
    import __graft_entry__ as g
    import bench as B
    pkg = g.load_package()
    N = pkg._native
    dev = torch.device("cuda", 0)
    P = 256
    X, y, offs = B.make_shard(torch, dev, n, (d + 3) // 4 * 4, P, "least_squares", "f32", 7)
    parts = [pkg.DevicePartition(y[s:e], X[s:e], d) for s, e in zip(offs[:-1], offs[1:])]
    engine = pkg.HipEngine(pkg.PartitionedData(parts))
    st = engine.stream
    a = d + 1
    engine.tsqr()   # registers
    tiles = sum(-(-(int(e) - int(s)) // 1024) for s, e in zip(offs[:-1], offs[1:]))
    plan = N.tsqr_plan("f32", d, tiles)
    out = torch.zeros(a * a, dtype=torch.float64, device=dev)
    gout = torch.zeros((d + 2) * (d + 2), dtype=torch.float64, device=dev)
    sout = torch.zeros(1 + 5 * d, dtype=torch.float64, device=dev)
    mrows = torch.randn(plan["items"] * plan["a_pad"], a, dtype=torch.float64, device=dev)
    Xd = X[:, :d].double()
    torch.cuda.synchronize()
    calls = [
        ("tsqr (tsqr_dense + merge levels)", lambda: engine.ctx.tsqr_device(out.data_ptr(), st.cuda_stream)),
        ("merge (tsqr_rows over items * a_pad rows)",
         lambda: engine.ctx.tsqr_rows_device(mrows.data_ptr(), mrows.shape[0], a, out.data_ptr(), st.cuda_stream)),
        ("gramian (gram_dense + gram_merge)", lambda: engine.ctx.gramian_device(gout.data_ptr(), st.cuda_stream)),
        ("column_stats (stats_dense)", lambda: engine.ctx.column_stats_device(sout.data_ptr(), st.cuda_stream)),
        ("torch.linalg.qr(X.double(), mode='r')", lambda: torch.linalg.qr(Xd, mode="r")),
    ]
    ms = {name: [] for name, _ in calls}
    with torch.cuda.stream(st):
        for k in range(warmup + reps):
            for name, call in calls:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                call()
                e1.record(st)
                e1.synchronize()
                if k >= warmup:
                    ms[name].append(e0.elapsed_time(e1))
    med = {}
    for name, _ in calls:
        med[name] = statistics.median(ms[name])
        line = {"shape": shape, "rows": n, "features": d, "call": name, "reps": len(ms[name]),
                "ms_median": round(med[name], 4), "ms_min": round(min(ms[name]), 4)}
        if name.startswith("tsqr") or name.startswith("torch"):
            rate = 2.0 * n * a * a / med[name] / 1e9
            line["Tfma_per_s_median"] = round(rate, 3)
            line["share_of_bare_mfma_rate"] = round(rate / BARE_TFMA, 4)
        if name.startswith("tsqr"):
            line["plan"] = plan
        print(json.dumps(line), flush=True)
    names = [name for name, _ in calls]
    t = med[names[0]]
    print(json.dumps({"shape": shape, "merge_share_of_tsqr": round(med[names[1]] / t, 3),
                      "tsqr_over_gramian": round(t / med[names[2]], 2), "tsqr_over_column_stats": round(t / med[names[3]], 2),
                      "tsqr_over_torch_qr": round(t / med[names[4]], 3),
                      "bar": "met" if t < med[names[4]] else "bar missed"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of each shape's own (smaller boxes)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    shapes = list(SHAPES) if a.shape == "all" else a.shape.split(",")
    for s in shapes:
        if s not in SHAPES:
            ap.error(f"unknown shape {s}")
    if a.child:
        n, d = SHAPES[shapes[0]]
        one_shape(shapes[0], a.rows or n, d, a.reps, a.warmup)
        return
    for s in shapes:   # a fresh process a shape
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shape", s, "--rows", str(a.rows),
                             "--reps", str(a.reps), "--warmup", str(a.warmup)]).returncode
        if rc:
            sys.exit(rc)


if __name__ == "__main__":
    main()
