"""Timings of the filter_features passes on one GPU (the numbers of DESIGN.md's filter_features section).

    python tools/filter_bench.py --rows 2000000 --features 256 [--reps 5] [--null] [--cpu-columns 2]

Every device figure is the median of `--reps` repetitions after two warm-up runs, with the minimum and maximum;
kernels are timed with events on the current stream, steps that include host work with a synchronised wall clock.
The CPU baseline runs np.histogram + entropy, np.std and sort + a float64 Python dip (tests/filter_oracle.py) on
`--cpu-columns` columns and is extrapolated to all features over 16 cores."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deep_cartograph_amd import features, hip  # noqa: E402


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dip-columns", type=int, default=0, help="columns per dip chunk (0: as the product chooses)")
    ap.add_argument("--dip-reps", type=int, default=3)
    ap.add_argument("--null", action="store_true", help="time the null distribution at m = 72000, 20000 samples")
    ap.add_argument("--cpu-columns", type=int, default=0)
    a = ap.parse_args()
    n, F = a.rows, a.features
    out = {"rows": n, "features": F, "device": torch.cuda.get_device_name(0)}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    X = torch.empty(n, F, device="cuda", dtype=torch.float32)
    step = max(1, (1 << 28) // F)
    for r in range(0, n, step):
        X[r:r + step] = torch.randn(min(step, n - r), F, generator=gen, device="cuda")
    X[:, ::8] += (torch.rand(n, (F + 7) // 8, generator=gen, device="cuda") < 0.5).float() * 3.0   # every 8th column bimodal
    gbytes = 4.0 * n * F / 1e9

    out["col_stats"] = timed(lambda: hip.col_stats_raw(X), a.reps)
    raw = hip.col_stats_raw(X).cpu().numpy()
    edges = torch.from_numpy(features.histogram_edges(raw[2], raw[3])).cuda()
    out["col_histogram"] = timed(lambda: hip.col_histogram(X, edges), a.reps)
    for k in ("col_stats", "col_histogram"):
        out[k]["TB_per_s"] = gbytes / out[k]["median_ms"]
    print(json.dumps({k: out[k] for k in ("col_stats", "col_histogram")}), flush=True)

    free, _ = torch.cuda.mem_get_info()
    C = a.dip_columns or features._chunk_columns(n, F, free // 2)
    C = min(C, F)
    out["dip_chunk_columns"] = C
    holder = {}

    def do_sort():
        holder["Xs"] = torch.sort(X[:, :C], dim=0).values.contiguous()

    out["sort_chunk"] = timed(do_sort, a.dip_reps, warmup=1)
    print(json.dumps({"dip_chunk_columns": C, "sort_chunk": out["sort_chunk"]}), flush=True)
    out["dip_chunk"] = timed(lambda: hip.dip_sorted(holder["Xs"]), a.dip_reps, warmup=1)
    print(json.dumps({"dip_chunk": out["dip_chunk"]}), flush=True)
    holder.clear()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dips = features.dip_statistic(X)
    out["dip_all_columns_wall_s"] = time.perf_counter() - t0
    if a.null:
        walls = []
        for _ in range(2):
            features._null_cache.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            null = features.dip_null_distribution(72000, 20000, 0)
            walls.append(time.perf_counter() - t0)
        out["null_m72000_B20000_wall_s"] = walls
        p = features.dip_pvalues(dips, n, null, 72000)
        out["columns_with_p_le_0.05"] = int((p <= 0.05).sum())
    print(json.dumps({k: v for k, v in out.items() if k.startswith(("dip_all", "null", "columns"))}), flush=True)

    if a.cpu_columns:
        from scipy.stats import entropy

        from tests import filter_oracle as fo

        cols = X[:, :a.cpu_columns].cpu().numpy()
        t = {"histogram_entropy_s": 0.0, "std_s": 0.0, "sort_s": 0.0, "dip_s": 0.0}
        for c in range(a.cpu_columns):
            col = np.ascontiguousarray(cols[:, c])
            t0 = time.perf_counter()
            hist, be = np.histogram(col, bins=100, density=True)
            entropy(hist * np.diff(be), base=2)
            t1 = time.perf_counter()
            np.std(col)
            t2 = time.perf_counter()
            s = np.sort(col).astype(np.float64)
            t3 = time.perf_counter()
            d = fo.dip(s)
            t4 = time.perf_counter()
            assert abs(d - dips[c]) <= 1e-10
            t["histogram_entropy_s"] += t1 - t0
            t["std_s"] += t2 - t1
            t["sort_s"] += t3 - t2
            t["dip_s"] += t4 - t3
        per_col = {k: v / a.cpu_columns for k, v in t.items()}
        out["cpu_per_column"] = per_col
        out["cpu_all_features_16_cores_s"] = sum(per_col.values()) * F / 16.0
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
