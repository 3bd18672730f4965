"""Timings of hierarchical clustering on one GPU (the numbers of DESIGN.md's linkage section).

    python tools/linkage_bench.py --n 8000 20000 --d 2 --method complete [--reps 3] [--cpu-max-n 20000]

Per n: the distance matrix alone (events around dcv_linkage_pdist), the whole hip.linkage call (synchronised wall
clock: it reads the merge counter between blocks of steps), the number of row searches the chain ran, the time per
chain step (one search launch + one update launch; chain = whole call - matrix) and the whole
statistics.cluster_data call.  Every device figure is the median of `--reps` runs after one warm-up.  The baseline is
scikit-learn's AgglomerativeClustering on the same points with the CPUs this process may use, skipped above
`--cpu-max-n`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deep_cartograph_amd import _lib, hip, statistics  # noqa: E402


def make_points(n, d, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.uniform(-0.8, 0.8, (6, d))
    P = c[rng.integers(0, 6, n)] + 0.07 * rng.standard_normal((n, d))
    return np.round(np.clip(P, -1, 1), 4)


def wall(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), float(max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[8000])
    ap.add_argument("--d", type=int, default=2)
    ap.add_argument("--method", default="complete", choices=sorted(hip.LINKAGE_METHOD))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-max-n", type=int, default=20000)
    a = ap.parse_args()
    lib = _lib.load()
    for n in a.n:
        P = make_points(n, a.d)
        Pd = torch.from_numpy(P).cuda()
        out = {"n": n, "d": a.d, "method": a.method, "device": torch.cuda.get_device_name(0),
               "workspace_GB": hip.linkage_workspace_bytes(n, a.d) / 1e9}
        ws = torch.empty(hip.linkage_workspace_bytes(n, a.d), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        ms = []
        for r in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(lib.dcv_linkage_pdist(Pd.data_ptr(), n, a.d, ws.data_ptr(), ws.numel(), stream), "dcv_linkage_pdist")
            e1.record()
            e1.synchronize()
            if r:
                ms.append(e0.elapsed_time(e1))
        del ws
        out["pdist_ms"] = float(np.median(ms))
        out["pdist_TB_per_s"] = 8.0 * n * n / 1e9 / out["pdist_ms"]
        res = {}

        def run():
            res["Z"], res["searches"] = hip.linkage(Pd, a.method, return_searches=True)

        med, lo, hi = wall(run, a.reps)
        out["linkage_s"] = {"median": med, "min": lo, "max": hi}
        out["searches"] = res["searches"]
        out["searches_per_n"] = res["searches"] / n
        out["chain_s"] = med - out["pdist_ms"] / 1e3
        out["us_per_step"] = out["chain_s"] / res["searches"] * 1e6
        settings = {"algorithm": "hierarchical", "linkage": a.method, "num_clusters": 6}
        med, lo, hi = wall(lambda: res.__setitem__("labels", statistics.cluster_data(P, dict(settings))[0]), a.reps)
        out["cluster_data_s"] = {"median": med, "min": lo, "max": hi}
        if n <= a.cpu_max_n:
            from sklearn.cluster import AgglomerativeClustering

            t0 = time.perf_counter()
            ref = AgglomerativeClustering(n_clusters=6, linkage=a.method).fit_predict(P)
            out["sklearn_s"] = time.perf_counter() - t0
            out["cpus"] = len(os.sched_getaffinity(0))
            out["labels_equal"] = bool(np.array_equal(ref, res["labels"]))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
