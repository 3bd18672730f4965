"""Timings of HDBSCAN on one GPU (the numbers of DESIGN.md's HDBSCAN section).

    python tools/hdbscan_bench.py --n 8000 20000 65536 262144 --min-samples 3 16 [--reps 3] [--cpu-max-s 60]

Per n and min_samples, on a 2-D mixture rounded to 4 decimals: the core distances (hip.core_distances), the minimum
spanning tree (hip.mr_mst: n - 1 Prim steps, one launch each; microseconds per step = that time / (n - 1)), the host
finish (hdbscan.finish: sort, single-linkage tree, condensation, selection, labels, centroids) and the whole
statistics.cluster_data call with min_cluster_size = 50.  Both device calls synchronise, so every figure is a
synchronised wall clock: the median of `--reps` runs after one warm-up.  The baseline is the live
sklearn.cluster.HDBSCAN on the same points with the CPUs this process may use; it is skipped once its time,
extrapolated quadratically from the previous size, passes `--cpu-max-s` seconds."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deep_cartograph_amd import hdbscan, hip, statistics  # noqa: E402

MIN_CLUSTER_SIZE = 50


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
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[8000, 20000, 65536, 262144])
    ap.add_argument("--d", type=int, default=2)
    ap.add_argument("--min-samples", type=int, nargs="+", default=[3, 16])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-max-s", type=float, default=60.0)
    a = ap.parse_args()
    for k in a.min_samples:
        last = None   # (n, seconds) of the last scikit-learn fit
        for n in sorted(a.n):
            P = make_points(n, a.d)
            Pd = torch.from_numpy(P).cuda()
            out = {"n": n, "d": a.d, "min_samples": k, "min_cluster_size": MIN_CLUSTER_SIZE, "device": torch.cuda.get_device_name(0),
                   "workspace_MB": (hip.mr_mst_workspace_bytes(n, a.d) + hip.core_distances_workspace_bytes(n, a.d, k)) / 1e6}
            res = {}
            out["core_s"] = wall(lambda: res.__setitem__("core", hip.core_distances(Pd, k)), a.reps)
            out["mst_s"] = wall(lambda: res.__setitem__("mst", hip.mr_mst(Pd, res["core"])), a.reps)
            out["us_per_step"] = out["mst_s"] / (n - 1) * 1e6
            out["finish_s"] = wall(lambda: hdbscan.finish(P, *res["mst"], MIN_CLUSTER_SIZE), a.reps)
            settings = {"algorithm": "hdbscan", "min_cluster_size": MIN_CLUSTER_SIZE, "min_samples": k}
            out["cluster_data_s"] = wall(lambda: res.__setitem__("labels", statistics.cluster_data(P, dict(settings))[0]), a.reps)
            out["clusters"] = int(res["labels"].max()) + 1
            guess = last[1] * (n / last[0]) ** 2 if last else 0.0
            if guess <= a.cpu_max_s:
                from sklearn.cluster import HDBSCAN

                t0 = time.perf_counter()
                ref = HDBSCAN(min_cluster_size=MIN_CLUSTER_SIZE, min_samples=k, store_centers="centroid").fit(P)
                out["sklearn_s"] = time.perf_counter() - t0
                out["cpus"] = len(os.sched_getaffinity(0))
                out["labels_equal"] = bool(np.array_equal(ref.labels_, res["labels"]))
                last = (n, out["sklearn_s"])
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
