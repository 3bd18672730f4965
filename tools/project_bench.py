"""Timings of hip.featurize_project on one GPU (the numbers of DESIGN.md 4.13).

    python tools/project_bench.py [--frames 1000000] [--atoms 256] [--d 4] [--reps 21]

The workload of DESIGN.md 4.9: `--frames` synthetic frames of `--atoms` atoms, atoms - 3 virtual dihedrals with sin / cos
encoding + atoms distances (762 features at 256 atoms), projected onto `--d` components with all four normalisation
vectors, from dense rows and from DCD planes.  Reported: the fused call, hip.featurize + hip.project_linear on the same
records in the same run (the frames x features matrix allocated once, outside the timing), and a `torch` copy of the
input bytes.  HIP events around the whole call after 3 warm-up calls, median of `--reps` repetitions with the minimum and
maximum.  Also: the peak device memory of projecting the 164-frame fixture of tests/golden two-step with its full
feature configuration (1078 distances + 202 dihedral columns) against fused with the 54 features a model keeps."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deep_cartograph_amd import hip  # noqa: E402
from deep_cartograph_amd import trajectory as tr  # noqa: E402

D, SC = 0, 1


def timed(fn, reps, warmup=3):
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


def workload(A):
    """(records of featurize_project, defs of featurize, F): dihedrals i .. i+3 as sin / cos, then distances i -- i + A/2."""
    rec, F = [], 0
    for i in range(A - 3):
        rec.append([SC, i, i + 1, i + 2, i + 3, F, F + 1, 0])
        F += 2
    for i in range(A):
        rec.append([D, i, (i + A // 2) % A, 0, 0, F, -1, 0])
        F += 1
    rec = np.asarray(rec, dtype=np.int32)
    defs, n_columns, src, _ = tr.records_to_featurize_defs(rec, F)
    assert n_columns == F and len(src) == 0
    return rec, defs, F


def device_cases(n, A, d, reps, out):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    rec, defs, F = workload(A)
    in_gb, matrix_gb = 12.0 * n * A / 1e9, 4.0 * n * F / 1e9
    out["shape"] = {"frames": n, "atoms": A, "records": len(rec), "features": F, "d": d, "input_GB": in_gb, "matrix_GB": matrix_gb,
                    "fused_algorithmic_GB": in_gb + 4.0 * n * d / 1e9, "two_step_algorithmic_GB": in_gb + 2 * matrix_gb + 4.0 * n * d / 1e9}
    src = torch.empty(n * A * 3, device="cuda", dtype=torch.float32)
    dst = torch.empty_like(src)
    out["torch_copy_of_the_input"] = timed(lambda: dst.copy_(src), reps)
    out["torch_copy_of_the_input"]["TB_per_s_read_plus_written"] = 2 * in_gb / out["torch_copy_of_the_input"]["median_ms"]
    del src, dst
    W = torch.randn(F, d, generator=gen, device="cuda")
    vec = dict(fmean=torch.randn(F, generator=gen, device="cuda") * 0.3, frange=torch.rand(F, generator=gen, device="cuda") + 0.5,
               cvmean=torch.randn(d, generator=gen, device="cuda"), cvrange=torch.rand(d, generator=gen, device="cuda") + 0.5)
    dense = (torch.randn(n, A, 3, generator=gen, device="cuda") * 12.0)
    words = 3 * (A + 2)
    results = {}
    for name in ("dense", "planes"):
        if name == "dense":
            xyz, strides = dense, None
        else:
            xyz = torch.full((n * words + 4,), float("nan"), device="cuda", dtype=torch.float32)
            xyz[:n * words].view(n, 3, A + 2)[:, :, 1:A + 1] = dense.transpose(1, 2)
            strides = (n, 1, words, 1, A + 2)
        res = torch.empty(n, d, device="cuda", dtype=torch.float32)
        key = f"fused_{name}"
        out[key] = timed(lambda: hip.featurize_project(xyz, rec, A, F, W, strides=strides, out=res, **vec), reps)
        out[key]["algorithmic_TB_per_s"] = out["shape"]["fused_algorithmic_GB"] / out[key]["median_ms"]
        print(json.dumps({key: out[key]}), flush=True)
        results[name] = res
        X = torch.empty(n, F, device="cuda", dtype=torch.float32)
        two = {}

        def two_step():
            hip.featurize(xyz, defs, A, strides=strides, out=X)
            two["out"] = hip.project_linear(X, W, **vec)[0]

        key = f"two_step_{name}"
        out[key] = timed(two_step, reps)
        out[key]["algorithmic_TB_per_s"] = out["shape"]["two_step_algorithmic_GB"] / out[key]["median_ms"]
        out[key]["featurize_alone"] = timed(lambda: hip.featurize(xyz, defs, A, strides=strides, out=X), reps)
        out[key]["project_alone"] = timed(lambda: hip.project_linear(X, W, **vec), reps)
        out[f"fused_over_two_step_{name}"] = out[f"fused_{name}"]["median_ms"] / out[key]["median_ms"]
        out[f"max_abs_difference_{name}"] = float((res - two["out"]).abs().max())
        print(json.dumps({key: out[key]}), flush=True)
        del X, two
        if name == "planes":
            del xyz
    out["layouts_same_bits"] = bool(torch.equal(results["dense"].view(torch.int32), results["planes"].view(torch.int32)))


def fixture_memory(out):
    """Peak device bytes (beyond the uploaded file) of projecting the reference's fixture: two-step with the full features
    configuration of the training run against fused with the model's 54 names."""
    golden = os.path.join(ROOT, "tests", "golden")
    g = np.load(os.path.join(golden, "compute_features_golden.npz"))
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        dcd, pdb = os.path.join(d, "CA_example.dcd"), os.path.join(d, "CA_example.pdb")
        with open(dcd, "wb") as f:
            f.write(g["dcd"].tobytes())
        with open(pdb, "w") as f:
            f.write(str(g["pdb"]))
        top = tr.read_topology(pdb)
        traj = tr.open_trajectory(dcd, top.n_atoms)
        flat = torch.from_numpy(np.array(traj.data)).cuda()
    full = {"distance_groups": {"dist": {"first_selection": "all", "second_selection": "all", "first_stride": 1, "second_stride": 10,
                                         "skip_neigh_residues": False, "skip_bonded_atoms": True}},
            "dihedral_groups": {"tor": {"selection": "all", "periodic_encoding": True, "search_mode": "virtual"}}}
    all_names, all_defs = tr.feature_definitions(full, top)
    names = [str(s) for s in np.load(os.path.join(golden, "features_164x54.npz"))["names"]]
    lin = np.load(os.path.join(golden, "linear_models.npz"))
    keep = torch.tensor([all_names.index(s) for s in names], device="cuda")
    W = torch.from_numpy(np.ascontiguousarray(lin["pca.cv_weights"])).cuda()
    vec = {k: torch.from_numpy(lin[f"pca.{v}"]).cuda() for k, v in (("fmean", "features_norm_mean"), ("frange", "features_norm_range"),
                                                                      ("cvmean", "cv_norm_mean"), ("cvrange", "cv_norm_range"))}
    rec = tr.definitions_from_labels(names, top)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    X = hip.featurize(flat, all_defs, top.n_atoms, strides=traj.layout())
    two, _ = hip.project_linear(X[:, keep].contiguous(), W, **vec)
    torch.cuda.synchronize()
    peak_two = torch.cuda.max_memory_allocated() - base
    del X
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fused, _ = hip.featurize_project(flat, rec, top.n_atoms, len(names), W, strides=traj.layout(), **vec)
    torch.cuda.synchronize()
    peak_fused = torch.cuda.max_memory_allocated() - base
    out["fixture_164_frames"] = {"two_step_features": len(all_names), "two_step_peak_bytes": int(peak_two), "fused_features": len(names),
                                 "fused_peak_bytes": int(peak_fused), "fused_workspace_bytes_of_that": int(
                                     hip._lib.load().dcv_featurize_project_workspace(traj.n_frames, top.n_atoms, len(rec), len(names), 2)),
                                 "max_abs_difference": float((fused - two).abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--atoms", type=int, default=256)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    fixture_memory(out)
    print(json.dumps({"fixture_164_frames": out["fixture_164_frames"]}), flush=True)
    device_cases(a.frames, a.atoms, a.d, a.reps, out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
