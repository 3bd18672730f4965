"""Timings of hip.transform_frames on one GPU (the numbers of DESIGN.md 4.12).

    python tools/transform_bench.py [--frames 1000000] [--atoms 256] [--reps 21] [--long-frames 2000] [--long-atoms 100000]
                                    [--tool-frames 0] [--cpu-frames 0]

A per-frame rigid transform of `--frames` synthetic frames of `--atoms` atoms, dense -> dense and DCD planes -> DCD record
image, and of `--long-frames` x `--long-atoms` for long rows, beside a `torch` copy of the same bytes from the same run.
Reported per case: time, algorithmic bytes (12 read + 12 written per atom and frame) over time, and that as a fraction of
the copy's rate.  Device figures: HIP events around the whole call after 3 warm-up calls, median of `--reps` repetitions
with the minimum and maximum.  `--tool-frames N` also times tools.align_trajectories end to end (fit + transform + file
write, wall clock) on a DCD file of N frames written to a temporary folder, and `--cpu-frames M` the NumPy oracle
(tests/align_oracle.py: Kabsch fit + transform) on 16 processes of M frames each."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deep_cartograph_amd import hip  # noqa: E402


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


def _oracle_worker(args):
    seed, frames, atoms = args
    from tests import align_oracle as ao
    from tests import geometry_oracle as go

    xyz, ref = go.synthetic(frames, atoms, seed)
    fit = np.arange(0, atoms, 2)
    t0 = time.perf_counter()
    ao.transform(xyz, ao.fit_transforms(xyz, fit, ref[fit])).astype(np.float32)
    return time.perf_counter() - t0


def transforms(n, gen):
    """[n, 16] float64: a rotation about z, centroids of a few hundred Angstrom; the arithmetic does not depend on the data."""
    ang = torch.rand(n, generator=gen, device="cuda", dtype=torch.float64) * 6.2831853
    rows = torch.zeros(n, 16, device="cuda", dtype=torch.float64)
    rows[:, 0], rows[:, 1], rows[:, 3], rows[:, 4], rows[:, 8] = torch.cos(ang), torch.sin(ang), -torch.sin(ang), torch.cos(ang), 1.0
    rows[:, 9:15] = (torch.rand(n, 6, generator=gen, device="cuda", dtype=torch.float64) - 0.5) * 600.0
    return rows


def device_cases(n, A, reps, tag, out):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    gbytes = 24.0 * n * A / 1e9
    out[f"{tag}_shape"] = {"frames": n, "atoms": A, "GB_read_plus_written": gbytes}
    src = torch.empty(int(gbytes * 1e9 / 8), device="cuda", dtype=torch.float32)   # a copy moves its bytes twice: read + write
    dst = torch.empty_like(src)
    copy = timed(lambda: dst.copy_(src), reps)
    copy["TB_per_s"] = gbytes / copy["median_ms"]
    out[f"{tag}_torch_copy"] = copy
    del src, dst
    rows = transforms(n, gen)
    dense = (torch.rand(n, A, 3, generator=gen, device="cuda") - 0.5) * 600.0
    words = 3 * (A + 2)
    results = {}
    for name in ("dense", "planes"):
        if name == "dense":
            xyz, strides = dense, None
            target, out_strides = torch.empty(n * A * 3, device="cuda", dtype=torch.float32), (0, 3 * A, 3, 1)
        else:
            xyz = torch.full((n * words + 4,), float("nan"), device="cuda", dtype=torch.float32)
            xyz[:n * words].view(n, 3, A + 2)[:, :, 1:A + 1] = dense.transpose(1, 2)
            strides = (n, 1, words, 1, A + 2)
            target, out_strides = torch.zeros(n * words, device="cuda", dtype=torch.float32), (1, words, 1, A + 2)
        key = f"{tag}_transform_{name}"
        out[key] = timed(lambda: hip.transform_frames(xyz, A, rows, strides=strides, out=target, out_strides=out_strides), reps)
        out[key]["TB_per_s"] = gbytes / out[key]["median_ms"]
        out[key]["fraction_of_copy"] = out[key]["TB_per_s"] / copy["TB_per_s"]
        results[name] = (target.view(n, A, 3) if name == "dense" else target.view(n, 3, A + 2)[:, :, 1:A + 1].transpose(1, 2)).clone()
        print(json.dumps({key: out[key]}), flush=True)
        if name == "planes":
            del xyz
        del target
    out[f"{tag}_layouts_same_bits"] = bool(torch.equal(results["dense"].view(torch.int32), results["planes"].contiguous().view(torch.int32)))
    from tests import align_oracle as ao
    from tests import features_oracle as fo

    head = min(n, 64)
    want = ao.transform(dense[:head].cpu().numpy(), rows[:head].cpu().numpy()).astype(np.float32)
    out[f"{tag}_first_frames_max_ulp"] = int(fo.ulp_distance_f32(results["dense"][:head].cpu().numpy(), want).max())


def whole_tool(n, A, out):
    from deep_cartograph_amd import tools, trajectory

    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    with tempfile.TemporaryDirectory() as d:
        names = ["CA"] * A
        ref = (torch.randn(A, 3, generator=gen, device="cuda") * 20.0)
        top = trajectory.Topology(names, ["ALA", "GLY", "SER", "LEU"] * (A // 4) + ["ALA"] * (A % 4), ["A"] * A, ["A"] * A,
                                  np.arange(1, A + 1, dtype=np.int64) % 10000, ref.cpu().numpy(), None)
        pdb, dcd = os.path.join(d, "system.pdb"), os.path.join(d, "system.dcd")
        trajectory.write_topology(pdb, top)
        with trajectory.write_dcd(dcd, A) as w:
            step = 100_000
            for lo in range(0, n, step):
                m = min(step, n - lo)
                frames = ref[None] + torch.randn(m, A, 3, generator=gen, device="cuda") + (torch.rand(m, 1, 3, generator=gen, device="cuda") - 0.5) * 600.0
                image = torch.zeros(m, 3, A + 2, device="cuda", dtype=torch.float32)
                image[:, :, 1:A + 1] = frames.transpose(1, 2)
                w.append(image.cpu().numpy().reshape(-1))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tools.align_trajectories(dcd, pdb, output_folder=os.path.join(d, "aligned"))
        torch.cuda.synchronize()
        out["whole_tool"] = {"frames": n, "atoms": A, "fit_atoms": A, "wall_s": time.perf_counter() - t0,
                             "output_bytes": os.path.getsize(os.path.join(d, "aligned", "system.dcd"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--atoms", type=int, default=256)
    ap.add_argument("--long-frames", type=int, default=2000)
    ap.add_argument("--long-atoms", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--tool-frames", type=int, default=0, help="frames of the end-to-end run of tools.align_trajectories (0: skip)")
    ap.add_argument("--cpu-frames", type=int, default=0, help="frames per process of the 16-process NumPy oracle (0: skip)")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    device_cases(a.frames, a.atoms, a.reps, "short_rows", out)
    if a.long_frames:
        device_cases(a.long_frames, a.long_atoms, a.reps, "long_rows", out)
    if a.tool_frames:
        whole_tool(a.tool_frames, a.atoms, out)
        print(json.dumps({"whole_tool": out["whole_tool"]}), flush=True)
    if a.cpu_frames:
        import multiprocessing as mp

        t0 = time.perf_counter()
        with mp.get_context("spawn").Pool(16) as pool:
            each = pool.map(_oracle_worker, [(i, a.cpu_frames, a.atoms) for i in range(16)])
        out["oracle_16_processes"] = {"frames_each": a.cpu_frames, "atoms": a.atoms, "slowest_s": max(each),
                                      "with_pool_start_s": time.perf_counter() - t0}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
