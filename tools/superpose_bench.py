"""Timings of hip.superpose on one GPU (the numbers of DESIGN.md 4.10).

    python tools/superpose_bench.py [--frames 1000000] [--atoms 256] [--reps 21] [--cpu-frames 62500]

RMSD + moments of `--frames` synthetic frames of `--atoms` atoms, fit on all atoms, in both layouts (dense (n, A, 3)
rows and DCD planes), beside three references from the same run: a `torch` copy of the same bytes, dcv_featurize's
staging-plus-stores case of DESIGN.md 4.9 (128 distances that name every atom: it reads the same bytes) and the NumPy
float64 oracle (tests/geometry_oracle.py) on 16 processes of `--cpu-frames` frames each.  The launch is also timed
with fewer outputs, which separates its phases: fit RMSD only (staging + fit + solve), RMSD of the selection (+ the
second residual pass), moments (+ phase B).  Device figures: HIP events around the whole call after 3 warm-up calls,
median of `--reps` repetitions with the minimum and maximum."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deep_cartograph_amd import hip  # noqa: E402
from deep_cartograph_amd._lib import FEAT_DISTANCE  # noqa: E402


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
    from tests import geometry_oracle as go

    xyz, ref = go.synthetic(frames, atoms, seed)
    fit = np.arange(atoms)
    t0 = time.perf_counter()
    go.superpose(xyz, fit, ref, fit, ref)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--atoms", type=int, default=256)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--cpu-frames", type=int, default=0, help="frames per process of the 16-process NumPy oracle (0: skip)")
    a = ap.parse_args()
    n, A = a.frames, a.atoms
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    ref = torch.randn(A, 3, generator=gen, device="cuda") * 20.0
    # per frame a rotation about z, a translation and 1 Angstrom of noise: the arithmetic does not depend on the data
    ang = torch.rand(n, generator=gen, device="cuda") * 6.2831853
    c, s = torch.cos(ang), torch.sin(ang)
    dense = torch.empty(n, A, 3, device="cuda", dtype=torch.float32)
    dense[:, :, 0] = c[:, None] * ref[None, :, 0] - s[:, None] * ref[None, :, 1]
    dense[:, :, 1] = s[:, None] * ref[None, :, 0] + c[:, None] * ref[None, :, 1]
    dense[:, :, 2] = ref[None, :, 2]
    dense += torch.randn(n, A, 3, generator=gen, device="cuda")
    dense += (torch.rand(n, 1, 3, generator=gen, device="cuda") - 0.5) * 600.0
    words = 3 * (A + 2)
    planes = torch.full((n * words + 4,), float("nan"), device="cuda", dtype=torch.float32)
    planes[:n * words].view(n, 3, A + 2)[:, :, 1:A + 1] = dense.transpose(1, 2)
    layouts = {"dense": (dense, None), "planes": (planes, (n, 1, words, 1, A + 2))}
    fit = np.arange(A)
    ref_h = ref.double().cpu().numpy()
    gbytes = 12.0 * n * A / 1e9
    out = {"frames": n, "atoms": A, "GB_read": gbytes, "device": torch.cuda.get_device_name(0)}

    src = torch.empty(int(gbytes * 1e9 / 8), device="cuda", dtype=torch.float32)   # a copy moves its bytes twice: read + write
    dst = torch.empty_like(src)
    out["torch_copy"] = timed(lambda: dst.copy_(src), a.reps)
    out["torch_copy"]["TB_per_s"] = gbytes / out["torch_copy"]["median_ms"]
    del src, dst
    defs = np.zeros((128, 6), dtype=np.int32)
    defs[:, 0], defs[:, 1], defs[:, 2], defs[:, 5] = FEAT_DISTANCE, np.arange(0, A, 2)[:128] % A, np.arange(1, A, 2)[:128] % A, np.arange(128)
    results = {}
    for name, (buf, strides) in layouts.items():
        feat = torch.empty(n, 128, device="cuda", dtype=torch.float32)
        out[f"featurize_staging_{name}"] = timed(lambda: hip.featurize(buf, defs, A, strides=strides, out=feat), a.reps)
        del feat
        for label, kw in (("fit_rmsd", dict(want=("rmsd",))), ("rmsd", dict(sel=fit, sel_ref=ref_h, want=("rmsd",))),
                          ("rmsd_moments", dict(sel=fit, sel_ref=ref_h, want=("rmsd", "moments")))):
            key = f"superpose_{label}_{name}"
            out[key] = timed(lambda: hip.superpose(buf, A, fit, ref_h, strides=strides, **kw), a.reps)
            out[key]["TB_per_s"] = gbytes / out[key]["median_ms"]
        results[name] = {k: v.cpu().numpy() for k, v in hip.superpose(buf, A, fit, ref_h, sel=fit, sel_ref=ref_h, strides=strides,
                                                                     want=("rmsd", "moments")).items()}
        print(json.dumps({k: v for k, v in out.items() if k.endswith(name)}), flush=True)
    out["layouts_same_bits"] = all(np.array_equal(results["dense"][k], results["planes"][k]) for k in ("rmsd", "moments"))
    from tests import geometry_oracle as go

    head = go.superpose(dense[:2000].cpu().numpy(), fit, ref_h, fit, ref_h)
    out["first_2000_frames_max_rmsd_error"] = float(np.abs(results["dense"]["rmsd"][:2000] - head["rmsd"]).max())
    if a.cpu_frames:
        import multiprocessing as mp

        t0 = time.perf_counter()
        with mp.get_context("spawn").Pool(16) as pool:
            each = pool.map(_oracle_worker, [(i, a.cpu_frames, A) for i in range(16)])
        out["oracle_16_processes"] = {"frames_each": a.cpu_frames, "slowest_s": max(each), "with_pool_start_s": time.perf_counter() - t0}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
