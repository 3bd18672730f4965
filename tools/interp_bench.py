"""Timings of hip.interpolate on one GPU (the numbers of DESIGN.md 4.11).

    python tools/interp_bench.py [--atoms 20000] [--reps 11] [--cpu-atoms 2000]

Two shapes, both kinds, with and without noise, dense rows in and out (and DCD planes in and out for PCHIP):
  upsampling       200 knots -> 20 000 frames: write-bound, the case of a short morph between two states;
  near-unit ratio  10 000 knots -> 10 000 frames: every knot is read once and one frame written per knot.
Algorithmic bytes of a call: 12 per output frame and atom written, 24 more read with noise, 12 per knot and atom read
(twice for makima, whose threshold needs a pass of its own).  The achieved bandwidth is those bytes over the time of the
whole call -- the upload of the times included --, beside a `torch` copy of as many bytes from the same run.  Device
figures: HIP events around the call after 3 warm-up calls, median of `--reps` repetitions with the minimum and
maximum.  `--cpu-atoms` atoms of the same arrays also go through scipy on the host, the reference's path (one process,
as the reference runs it); the first 64 of them are compared with the device's output."""
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

COPY_TB_S = 6.29   # float4 copy on the MI355X: the streaming roof the design document quotes


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


def scipy_reference(y, t, kind):
    from scipy.interpolate import Akima1DInterpolator, PchipInterpolator

    x = np.arange(y.shape[0], dtype=np.float64)
    t0 = time.perf_counter()
    f = PchipInterpolator(x, y, axis=0) if kind == "pchip" else Akima1DInterpolator(x, y, axis=0, method="makima", extrapolate=True)
    out = f(t).astype(np.float32)
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--cpu-atoms", type=int, default=0, help="atoms of the same arrays that also go through scipy on the host (0: skip)")
    ap.add_argument("--shapes", nargs="+", default=["upsampling", "near_unit"])
    a = ap.parse_args()
    A = a.atoms
    shapes = {"upsampling": (200, 20000), "near_unit": (10000, 10000)}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "atoms": A}), flush=True)
    for name in a.shapes:
        n, n_out = shapes[name]
        dense = 100.0 + torch.cumsum(torch.randn(n, A, 3, generator=gen, device="cuda"), dim=0)   # a random walk per column, about 100 A
        words = 3 * (A + 2)
        planes = torch.zeros(n * words + 4, device="cuda", dtype=torch.float32)
        planes[:n * words].view(n, 3, A + 2)[:, :, 1:A + 1] = dense.transpose(1, 2)
        t = np.linspace(0.5, n - 0.5, n_out)
        noise = torch.randn(n_out, A, 3, generator=gen, device="cuda", dtype=torch.float64) * 0.3
        out_dense = torch.empty(n_out * 3 * A, device="cuda", dtype=torch.float32)
        out_planes = torch.empty(n_out * words + 4, device="cuda", dtype=torch.float32)
        res = {"shape": name, "knots": n, "frames": n_out}
        for kind in ("pchip", "makima"):
            for with_noise in (False, True):
                for layout in (("dense", "planes") if kind == "pchip" else ("dense",)):
                    gb = (12.0 * n_out * A + (24.0 * n_out * A if with_noise else 0.0) + 12.0 * n * A * (2 if kind == "makima" else 1)) / 1e9
                    if layout == "dense":
                        fn = lambda: hip.interpolate(dense, A, t, kind=kind, noise=noise if with_noise else None, out=out_dense,
                                                     out_strides=(0, 3 * A, 3, 1))
                    else:
                        fn = lambda: hip.interpolate(planes, A, t, kind=kind, strides=(n, 1, words, 1, A + 2), noise=noise if with_noise else None,
                                                     out=out_planes, out_strides=(1, words, 1, A + 2))
                    r = timed(fn, a.reps)
                    r.update(GB=gb, TB_per_s=gb / r["median_ms"], share_of_copy_rate=gb / r["median_ms"] / COPY_TB_S)
                    res[f"{kind}_{layout}{'_noise' if with_noise else ''}"] = r
        src = torch.empty(int(12.0 * n_out * A / 8), device="cuda", dtype=torch.float32)   # a copy moves its bytes twice: read + write
        dst = torch.empty_like(src)
        res["torch_copy_of_the_output_bytes"] = timed(lambda: dst.copy_(src), a.reps)
        res["torch_copy_of_the_output_bytes"]["TB_per_s"] = 12.0 * n_out * A / 1e9 / res["torch_copy_of_the_output_bytes"]["median_ms"]
        del src, dst
        same = hip.interpolate(planes, A, t, kind="pchip", strides=(n, 1, words, 1, A + 2))
        res["layouts_same_bits"] = bool(torch.equal(same, hip.interpolate(dense, A, t, kind="pchip")))
        del same
        if a.cpu_atoms:
            c = min(a.cpu_atoms, A)
            y = dense[:, :c].cpu().numpy()
            for kind in ("pchip", "makima"):
                ref, seconds = scipy_reference(y, t, kind)
                got = hip.interpolate(dense[:, :c].contiguous(), c, t, kind=kind).cpu().numpy()
                res[f"scipy_{kind}"] = {"atoms": c, "seconds": seconds, "seconds_scaled_to_all_atoms": seconds * A / c,
                                        "max_abs_difference_first_64_atoms": float(np.abs(got[:, :64] - ref[:, :64]).max())}
        print(json.dumps(res), flush=True)
        del dense, planes, noise, out_dense, out_planes


if __name__ == "__main__":
    main()
