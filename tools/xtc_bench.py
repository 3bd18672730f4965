"""Timings of hip.xtc_decode and hip.xtc_encode on one GPU (the numbers of DESIGN.md 4.14 and 4.15).

    python tools/xtc_bench.py [--frames 1000000] [--atoms 256] [--distinct 512] [--reps 11] [--tool-frames 0] [--extract-frames 0]

`--distinct` frames of `--atoms` atoms are made with the structural encoder of tests/xtc_oracle.py (runs of 0 to 8 small
atoms in a random order, smallidx between 20 and 30, precision 1000: a legal stream, not GROMACS's own choice of runs)
and replicated on the device to `--frames` frames.  Reported for a dense (n, A, 3) output and for the planes of a DCD
record image: the time of the whole call (descriptor upload and the one kernel) by HIP events after 2 warm-up calls, as
the median of `--reps` repetitions with the minimum and maximum; frames/s; compressed GB/s in and decoded GB/s out (12
bytes per atom and frame); and the time of a `torch` copy of the output bytes in the same run, the bound the stores
cannot beat.  The first 64 frames of the output are compared with the CPU oracle.  `--tool-frames N` also times
tools.import_trajectories end to end (index, upload, decode, download, file write; wall clock) on an .xtc file of N
frames written to a temporary folder.

The encode section runs in the same process on the frames the decoder has just produced (dense rows and the planes of a
DCD record image): the encode kernel alone (dcv_xtc_encode without frame indices: one launch and nothing else), the whole
call of hip.xtc_encode (encode, descriptor download, prefix sum on the host, pack), the output bits per atom, and the
ratios to the `torch` copy of the input bytes and to hip.xtc_decode of the same frames.  The first 64 frames of the image
are compared with the CPU oracle (tests/xtc_encode_oracle.py).  `--extract-frames N` also times
trajectory.extract_frames end to end (every second frame of a .dcd of N frames; upload, encode, download, file write;
wall clock)."""
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

from deep_cartograph_amd import _lib, hip  # noqa: E402
from tests import xtc_encode_oracle as eo  # noqa: E402
from tests import xtc_oracle as xo  # noqa: E402


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


def make_frames(distinct, atoms, seed=0):
    """(bytes of `distinct` frames, their descriptors as tests/xtc_oracle.frames gives them)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    data = []
    for f in range(distinct):
        script, left = [], atoms
        while left:
            r = int(rng.integers(0, min(8, left - 1), endpoint=True))
            script.append((r, 0, False))
            left -= 1 + r
        smallidx = int(rng.integers(20, 31))
        centre = rng.integers(1000, 6000, size=3)
        ints = xo.make_ints(rng, script, smallidx, centre - 4000, centre + 4000)
        data.append(xo.encode_frame(ints, script, smallidx, 1000.0, step=f, time=float(f)))
    data = b"".join(data)
    return data, xo.frames(data)


def descriptors(frames, copies, block_bytes):
    one = np.zeros(len(frames), dtype=_lib.XTC_FRAME_DTYPE)
    for i, f in enumerate(frames):
        one[i] = (f["offset"], f["nbytes"], f["smallidx"], f["precision"], 0, f["minint"], f["maxint"])
    desc = np.tile(one, copies)
    desc["offset"] += np.repeat(np.arange(copies, dtype=np.int64) * block_bytes, len(frames))
    return desc


def device_cases(a, out):
    block, frames = make_frames(a.distinct, a.atoms)
    copies = max(1, a.frames // a.distinct)
    n, A = copies * a.distinct, a.atoms
    desc = descriptors(frames, copies, len(block))
    data = torch.from_numpy(np.frombuffer(block, dtype=np.uint8).copy()).cuda().repeat(copies)
    payload = float(sum((f["nbytes"] + 3) // 4 * 4 for f in frames)) * copies
    out["shape"] = {"frames": n, "atoms": A, "distinct_frames": a.distinct, "file_GB": data.numel() / 1e9, "payload_GB": payload / 1e9,
                    "decoded_GB": 12.0 * n * A / 1e9, "payload_bits_per_atom": 8 * payload / (n * A)}
    src = torch.empty(3 * n * A, device="cuda", dtype=torch.float32)
    dst = torch.empty_like(src)
    out["torch_copy_of_output"] = timed(lambda: dst.copy_(src), a.reps)
    del src, dst
    words = 3 * (A + 2)
    want = xo.decode(block)[1][:64]
    for name, size, strides in (("dense", 3 * n * A, (0, 3 * A, 3, 1)), ("dcd_planes", n * words, (1, words, 1, A + 2))):
        target = torch.zeros(size, device="cuda", dtype=torch.float32)
        status = hip.xtc_decode(data, desc, A, out=target, out_strides=strides, return_status=True)[1]
        r = timed(lambda: hip.xtc_decode(data, desc, A, out=target, out_strides=strides, return_status=True), a.reps)
        r["frames_per_s"] = n / (r["median_ms"] * 1e-3)
        r["compressed_GB_per_s_in"] = payload / 1e9 / (r["median_ms"] * 1e-3)
        r["decoded_GB_per_s_out"] = 12.0 * n * A / 1e9 / (r["median_ms"] * 1e-3)
        r["times_the_copy"] = r["median_ms"] / out["torch_copy_of_output"]["median_ms"]
        r["all_frames_decoded"] = not bool(status.any())
        head = target[:64 * 3 * A].view(64, A, 3) if name == "dense" else target[:64 * words].view(64, 3, A + 2)[:, :, 1:A + 1].transpose(1, 2)
        r["first_frames_equal_oracle"] = bool(np.array_equal(head.cpu().numpy(), want[:64]))
        out[f"decode_{name}"] = r
        print(json.dumps({f"decode_{name}": r}), flush=True)
        encode_case(a, out, name, target, (n, *strides), n, A, want)
        del target
    return block


def encode_case(a, out, name, xyz, layout, n, A, want):
    """The frames the decoder left in `xyz` (layout: n, offset, frame, atom, comp) encoded again."""
    lib = _lib.load()
    slot = lib.dcv_xtc_encode_slot_bytes(A)
    slots = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
    desc = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    _, off, fs, as_, cs = layout
    stream = torch.cuda.current_stream().cuda_stream

    def kernel():
        rc = lib.dcv_xtc_encode(xyz.data_ptr() + 4 * off, n, fs, as_, cs, A, None, n, 0.1, 1000.0, slots.data_ptr(), slots.numel(), desc.data_ptr(),
                                status.data_ptr(), None, 0, stream)
        assert rc == 0, lib.dcv_last_error()

    k = timed(kernel, a.reps)
    nbytes = desc.cpu().numpy().view(_lib.XTC_FRAME_DTYPE)["nbytes"].astype(np.int64)
    k["all_frames_encoded"] = not bool(status.any())
    k["payload_GB"] = float(nbytes.sum()) / 1e9
    k["payload_bits_per_atom"] = 8.0 * float(nbytes.sum()) / (n * A)
    del slots, desc, status
    image = hip.xtc_encode(xyz, A, strides=layout)
    w = timed(lambda: hip.xtc_encode(xyz, A, strides=layout), a.reps)
    head = eo.encode(want, 1000.0)
    head = eo.file_image(head[0], head[2], A)
    w["first_frames_equal_oracle"] = image[:len(head)].cpu().numpy().tobytes() == head
    w["image_GB"] = image.numel() / 1e9
    for r in (k, w):
        r["frames_per_s"] = n / (r["median_ms"] * 1e-3)
        r["input_GB_per_s"] = 12.0 * n * A / 1e9 / (r["median_ms"] * 1e-3)
        r["times_the_copy"] = r["median_ms"] / out["torch_copy_of_output"]["median_ms"]
        r["times_the_decoder"] = r["median_ms"] / out[f"decode_{name}"]["median_ms"]
    out[f"encode_kernel_{name}"], out[f"encode_call_{name}"] = k, w
    print(json.dumps({f"encode_kernel_{name}": k, f"encode_call_{name}": w}), flush=True)


def whole_extract(n, block, distinct, out):
    """trajectory.extract_frames on a .dcd of n frames (the decoded block repeated), every second frame."""
    from deep_cartograph_amd import trajectory as tr

    xyz = xo.decode(block)[1]
    A = xyz.shape[1]
    with tempfile.TemporaryDirectory() as d:
        dcd, pdb = os.path.join(d, "run.dcd"), os.path.join(d, "run.pdb")
        top = tr.Topology(["CA"] * A, ["ALA"] * A, ["A"] * A, ["A"] * A, np.arange(1, A + 1), xyz[0], None)
        tr.write_topology(pdb, top)
        with tr.write_dcd(dcd, A) as w:
            img = w.image(len(xyz))
            o, fs, _, cs = w.layout()
            for c in range(3):
                img.reshape(-1, fs)[:, o + c * cs:o + c * cs + A] = xyz[:, :, c]
            for _ in range(max(1, n // distinct)):
                w.append(img)
            total = w.n_frames
        t0 = time.perf_counter()
        path = tr.extract_frames(dcd, pdb, np.arange(0, total, 2), os.path.join(d, "half.xtc"))
        torch.cuda.synchronize()
        out["extract_frames"] = {"source_frames": total, "frames": (total + 1) // 2, "wall_s": time.perf_counter() - t0, "dcd_bytes": os.path.getsize(dcd),
                                 "xtc_bytes": os.path.getsize(path)}


def whole_tool(n, block, distinct, out):
    from deep_cartograph_amd import tools

    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "run.xtc")
        with open(path, "wb") as f:
            for _ in range(max(1, n // distinct)):
                f.write(block)
        t0 = time.perf_counter()
        paths = tools.import_trajectories([path], os.path.join(d, "imported"))
        torch.cuda.synchronize()
        out["import_trajectories"] = {"frames": max(1, n // distinct) * distinct, "wall_s": time.perf_counter() - t0, "xtc_bytes": os.path.getsize(path),
                                      "dcd_bytes": os.path.getsize(paths[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--atoms", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=512)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--tool-frames", type=int, default=0, help="frames of the end-to-end run of tools.import_trajectories (0: skip)")
    ap.add_argument("--extract-frames", type=int, default=0, help="source frames of the end-to-end run of trajectory.extract_frames (0: skip)")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    block = device_cases(a, out)
    if a.tool_frames:
        whole_tool(a.tool_frames, block, a.distinct, out)
    if a.extract_frames:
        whole_extract(a.extract_frames, block, a.distinct, out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
