"""Import step for GROMACS ``.xtc`` trajectories: the compressed coordinates are decoded on the device (hip.xtc_decode,
csrc/xtc.hip) into the ``.dcd`` or ``.npy`` files every tool of the package maps in place.

An XTC file cannot be mapped: its coordinates are a variable-length bit stream (include/dcv.h has the format), so
``trajectory.open_trajectory`` keeps refusing it.  ``import_trajectory`` builds the frame index on the host
(``trajectory.index_xtc``: one pass over the headers), uploads the compressed bytes of a chunk of frames, decodes them
into a device image of DCD frame records (``DcdWriter.layout()``) or a dense array, downloads the image and appends it.
``route`` is the one helper the tool entries call: ``.xtc`` inputs are imported into ``<output_folder>/xtc_import/`` and
the ``.dcd`` handed on, everything else passes through.  The box, the steps and the times stay in the index: the DCD
writer has no unit-cell block and nothing downstream applies periodic boundaries.

    python -m deep_cartograph_amd.xtc run.xtc [more.xtc ...] -out imported [-format dcd|npy] [-stride 1]"""
from __future__ import annotations

import argparse
import logging
import os
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np

from . import frame_io, trajectory

logger = logging.getLogger(__name__)

NM_TO_ANGSTROM = 10.0   # XTC stores nanometres, the package's coordinates are Angstrom
IMPORT_FOLDER = "xtc_import"


def is_xtc(path) -> bool:
    return os.path.splitext(str(path))[1].lower() == ".xtc"


def import_trajectory(path: str, output_path: str, traj_stride: int = 1, memory_budget: Optional[int] = None) -> str:
    """Decode every ``traj_stride``-th frame of the ``.xtc`` file ``path`` into ``output_path`` (``.dcd`` without unit-cell
    blocks, or ``.npy`` of (n, A, 3) float32), in Angstrom.  Frames go through the device in chunks that hold their
    compressed bytes and their decoded image at once, at most ``memory_budget`` bytes (default: a quarter of free device
    memory, at most 4 GiB); they land under ``<output_path>.partial`` and are renamed at the end.  No CPU fallback."""
    import torch

    from . import hip
    from ._lib import DcvError

    ext = frame_io.coordinate_format(output_path, "an imported trajectory")
    stride = int(traj_stride)
    if stride < 1:
        raise ValueError(f"traj_stride must be at least 1, got {stride}")
    index = trajectory.index_xtc(path)
    if not torch.cuda.is_available():
        raise DcvError("import_trajectories needs an MI355X (cuda) device: XTC frames are decoded by libdcv.so, there is no CPU fallback")
    frames = np.arange(0, index.n_frames, stride, dtype=np.int64)
    n, A = int(frames.size), index.n_atoms
    words = 3 * (A + 2) if ext == ".dcd" else 3 * A
    # a chunk holds the file bytes from its first to its last frame (skipped frames included), its descriptors, status words
    # and decoded image; sized by the mean frame, the longest chunk of a file whose frames differ in size is a little larger
    per_frame = stride * int(np.ceil((index.offset[-1] + index.frame_bytes()[-1] - index.offset[0]) / index.n_frames)) + 48 + 4 + 4 * words
    chunk, ranges = frame_io.plan_chunks(n, per_frame, frame_io.resolve_budget(memory_budget))
    logger.info(f"Importing {n} frames of {A} atoms of {Path(path).name} in chunks of {chunk} frames")
    data = np.memmap(path, dtype=np.uint8, mode="r")
    os.makedirs(os.path.dirname(os.path.abspath(output_path)), exist_ok=True)
    with frame_io.CoordinateSink(output_path, n, A) as sink:
        for lo, hi in ranges:
            first, last, desc = index.span(frames[lo:hi])
            buf = torch.from_numpy(np.array(data[first:last])).cuda()
            image = sink.image(hi - lo)
            try:
                hip.xtc_decode(buf, desc, A, NM_TO_ANGSTROM, out=image, out_strides=sink.layout())
            except DcvError as e:   # a corrupt frame: the sink leaves nothing behind that a restart could take for done
                raise DcvError(f"{path}: frames {int(frames[lo])}..{int(frames[hi - 1])} (every {stride}): {e}") from None
            sink.append(image)
            del buf, image
    return output_path


def import_trajectories(trajectories, output_folder: str, traj_format: str = "dcd", traj_stride: int = 1,
                        memory_budget: Optional[int] = None) -> List[str]:
    """Every ``.xtc`` among ``trajectories`` decoded into ``<output_folder>/<stem>.<traj_format>`` ("dcd" or "npy"); inputs
    that are not ``.xtc`` pass through unchanged.  Returns the paths in the order given.  A trajectory whose output
    exists is skipped.  The output keeps the trajectory's stem: the tools name their folders by it."""
    if traj_format not in ("dcd", "npy"):
        raise ValueError(f"traj_format must be 'dcd' or 'npy', got {traj_format!r} (writing xtc is not supported)")
    trajectories = [trajectories] if isinstance(trajectories, (str, os.PathLike)) else list(trajectories or [])
    out = []
    for path in trajectories:
        path = str(path)
        if not is_xtc(path):
            out.append(path)
            continue
        if not os.path.exists(path):
            raise FileNotFoundError(f"File not found: {path}")
        target = os.path.join(output_folder, f"{Path(path).stem}.{traj_format}")
        if os.path.exists(target):
            logger.info(f"Skipping {Path(path).name}. {target} already exists.")
        else:
            import_trajectory(path, target, traj_stride, memory_budget)
        out.append(target)
    return out


def route(trajectories, output_folder: str, memory_budget: Optional[int] = None):
    """The tool entries' one way in: ``.xtc`` members of ``trajectories`` (a path, a list, or None) are imported into
    ``<output_folder>/xtc_import/`` as ``.dcd`` and replaced by that file; everything else is returned as it came."""
    if trajectories is None:
        return None
    single = isinstance(trajectories, (str, os.PathLike))
    paths = [str(trajectories)] if single else [str(p) for p in trajectories]
    if not any(is_xtc(p) for p in paths):
        return trajectories
    from . import tools   # through the tools entry: one place to replace in a test

    routed = tools.import_trajectories(paths, os.path.join(output_folder, IMPORT_FOLDER), traj_format="dcd", memory_budget=memory_budget)
    return routed[0] if single else routed


def main(argv: Optional[Sequence[str]] = None) -> List[str]:
    p = argparse.ArgumentParser(prog="python -m deep_cartograph_amd.xtc", description="Decode GROMACS .xtc trajectories on the device into .dcd or .npy")
    p.add_argument("trajectories", nargs="+", help=".xtc files (other files pass through)")
    p.add_argument("-out", "-output", dest="out", required=True, help="output folder")
    p.add_argument("-format", dest="format", choices=("dcd", "npy"), default="dcd")
    p.add_argument("-stride", dest="stride", type=int, default=1, help="keep every n-th frame")
    a = p.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    paths = import_trajectories(a.trajectories, a.out, a.format, a.stride)
    for path in paths:
        print(path)
    return paths


if __name__ == "__main__":
    main()
