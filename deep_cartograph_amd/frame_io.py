"""How the trajectory tools move coordinates through the device in chunks: the memory budget, the chunk
plan, the frame stream (`Trajectory.span` slices uploaded as they lie in the file) and the coordinate sink (`.dcd` /
`.npy` output under a temporary name).  A leaf module: it imports `trajectory` and nothing else from the package.  A
chunk is a range [lo, hi) of the frames a tool visits; the tool owns the device bytes one such frame takes."""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import numpy as np

from . import trajectory

# every chunk also exists once as a pageable host copy on its way up or down, so the default budget is capped for the host's sake
DEFAULT_CHUNK_BYTES = 4 << 30


def resolve_budget(memory_budget: Optional[int]) -> int:
    """The device bytes a chunk may take: `memory_budget` when given, else a quarter of what is free, capped."""
    if memory_budget is not None:
        return memory_budget
    import torch

    return min(torch.cuda.mem_get_info()[0] // 4, DEFAULT_CHUNK_BYTES)


def plan_chunks(n: int, per_frame_bytes: int, budget: int) -> Tuple[int, List[Tuple[int, int]]]:
    """(chunk length, [lo, hi) ranges) for `n` frames of `per_frame_bytes` within `budget`; at least one frame a chunk."""
    chunk = int(max(1, min(n, budget // per_frame_bytes)))
    return chunk, [(lo, min(n, lo + chunk)) for lo in range(0, n, chunk)]


def spans(traj: trajectory.Trajectory, ranges: List[Tuple[int, int]], stride: int = 1):
    """(lo, hi, slice of the mapped file, layout inside the slice) of frames lo * stride, ..., (hi - 1) * stride for every
    range: the host half of the stream."""
    for lo, hi in ranges:
        yield (lo, hi) + traj.span(lo * stride, (hi - 1) * stride + 1, stride)


def upload(span: np.ndarray):
    """A slice of a mapped trajectory as a device tensor: one pageable host copy, one transfer."""
    import torch

    return torch.from_numpy(np.array(span, dtype=np.float32)).cuda()


def stream(traj: trajectory.Trajectory, ranges: List[Tuple[int, int]], stride: int = 1):
    """(lo, hi, device buffer, layout) for every range.  The stream drops its reference to a buffer before it uploads the
    next; a consumer that does the same (`del buf`) has one chunk on the device at a time."""
    for lo, hi, span, layout in spans(traj, ranges, stride):
        buf = upload(span)
        yield lo, hi, buf, layout
        del buf


def coordinate_format(path: str, what: str) -> str:
    """".dcd" or ".npy", the extension of `path`; anything else is refused in the caller's words (`what` is written)."""
    ext = os.path.splitext(path)[1].lower()
    if ext not in (".dcd", ".npy"):
        raise ValueError(f"{path}: {what} is written as .dcd or .npy")
    return ext


class CoordinateSink:
    """Chunked output of `n_frames` frames of `n_atoms` atoms as `path`: a `.dcd` without unit-cell blocks
    (trajectory.DcdWriter) or a `.npy` of (n, A, 3) float32.  A chunk of k frames is one 1-D float32 *image* of
    ``k * frame_words`` words (`image`); a kernel writes the coordinates into it through ``out_strides = layout()`` -- the
    planes of DCD frame records, or dense rows -- and `append` downloads it and adds it to the file (the DCD record
    markers are stamped on the host).  The frames land under ``<path>.partial``: a clean exit renames that file to `path`,
    an exception removes it, so an interrupted run leaves nothing a restart could take for done."""

    def __init__(self, path: str, n_frames: int, n_atoms: int, what: str = "the trajectory"):
        self.path, self.partial_path, self.n_atoms, self.n_written = path, path + ".partial", int(n_atoms), 0
        self._writer = self._rows = None
        if coordinate_format(path, what) == ".dcd":
            self._writer = trajectory.write_dcd(self.partial_path, self.n_atoms)
            self.frame_words = self._writer.frame_words
        else:
            self._rows = np.lib.format.open_memmap(self.partial_path, mode="w+", dtype=np.float32, shape=(int(n_frames), self.n_atoms, 3))
            self.frame_words = 3 * self.n_atoms

    def layout(self) -> Tuple[int, int, int, int]:
        """(offset, frame_stride, atom_stride, comp_stride) of the coordinates inside an image, in elements."""
        return self._writer.layout() if self._writer else (0, 3 * self.n_atoms, 3, 1)

    def image(self, k: int, device="cuda"):
        """An uninitialised image of `k` frames: every word is a coordinate the kernel writes or a marker `append` stamps."""
        import torch

        return torch.empty(k * self.frame_words, dtype=torch.float32, device=device)

    def append(self, image) -> None:
        image = image.cpu().numpy()
        k = image.size // self.frame_words
        if self._writer:
            self._writer.append(image)
        else:
            self._rows[self.n_written:self.n_written + k] = image.reshape(k, self.n_atoms, 3)
        self.n_written += k

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if self._writer:
            self._writer.__exit__(exc_type, exc, tb)
        elif exc_type is None:
            self._rows.flush()
        self._rows = None
        if exc_type is None:
            os.replace(self.partial_path, self.path)
        else:
            os.remove(self.partial_path)
        return False
