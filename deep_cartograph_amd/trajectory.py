"""Host side of compute_features, analyze_geometry and traj_augmentation: topology, atom selections, trajectory files
(read and written) and the feature definitions the device kernel (hip.featurize) evaluates.  NumPy only -- no
MDAnalysis, no PLUMED.

What the reference does with MDAnalysis and a `plumed driver` subprocess (tools/compute_features/compute_features.py,
modules/md/md.py) is restated for the feature kinds its own test data pins:

* ``read_topology``        PDB ATOM / HETATM / CONECT records up to the first ENDMDL;
* ``select_atoms``         a documented subset of the MDAnalysis selection grammar (below);
* ``open_trajectory``      little-endian CHARMM / NAMD ``.dcd`` (memory-mapped, never transposed) and ``.npy``;
* ``index_xtc``            the frame index of a GROMACS ``.xtc`` (headers only; the payloads are decoded on the device by
                           hip.xtc_decode, xtc.py has the import step);
* ``write_dcd``, ``write_topology``  the way back out (traj_augmentation): a chunked DCD writer whose record images a
                           kernel fills in place, and a PDB of a selection with its CONECT records;
* ``write_xtc``, ``extract_frames``  chosen frames of a trajectory written as a GROMACS ``.xtc`` (traj_cluster's cluster
                           ensembles): the frames are compressed on the device (hip.xtc_encode), the writer appends
                           finished file images;
* ``feature_definitions``  names and kernel records of the distance and virtual-dihedral groups, with the
                           reference's labelling rules and order (md.py:26-129, 226-273, 479-545, 580-717).

Selection grammar: ``all``; ``name``, ``resname``, ``segid`` / ``chainID`` followed by one or more values, each
optionally ending in the wildcard ``*``; ``resid`` followed by values ``7``, ``3:9`` or ``3-9`` (inclusive);
``not``, ``and``, ``or`` (binding in that order) and parentheses.  Anything else -- ``protein``, ``backbone``,
``around``, ``index``, ``?`` wildcards ... -- raises ValueError naming the token.  A selection is returned in
topology order, as MDAnalysis returns it.  ``segid`` is the PDB segment identifier (columns 73-76) and falls back to
the chain identifier where that field is blank, as in MDAnalysis.

Out of scope (ValueError naming the option): ``coordinate_groups`` (need a per-frame optimal fit),
``distance_to_center_groups``, and the ``protein_backbone`` / ``real`` dihedral search modes.  Periodic boundaries
are not applied: the reference's distances are NOPBC and its torsions follow a WHOLEMOLECULES step, so a trajectory
whose molecule is split across the box must be made whole first.  XTC is not mapped but imported (xtc.py)."""
from __future__ import annotations

import logging
import math
import os
import re
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Set, Tuple

import numpy as np

from ._lib import FEAT_DISTANCE, FEAT_TORSION, FEAT_TORSION_SINCOS, XTC_FRAME_DTYPE

logger = logging.getLogger(__name__)

COVALENT_BOND_THRESHOLD = 2.0   # Angstrom: the reference's guess for a bond when the topology has no CONECT records


# ------------------------------------------------------------------------------------------------ topology
@dataclass
class Topology:
    names: List[str]
    resnames: List[str]
    chains: List[str]
    segids: List[str]
    resids: np.ndarray            # int64 [A]
    positions: np.ndarray         # float32 [A, 3], Angstrom
    bonds: Optional[Set[Tuple[int, int]]]   # pairs (i < j) of 0-based atom indices from CONECT; None without CONECT records

    @property
    def n_atoms(self) -> int:
        return len(self.names)


def read_topology(path: str) -> Topology:
    """Atoms (and CONECT bonds, if any) of the first model of a PDB file."""
    names, resnames, chains, segids, resids, pos, serials = [], [], [], [], [], [], []
    conect: List[Tuple[int, int]] = []
    in_first_model = True
    with open(path) as f:
        for line in f:
            rec = line[:6].strip()
            if rec == "ENDMDL":
                in_first_model = False
            elif rec in ("ATOM", "HETATM") and in_first_model:
                try:
                    serials.append(int(line[6:11]))
                except ValueError:
                    serials.append(len(serials) + 1)   # overflowed serial columns
                names.append(line[12:16].strip())
                resnames.append(line[17:21].strip())
                chains.append(line[21:22].strip())
                segids.append(line[72:76].strip() or chains[-1])
                resids.append(int(line[22:26]))
                pos.append((float(line[30:38]), float(line[38:46]), float(line[46:54])))
            elif rec == "CONECT":
                fields = [line[i:i + 5] for i in range(6, min(len(line.rstrip("\n")), 31), 5)]
                nums = [int(x) for x in fields if x.strip()]
                conect.extend((nums[0], other) for other in nums[1:])   # a record without partners (or empty) yields no pair
    if not names:
        raise ValueError(f"{path}: no ATOM or HETATM records")
    bonds = None
    if conect:
        index = {s: i for i, s in enumerate(serials)}
        bonds = set()
        for a, b in conect:
            if a in index and b in index and index[a] != index[b]:
                i, j = index[a], index[b]
                bonds.add((min(i, j), max(i, j)))
    return Topology(names, resnames, chains, segids, np.asarray(resids, dtype=np.int64),
                    np.asarray(pos, dtype=np.float32).reshape(-1, 3), bonds)


# ------------------------------------------------------------------------------------------------ selections
_RESERVED = {"and", "or", "not", "(", ")"}
_STRING_KEYWORDS = {"name": "names", "resname": "resnames", "segid": "segids", "chainID": "chains", "chainid": "chains"}
_RESID_VALUE = re.compile(r"^(-?\d+)(?:[:-](-?\d+))?$")


def _match_strings(values: List[str], patterns: List[str]) -> np.ndarray:
    mask = np.zeros(len(values), dtype=bool)
    for p in patterns:
        stem = p[:-1] if p.endswith("*") else p
        if not stem and not p.endswith("*") or any(ch in stem for ch in "*?[]"):
            raise ValueError(f"unsupported selection token '{p}': only a trailing '*' wildcard is understood")
        if p.endswith("*"):
            mask |= np.fromiter((v.startswith(stem) for v in values), dtype=bool, count=len(values))
        else:
            mask |= np.fromiter((v == stem for v in values), dtype=bool, count=len(values))
    return mask


class _Parser:
    def __init__(self, top: Topology, selection: str):
        self.top = top
        self.tokens = selection.replace("(", " ( ").replace(")", " ) ").split()
        self.pos = 0
        if not self.tokens:
            raise ValueError("empty selection")

    def peek(self) -> Optional[str]:
        return self.tokens[self.pos] if self.pos < len(self.tokens) else None

    def take(self) -> str:
        tok = self.tokens[self.pos]
        self.pos += 1
        return tok

    def values(self, keyword: str) -> List[str]:
        vals = []
        while self.peek() is not None and self.peek() not in _RESERVED:
            vals.append(self.take())
        if not vals:
            raise ValueError(f"selection keyword '{keyword}' needs at least one value")
        return vals

    def parse(self) -> np.ndarray:
        mask = self.or_expr()
        if self.peek() is not None:
            raise ValueError(f"unsupported selection token '{self.peek()}'")
        return mask

    def or_expr(self) -> np.ndarray:
        mask = self.and_expr()
        while self.peek() == "or":
            self.take()
            mask = mask | self.and_expr()
        return mask

    def and_expr(self) -> np.ndarray:
        mask = self.not_expr()
        while self.peek() == "and":
            self.take()
            mask = mask & self.not_expr()
        return mask

    def not_expr(self) -> np.ndarray:
        if self.peek() == "not":
            self.take()
            return ~self.not_expr()
        return self.primary()

    def primary(self) -> np.ndarray:
        if self.peek() is None:
            raise ValueError("selection ends where a term was expected")
        tok = self.take()
        if tok == "(":
            mask = self.or_expr()
            if self.peek() != ")":
                raise ValueError("unbalanced parenthesis in selection")
            self.take()
            return mask
        if tok == "all":
            return np.ones(self.top.n_atoms, dtype=bool)
        if tok in _STRING_KEYWORDS:
            return _match_strings(getattr(self.top, _STRING_KEYWORDS[tok]), self.values(tok))
        if tok == "resid":
            mask = np.zeros(self.top.n_atoms, dtype=bool)
            for v in self.values(tok):
                m = _RESID_VALUE.match(v)
                if not m:
                    raise ValueError(f"unsupported selection token '{v}' after resid")
                lo = int(m.group(1))
                hi = int(m.group(2)) if m.group(2) is not None else lo
                mask |= (self.top.resids >= lo) & (self.top.resids <= hi)
            return mask
        raise ValueError(f"unsupported selection token '{tok}'")


def select_atoms(top: Topology, selection: str) -> np.ndarray:
    """0-based indices (ascending) of the atoms a selection string names."""
    return np.flatnonzero(_Parser(top, selection).parse())


# ------------------------------------------------------------------------------------------------ trajectories
@dataclass
class Trajectory:
    """A trajectory as one flat float32 buffer (memory-mapped) plus the addressing the kernel needs: coordinate c of
    atom a of frame f is ``data[offset + f*frame_stride + a*atom_stride + c*comp_stride]`` (Angstrom)."""
    data: np.ndarray
    n_frames: int
    n_atoms: int
    offset: int
    frame_stride: int
    atom_stride: int
    comp_stride: int

    def layout(self, start: int = 0, stop: Optional[int] = None, step: int = 1) -> Tuple[int, int, int, int, int]:
        """(n, offset, frame_stride, atom_stride, comp_stride) of frames [start:stop:step] -- the `strides` argument of
        hip.featurize for the whole buffer."""
        stop = self.n_frames if stop is None else min(stop, self.n_frames)
        n = max(0, (stop - start + step - 1) // step)
        return n, self.offset + start * self.frame_stride, step * self.frame_stride, self.atom_stride, self.comp_stride

    def span(self, start: int, stop: int, step: int = 1) -> Tuple[np.ndarray, Tuple[int, int, int, int, int]]:
        """The smallest slice of the buffer that holds frames [start:stop:step], and their layout inside that slice: what
        one chunk uploads.  16-byte alignment of the file is kept (the slice starts on a multiple of 4 elements)."""
        n, off, fs, as_, cs = self.layout(start, stop, step)
        if n == 0:
            return self.data[:0], (0, 0, fs, as_, cs)
        first = off // 4 * 4
        last = off + (n - 1) * fs + (self.n_atoms - 1) * as_ + 2 * cs
        return self.data[first:last + 1], (n, off - first, fs, as_, cs)

    def frames(self, start: int = 0, stop: Optional[int] = None, step: int = 1) -> np.ndarray:
        """(n, A, 3) float32 copy of frames [start:stop:step] (for host-side checks; the device path never needs it)."""
        n, off, fs, as_, cs = self.layout(start, stop, step)
        idx = (off + fs * np.arange(n, dtype=np.int64)[:, None, None] + as_ * np.arange(self.n_atoms, dtype=np.int64)[None, :, None]
               + cs * np.arange(3, dtype=np.int64)[None, None, :])
        return np.asarray(self.data[idx], dtype=np.float32)


def _open_dcd(path: str, n_atoms: Optional[int]) -> Trajectory:
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(92)
        if len(head) < 92 or head[4:8] != b"CORD":
            raise ValueError(f"{path}: not a DCD file (no CORD header)")
        if np.frombuffer(head, dtype="<i4", count=1)[0] != 84:
            if np.frombuffer(head, dtype=">i4", count=1)[0] == 84:
                raise ValueError(f"{path}: big-endian DCD files are not supported (the file is mapped as little-endian float32)")
            raise ValueError(f"{path}: not a DCD file (header record of {np.frombuffer(head, dtype='<i4', count=1)[0]} bytes)")
        icntrl = np.frombuffer(head, dtype="<i4", count=20, offset=8)
        nset, fixed, charmm = int(icntrl[0]), int(icntrl[8]), int(icntrl[19]) != 0
        has_cell = charmm and int(icntrl[10]) != 0
        if fixed != 0:
            raise ValueError(f"{path}: DCD with {fixed} fixed atoms: frames after the first hold only the free atoms, not supported")
        if charmm and int(icntrl[11]) != 0:
            raise ValueError(f"{path}: DCD with the 4th-dimension flag set is not supported")
        rec = np.frombuffer(f.read(8), dtype="<i4", count=2)
        title_bytes, ntitle = int(rec[0]), int(rec[1])
        if title_bytes < 4 or (title_bytes - 4) % 80 != 0 or ntitle < 0:
            raise ValueError(f"{path}: malformed DCD title block ({title_bytes} bytes, {ntitle} lines)")
        f.seek(title_bytes - 4 + 4, os.SEEK_CUR)   # the title lines and the closing marker
        rec = np.frombuffer(f.read(12), dtype="<i4", count=3)
        if rec.size != 3 or rec[0] != 4 or rec[2] != 4:
            raise ValueError(f"{path}: malformed DCD atom-count block")
        natom = int(rec[1])
        header_bytes = f.tell()
    if n_atoms is not None and natom != n_atoms:
        raise ValueError(f"{path}: {natom} atoms in the trajectory, {n_atoms} in the topology")
    cell_words = 14 if has_cell else 0          # marker + 6 float64 + marker
    frame_words = cell_words + 3 * (natom + 2)
    if header_bytes + nset * frame_words * 4 != size:
        raise ValueError(f"{path}: {size} bytes do not match the header's {nset} frames of {natom} atoms "
                         f"({header_bytes} + {nset} x {frame_words * 4} bytes): truncated or unfinished file")
    data = np.memmap(path, dtype="<f4", mode="r") if size else np.zeros(0, dtype=np.float32)
    return Trajectory(data, nset, natom, header_bytes // 4 + cell_words + 1, frame_words, 1, natom + 2)


def open_trajectory(path: str, n_atoms: Optional[int] = None) -> Trajectory:
    """Memory-map a trajectory: ``.dcd`` (little-endian CHARMM / NAMD / X-PLOR, with or without the unit-cell block) or
    ``.npy`` holding (n, A, 3) float32 in Angstrom.  ``n_atoms`` (the topology's) is checked when given.  A GROMACS
    ``.xtc`` is refused: its coordinates are a variable-length bit stream, which cannot be mapped; ``index_xtc`` finds its
    frames and tools.import_trajectories decodes them on the device into a ``.dcd`` or ``.npy`` this function maps (the
    tool entries do that themselves for ``.xtc`` inputs)."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".dcd":
        return _open_dcd(path, n_atoms)
    if ext == ".npy":
        arr = np.load(path, mmap_mode="r")
        if arr.ndim != 3 or arr.shape[2] != 3 or arr.dtype != np.float32:
            raise ValueError(f"{path}: expected a (frames, atoms, 3) float32 array, got {arr.shape} {arr.dtype}")
        if n_atoms is not None and arr.shape[1] != n_atoms:
            raise ValueError(f"{path}: {arr.shape[1]} atoms in the trajectory, {n_atoms} in the topology")
        return Trajectory(arr.reshape(-1), arr.shape[0], arr.shape[1], 0, 3 * arr.shape[1], 3, 1)
    raise ValueError(f"{path}: unsupported trajectory format '{ext}' (supported: .dcd, .npy; XTC is a compressed bit stream that cannot be "
                     "mapped in place: decode it first with tools.import_trajectories, as the tools do for their .xtc inputs)")


# ------------------------------------------------------------------------------------------------ XTC frame index
XTC_MAGIC, XTC_MAGIC_64 = 1995, 2023
XTC_FIRSTIDX, XTC_LASTIDX = 9, 72
_XTC_HEADER = struct.Struct(">iiif9fi")      # magic, natoms, step, time, box, natoms
_XTC_COMPRESSED = struct.Struct(">f3i3iii")  # precision, minint, maxint, smallidx, nbytes


@dataclass
class XtcIndex:
    """Where the frames of a GROMACS ``.xtc`` file lie and what their headers say (``index_xtc``).  Per frame (arrays of
    ``n_frames``): ``offset`` -- the byte offset of the compressed payload, or of the float32 coordinates of a *raw* frame
    (``raw``: a file of at most 9 atoms stores them uncompressed) --, ``nbytes`` of payload (0 for raw frames),
    ``precision``, ``minint`` / ``maxint`` [n, 3], ``smallidx``, ``step``, ``time`` (ps) and ``box`` [n, 3, 3] (nm).  The box,
    the steps and the times are kept here only: nothing downstream applies periodic boundaries."""
    path: str
    n_frames: int
    n_atoms: int
    raw: bool
    offset: np.ndarray
    nbytes: np.ndarray
    precision: np.ndarray
    minint: np.ndarray
    maxint: np.ndarray
    smallidx: np.ndarray
    step: np.ndarray
    time: np.ndarray
    box: np.ndarray

    def frame_bytes(self) -> np.ndarray:
        """Bytes each frame's coordinates take in the file (payload padded to 4; 12 per atom for raw frames)."""
        return np.full(self.n_frames, 12 * self.n_atoms, dtype=np.int64) if self.raw else (self.nbytes.astype(np.int64) + 3) // 4 * 4

    def span(self, frames) -> Tuple[int, int, np.ndarray]:
        """(first byte, end byte, descriptors) of the frames ``frames`` (ascending indices): the smallest slice of the file
        that holds them -- it starts on the 4-byte grid, as every field of the file does -- and their XTC_FRAME_DTYPE
        descriptors with offsets relative to that slice: what one chunk uploads and hands to hip.xtc_decode."""
        frames = np.asarray(frames, dtype=np.int64).reshape(-1)
        desc = np.zeros(frames.size, dtype=XTC_FRAME_DTYPE)
        if frames.size == 0:
            return 0, 0, desc
        first = int(self.offset[frames[0]])
        last = int(self.offset[frames[-1]] + self.frame_bytes()[frames[-1]])
        desc["offset"] = self.offset[frames] - first
        desc["nbytes"], desc["smallidx"], desc["precision"] = self.nbytes[frames], self.smallidx[frames], self.precision[frames]
        desc["raw"] = int(self.raw)
        desc["minint"], desc["maxint"] = self.minint[frames], self.maxint[frames]
        return first, last, desc


def index_xtc(path: str, n_atoms: Optional[int] = None) -> XtcIndex:
    """One pass over the frame headers of a GROMACS ``.xtc`` file (memory-mapped; the payloads are not read).  Every
    integer and float of the file is big-endian; a frame is
    ``int32 magic (1995), natoms, step; float32 time, box[9]; int32 natoms``, then for at most 9 atoms ``3 natoms`` float32
    (nm) and nothing else, otherwise ``float32 precision; int32 minint[3], maxint[3], smallidx, nbytes`` and ``nbytes`` of
    payload padded with zeros to a multiple of 4 (include/dcv.h has the payload).  Raises ValueError naming the file and
    the frame for: magic 2023 (the variant with 64-bit byte counts, not read), any other magic, an atom count that
    changes between frames or differs from ``n_atoms``, a header or payload that runs past the end of the file,
    ``smallidx`` outside [9, 72], ``maxint < minint`` and a precision that is not finite and positive."""
    size = os.path.getsize(path)
    data = np.memmap(path, dtype=np.uint8, mode="r") if size else np.zeros(0, dtype=np.uint8)
    cols: Dict[str, list] = {k: [] for k in ("offset", "nbytes", "precision", "minint", "maxint", "smallidx", "step", "time", "box")}
    pos, frame, natoms = 0, 0, None
    while pos < size:
        where = f"{path}: frame {frame}"
        if pos + 56 > size:
            raise ValueError(f"{where}: the header at byte {pos} runs past the end of the file ({size} bytes): truncated file")
        magic, n, step, time, *box, n2 = _XTC_HEADER.unpack_from(data, pos)
        if magic == XTC_MAGIC_64:
            raise ValueError(f"{where}: magic 2023, the XTC variant with 64-bit byte counts, is not supported (only magic 1995)")
        if magic != XTC_MAGIC:
            raise ValueError(f"{where}: magic {magic} at byte {pos}, not an XTC frame (expected 1995)")
        if n != n2 or n < 1:
            raise ValueError(f"{where}: inconsistent atom counts in the header ({n} and {n2})")
        if natoms is None:
            if n_atoms is not None and n != n_atoms:
                raise ValueError(f"{where}: {n} atoms in the trajectory, {n_atoms} in the topology")
            natoms = n
        elif n != natoms:
            raise ValueError(f"{where}: {n} atoms, the frames before it have {natoms}: the atom count changes")
        cols["step"].append(step)
        cols["time"].append(time)
        cols["box"].append(box)
        pos += 56
        if natoms <= 9:
            length = 12 * natoms
            fields = (0, 0.0, (0, 0, 0), (0, 0, 0), 0)
        else:
            if pos + 36 > size:
                raise ValueError(f"{where}: the header at byte {pos - 56} runs past the end of the file ({size} bytes): truncated file")
            precision, *ints = _XTC_COMPRESSED.unpack_from(data, pos)
            minint, maxint, smallidx, nbytes = ints[0:3], ints[3:6], ints[6], ints[7]
            if not (math.isfinite(precision) and precision > 0):
                raise ValueError(f"{where}: precision {precision} is not finite and positive")
            if any(hi < lo for lo, hi in zip(minint, maxint)):
                raise ValueError(f"{where}: maxint {maxint} below minint {minint}")
            if not XTC_FIRSTIDX <= smallidx <= XTC_LASTIDX:
                raise ValueError(f"{where}: smallidx {smallidx} outside [{XTC_FIRSTIDX}, {XTC_LASTIDX}]")
            if nbytes < 0:
                raise ValueError(f"{where}: a payload of {nbytes} bytes")
            pos += 36
            length = (nbytes + 3) // 4 * 4
            fields = (nbytes, precision, minint, maxint, smallidx)
        if pos + length > size:
            raise ValueError(f"{where}: {length} bytes of coordinates at byte {pos} run past the end of the file ({size} bytes): truncated file")
        cols["offset"].append(pos)
        for key, v in zip(("nbytes", "precision", "minint", "maxint", "smallidx"), fields):
            cols[key].append(v)
        pos += length
        frame += 1
    if frame == 0:
        raise ValueError(f"{path}: frame 0: the file is empty")
    return XtcIndex(path, frame, natoms, natoms <= 9, np.asarray(cols["offset"], dtype=np.int64), np.asarray(cols["nbytes"], dtype=np.int32),
                    np.asarray(cols["precision"], dtype=np.float32), np.asarray(cols["minint"], dtype=np.int32).reshape(-1, 3),
                    np.asarray(cols["maxint"], dtype=np.int32).reshape(-1, 3), np.asarray(cols["smallidx"], dtype=np.int32),
                    np.asarray(cols["step"], dtype=np.int64), np.asarray(cols["time"], dtype=np.float32),
                    np.asarray(cols["box"], dtype=np.float32).reshape(-1, 3, 3))


# ------------------------------------------------------------------------------------------------ writers
_DCD_TITLE = b"Written by deep_cartograph_amd"


class DcdWriter:
    """Chunked writer of a little-endian CHARMM-style DCD file without unit-cell blocks (what ``open_trajectory`` maps).
    A chunk of k frames is one float32 *record image* of ``k * frame_words`` words: per frame the planes X[A], Y[A],
    Z[A], each between two 4-byte record markers.  ``layout()`` is where a kernel writes the coordinates inside such an
    image (the ``out_strides`` of hip.interpolate); ``append`` stamps the markers on the host and appends the image to
    the file; ``close`` writes the final frame count into the header.  Until then the header says 0 frames, so an
    interrupted file is refused by the reader instead of being taken for a shorter trajectory."""

    def __init__(self, path: str, n_atoms: int):
        if n_atoms < 1:
            raise ValueError(f"write_dcd: {n_atoms} atoms")
        self.path, self.n_atoms, self.n_frames = path, int(n_atoms), 0
        self.frame_words = 3 * (self.n_atoms + 2)
        self._file = open(path, "wb")
        self._file.write(self._header(0))

    def _header(self, n_frames: int) -> bytes:
        icntrl = np.zeros(20, dtype="<i4")
        icntrl[0], icntrl[1], icntrl[2], icntrl[3] = n_frames, 0, 1, n_frames   # frames, first step, steps between frames, steps
        icntrl[9] = np.float32(1.0).view(np.int32)                                # time step
        icntrl[19] = 24                                                           # CHARMM version: CHARMM-style layout, no cell (icntrl[10] = 0)
        title = _DCD_TITLE.ljust(80)
        return b"".join([np.int32(84).astype("<i4").tobytes(), b"CORD", icntrl.tobytes(), np.int32(84).astype("<i4").tobytes(),
                         np.asarray([84, 1], dtype="<i4").tobytes(), title, np.asarray([84], dtype="<i4").tobytes(),
                         np.asarray([4, self.n_atoms, 4], dtype="<i4").tobytes()])

    def layout(self) -> Tuple[int, int, int, int]:
        """(offset, frame_stride, atom_stride, comp_stride) of the coordinates inside a record image, in elements."""
        return 1, self.frame_words, 1, self.n_atoms + 2

    def image(self, n_frames: int) -> np.ndarray:
        """A zeroed record image of ``n_frames`` frames with the markers in place."""
        img = np.zeros(n_frames * self.frame_words, dtype=np.float32)
        self._stamp(img)
        return img

    def _stamp(self, img: np.ndarray) -> None:
        planes = img.view(np.int32).reshape(-1, self.n_atoms + 2)
        planes[:, 0] = planes[:, -1] = 4 * self.n_atoms

    def append(self, image: np.ndarray) -> None:
        """Append whole frames: a float32 record image (its marker slots may hold anything: they are stamped here)."""
        image = np.ascontiguousarray(image, dtype=np.float32).reshape(-1)
        if image.size % self.frame_words:
            raise ValueError(f"write_dcd: an image of {image.size} words is not a whole number of frames of {self.frame_words}")
        self._stamp(image)
        self._file.write(image.astype("<f4", copy=False).tobytes())
        self.n_frames += image.size // self.frame_words

    def close(self) -> None:
        if self._file is None:
            return
        self._file.seek(0)
        self._file.write(self._header(self.n_frames))
        self._file.close()
        self._file = None

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        elif self._file is not None:   # leave the header at 0 frames: the reader refuses the file
            self._file.close()
            self._file = None
        return False


def write_dcd(path: str, n_atoms: int) -> DcdWriter:
    """Open ``path`` for chunked DCD output (see :class:`DcdWriter`)."""
    return DcdWriter(path, n_atoms)


class XtcWriter:
    """Chunked writer of a GROMACS ``.xtc`` file.  A chunk is a finished *file image* -- whole big-endian frames, as
    hip.xtc_encode returns them -- so ``append`` only checks that the image starts with a frame of this writer's atom
    count and appends it.  The frames land under ``<path>.partial``; ``close`` renames that file to ``path``, so an
    interrupted run leaves nothing a restart could take for a finished ensemble."""

    def __init__(self, path: str, n_atoms: int):
        if n_atoms < 1:
            raise ValueError(f"write_xtc: {n_atoms} atoms")
        self.path, self.partial_path, self.n_atoms, self.n_bytes = path, path + ".partial", int(n_atoms), 0
        self._file = open(self.partial_path, "wb")

    def append(self, image) -> None:
        """Append whole frames: the bytes of a file image (bytes, or a uint8 array)."""
        data = image if isinstance(image, (bytes, bytearray, memoryview)) else np.ascontiguousarray(image, dtype=np.uint8).tobytes()
        if len(data) == 0:
            return
        if len(data) % 4 or len(data) < 56:
            raise ValueError(f"write_xtc: an image of {len(data)} bytes is not a whole number of frames (every field of the file takes 4 bytes)")
        magic, n = struct.unpack_from(">ii", data, 0)
        if magic != XTC_MAGIC or n != self.n_atoms:
            raise ValueError(f"write_xtc: the image starts with magic {magic} and {n} atoms, expected {XTC_MAGIC} and {self.n_atoms}")
        self._file.write(data)
        self.n_bytes += len(data)

    def close(self) -> None:
        if self._file is None:
            return
        self._file.close()
        self._file = None
        os.replace(self.partial_path, self.path)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        elif self._file is not None:   # nothing is left under the final name, and nothing half-written under the other
            self._file.close()
            self._file = None
            os.remove(self.partial_path)
        return False


def write_xtc(path: str, n_atoms: int) -> XtcWriter:
    """Open ``path`` for chunked XTC output (see :class:`XtcWriter`)."""
    return XtcWriter(path, n_atoms)


def extraction_chunks(frames: np.ndarray, frame_bytes: int, out_bytes: int, memory_budget: int) -> List[Tuple[int, int]]:
    """[lo, hi) ranges of the ascending frame indices ``frames`` so that a chunk's device memory -- the source frames from
    its first to its last index (``frame_bytes`` each, the skipped ones included) and ``out_bytes`` per chosen frame --
    stays within ``memory_budget``; a chunk holds at least one frame."""
    chunks, lo, n = [], 0, len(frames)
    while lo < n:
        hi = lo + 1
        while hi < n and (int(frames[hi]) - int(frames[lo]) + 1) * frame_bytes + (hi + 1 - lo) * out_bytes <= memory_budget:
            hi += 1
        chunks.append((lo, hi))
        lo = hi
    return chunks


def extract_frames(trajectory_path: str, topology_path: str, frames, out_path: str, memory_budget: Optional[int] = None,
                   precision: float = 1000.0) -> Optional[str]:
    """The frames ``frames`` of a trajectory (``.dcd``, mapped in place, or ``.npy``) written as the GROMACS ``.xtc`` file
    ``out_path``, in ascending order of their indices whatever order they are given in (reference md.py:715-760,
    extract_XTC).  The topology (a PDB) gives the atom count the trajectory must have.  An index outside the trajectory
    raises ValueError naming the file and the index; an empty list logs a warning and writes nothing (returns None).
    The frames go through the device in chunks of at most ``memory_budget`` bytes (default: a quarter of free device
    memory, at most 4 GiB): the source frames of a chunk are uploaded as they lie in the file, hip.xtc_encode gathers and
    compresses the chosen ones, and the finished file image is downloaded and appended.  Steps are the source frame
    indices, times those indices as float32, the box zeros: DCD input carries neither times nor, here, a box.
    No CPU fallback."""
    frames = np.sort(np.asarray(list(frames) if not isinstance(frames, np.ndarray) else frames, dtype=np.int64).reshape(-1))
    if frames.size == 0:
        logger.warning(f"No frames to extract from {trajectory_path}: {out_path} is not written.")
        return None
    traj = open_trajectory(trajectory_path, read_topology(topology_path).n_atoms)
    if frames[0] < 0 or frames[-1] >= traj.n_frames:
        bad = int(frames[0]) if frames[0] < 0 else int(frames[-1])
        raise ValueError(f"{trajectory_path}: frame {bad} asked for, the trajectory has frames 0 to {traj.n_frames - 1}")
    import torch

    from . import frame_io, hip   # frame_io builds on this module
    from ._lib import DcvError

    if not torch.cuda.is_available():
        raise DcvError("extract_frames needs an MI355X (cuda) device: XTC frames are encoded by libdcv.so, there is no CPU fallback")
    memory_budget = frame_io.resolve_budget(memory_budget)
    A = traj.n_atoms
    out_bytes = 2 * (13 * A + 4) + 92 + 120 + 48 + 8 + 4   # slot and image, pack record, descriptor, index, status
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with write_xtc(out_path, A) as writer:
        for lo, hi in extraction_chunks(frames, 4 * traj.frame_stride, out_bytes, int(memory_budget)):
            first, last = int(frames[lo]), int(frames[hi - 1])
            data, layout = traj.span(first, last + 1)
            buf = frame_io.upload(data)
            try:
                image = hip.xtc_encode(buf, A, strides=layout, frames=frames[lo:hi] - first, precision=precision, step=frames[lo:hi],
                                       time=frames[lo:hi].astype(np.float32))
            except DcvError as e:
                raise DcvError(f"{trajectory_path}: frames {first}..{last}: {e}") from None
            writer.append(image.cpu().numpy())
            del buf, image
    return out_path


def write_topology(path: str, top: Topology, atoms=None) -> None:
    """A PDB file of the atoms ``atoms`` (indices into ``top``, default all) with the topology's own positions and fields,
    renumbered from 1, and CONECT records for the bonds whose both ends are kept.  ``read_topology`` reads it back with
    equal fields; a topology whose bonds are all lost in the selection reads back without bonds (None)."""
    atoms = np.arange(top.n_atoms) if atoms is None else np.asarray(atoms, dtype=np.int64).reshape(-1)
    new = {int(a): i for i, a in enumerate(atoms)}
    lines = []
    for i, a in enumerate(atoms):
        a = int(a)
        name = top.names[a]
        name = name[:4] if len(name) >= 4 else " " + name.ljust(3)
        x, y, z = (float(v) for v in top.positions[a])
        lines.append(f"ATOM  {(i + 1) % 100000:5d} {name}{' '}{top.resnames[a][:4].ljust(4)}{(top.chains[a] or ' ')[:1]}"
                     f"{int(top.resids[a]):4d}    {x:8.3f}{y:8.3f}{z:8.3f}{1.0:6.2f}{0.0:6.2f}      {top.segids[a][:4].ljust(4)}")
    if top.bonds and len(atoms) < 100000:
        partners: Dict[int, List[int]] = {}
        for i, j in sorted(top.bonds):
            if i in new and j in new:
                partners.setdefault(new[i], []).append(new[j])
                partners.setdefault(new[j], []).append(new[i])
        for i in sorted(partners):
            for k in range(0, len(partners[i]), 4):
                lines.append("CONECT" + f"{i + 1:5d}" + "".join(f"{j + 1:5d}" for j in sorted(partners[i])[k:k + 4]))
    lines.append("END")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


# ------------------------------------------------------------------------------------------------ feature definitions
def _entity(top: Topology, i: int) -> str:
    return f"@{top.names[i]}_{int(top.resids[i])}"


def _heavy(top: Topology, atoms: np.ndarray) -> np.ndarray:
    return np.asarray([i for i in atoms if not top.names[i].startswith("H")], dtype=np.int64)   # "not name H*"


def _distance_group(top: Topology, group: Dict) -> List[Tuple[str, int, int]]:
    """(label, atom, atom) of one distance group, md.py:26-129."""
    sel1, sel2 = group.get("first_selection", "all"), group.get("second_selection", "all")
    first = _heavy(top, select_atoms(top, sel1))[::int(group.get("first_stride", 1))]
    second = _heavy(top, select_atoms(top, sel2))[::int(group.get("second_stride", 1))]
    if len(first) == 0:
        raise ValueError(f"First selection: '{sel1}' is empty, please review the selection string.")
    if len(second) == 0:
        raise ValueError(f"Second selection: '{sel2}' is empty, please review the selection string.")
    skip_neighbors, skip_bonded = bool(group.get("skip_neigh_residues", False)), bool(group.get("skip_bonded_atoms", False))
    pos = top.positions.astype(np.float64)
    seen: Set[str] = set()
    found = []
    for i in first:
        ei = _entity(top, i)
        for j in second:
            if i == j:
                continue
            ej = _entity(top, j)
            label = f"{ei}-{ej}"
            if label in seen or f"{ej}-{ei}" in seen:
                continue
            if skip_bonded:
                if top.bonds is not None:
                    if (min(i, j), max(i, j)) in top.bonds:
                        continue
                elif float(np.sqrt(((pos[i] - pos[j]) ** 2).sum())) < COVALENT_BOND_THRESHOLD:
                    continue
            if skip_neighbors and abs(int(top.resids[i]) - int(top.resids[j])) <= 1:
                continue
            seen.add(label)
            found.append((label, int(i), int(j)))
    return found


def _virtual_dihedrals(top: Topology, selection: str) -> List[Tuple[str, int, int, int, int]]:
    """(label, four atoms) of the virtual dihedrals of a selection, md.py:226-273.  The reference counts the HEAVY atoms
    of the selection but indexes the selection BEFORE the hydrogens were removed (md.py:265-268); with hydrogens in the
    selection that yields fewer dihedrals than there are heavy-atom quadruples and quadruples that contain hydrogens.
    Reproduced as it stands: feature names are the contract with models trained on the reference's output."""
    atoms = select_atoms(top, selection)
    n_heavy = len(_heavy(top, atoms))
    if n_heavy == 0:
        raise ValueError(f"Selection: '{selection}' is empty, please review the selection string.")
    found = []
    for i in range(3, n_heavy):
        quad = [int(atoms[i - 3]), int(atoms[i - 2]), int(atoms[i - 1]), int(atoms[i])]
        found.append(("-".join(_entity(top, a) for a in quad), *quad))
    return found


def feature_definitions(features_configuration: Dict, top: Topology) -> Tuple[List[str], np.ndarray]:
    """(names, defs): the feature names in the reference's order (distance groups, then dihedral groups, each in
    dictionary order; md.py:580-717) and the (n_defs, 6) int32 records [kind, a0, a1, a2, a3, out_column] of
    hip.featurize.  The atoms of a record are the ones that produced its label."""
    cfg = features_configuration or {}
    if cfg.get("coordinate_groups"):
        raise ValueError("coordinate_groups are not supported: coordinates need a per-frame optimal fit to a template")
    if cfg.get("distance_to_center_groups"):
        raise ValueError("distance_to_center_groups are not supported")
    names: List[str] = []
    defs: List[List[int]] = []
    for group in (cfg.get("distance_groups") or {}).values():
        for label, i, j in _distance_group(top, group or {}):
            defs.append([FEAT_DISTANCE, i, j, 0, 0, len(names)])
            names.append(f"dist-{label}")
    for group in (cfg.get("dihedral_groups") or {}).values():
        group = group or {}
        mode = group.get("search_mode", "real")
        if mode != "virtual":
            raise ValueError(f"search_mode '{mode}' is not supported: only 'virtual' dihedrals are computed")
        encode = bool(group.get("periodic_encoding", True))
        for label, a, b, c, d in _virtual_dihedrals(top, group.get("selection", "all")):
            defs.append([FEAT_TORSION_SINCOS if encode else FEAT_TORSION, a, b, c, d, len(names)])
            names.extend([f"sin-{label}", f"cos-{label}"] if encode else [f"tor-{label}"])
    if not names:
        raise ValueError("No features found, please check the features section of the configuration file and the topology.")
    return names, np.asarray(defs, dtype=np.int32).reshape(-1, 6)


# ------------------------------------------------------------------------------------------------ labels -> records
_LABEL_KINDS = {"dist": (FEAT_DISTANCE, 2), "tor": (FEAT_TORSION, 4), "sin": (FEAT_TORSION_SINCOS, 4), "cos": (FEAT_TORSION_SINCOS, 4)}


def _label_atoms(label: str, n_entities: int, rest: str, index: Dict[Tuple[str, int], List[int]]) -> List[int]:
    """The atoms of the entities ``@name_resid`` of a label, joined by '-' as ``feature_definitions`` joins them."""
    if "center_" in rest:
        raise ValueError(f"feature label '{label}': distances to a geometric center are not supported")
    if not rest.startswith("@"):
        raise ValueError(f"feature label '{label}' is not of the form <kind>-@name_resid-...")
    parts = rest[1:].split("-@")
    atoms = []
    for part in parts:
        name, sep, resid = part.rpartition("_")
        if not sep or not name or not re.fullmatch(r"-?\d+", resid):
            raise ValueError(f"feature label '{label}': entity '@{part}' is not of the form @name_resid")
        found = index.get((name, int(resid)), [])
        if len(found) != 1:
            if len(parts) == 1 and n_entities == 4:   # '@phi_5', '@psi_5', ...: a named dihedral of the reference's real search mode
                raise ValueError(f"feature label '{label}': named dihedrals ('@{part}') are not supported, only virtual dihedrals "
                                 "given by their four atoms")
            raise ValueError(f"feature label '{label}': entity '@{part}' matches {'no atom' if not found else f'{len(found)} atoms'} "
                             "of the topology" + (" (several chains? the label cannot tell them apart)" if found else ""))
        atoms.append(found[0])
    if len(atoms) != n_entities:
        raise ValueError(f"feature label '{label}' names {len(atoms)} atoms, its kind needs {n_entities}")
    return atoms


def definitions_from_labels(labels: List[str], top: Topology) -> np.ndarray:
    """The inverse of the naming rules of ``feature_definitions``: the (n_rec, 8) int32 records
    [kind, a0, a1, a2, a3, feature0, feature1, 0] of hip.featurize_project for the feature names of a model
    (features_labels.txt).  The position of a label is its feature index.  ``dist-@a-@b`` and ``tor-@a-@b-@c-@d`` give
    one record each (feature1 = -1); ``sin-X`` and ``cos-X`` of the same four atoms share ONE record (feature0 the sine,
    feature1 the cosine), the index of a partner the model does not keep is -1.  Records stand in the order in which
    the labels first name them.  Nothing is guessed: an entity that matches no atom or several, a duplicate label and
    every other form (``coord-``, ``center_`` entities, ``@phi_7``, ...) raise ValueError naming the label."""
    index: Dict[Tuple[str, int], List[int]] = {}
    for i, (name, resid) in enumerate(zip(top.names, top.resids)):
        index.setdefault((name, int(resid)), []).append(i)
    records: List[List[int]] = []
    sincos: Dict[Tuple[int, ...], int] = {}   # four atoms -> record
    seen: Set[str] = set()
    for feature, label in enumerate(labels):
        label = str(label)
        if label in seen:
            raise ValueError(f"feature label '{label}' appears twice")
        seen.add(label)
        kind_name, sep, rest = label.partition("-")
        if kind_name == "coord":
            raise ValueError(f"feature label '{label}': coordinate features are not supported (they need a per-frame optimal fit)")
        if not sep or kind_name not in _LABEL_KINDS:
            raise ValueError(f"feature label '{label}' is not a dist-, tor-, sin- or cos- label")
        kind, n_entities = _LABEL_KINDS[kind_name]
        atoms = _label_atoms(label, n_entities, rest, index)
        if kind != FEAT_TORSION_SINCOS:
            records.append([kind, *atoms, *([0] * (4 - n_entities)), feature, -1, 0])
            continue
        r = sincos.setdefault(tuple(atoms), len(records))
        if r == len(records):
            records.append([kind, *atoms, -1, -1, 0])
        records[r][5 if kind_name == "sin" else 6] = feature
    if not records:
        raise ValueError("no feature labels given")
    return np.asarray(records, dtype=np.int32).reshape(-1, 8)


def records_to_featurize_defs(records: np.ndarray, n_features: int) -> Tuple[np.ndarray, int, np.ndarray, np.ndarray]:
    """(defs, n_columns, src, dst): the (n_rec, 6) records of hip.featurize that fill a frames x n_columns matrix whose
    column i < n_features is feature i of ``records``.  A sine / cosine record whose two features are not neighbouring
    columns (a lone sine or cosine, or a pair the model's order separates) writes its two values into a scratch pair
    behind the features; column ``src[k]`` is then to be copied to column ``dst[k]``."""
    records = np.asarray(records, dtype=np.int32).reshape(-1, 8)
    defs = np.zeros((len(records), 6), dtype=np.int32)
    defs[:, :5] = records[:, :5]
    n_columns, src, dst = int(n_features), [], []
    for r, (kind, f0, f1) in enumerate(records[:, [0, 5, 6]].tolist()):
        if kind != FEAT_TORSION_SINCOS or (f0 >= 0 and f1 == f0 + 1):
            defs[r, 5] = f0
            continue
        defs[r, 5] = n_columns
        for k, f in enumerate((f0, f1)):
            if f >= 0:
                src.append(n_columns + k)
                dst.append(f)
        n_columns += 2
    return defs, n_columns, np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
