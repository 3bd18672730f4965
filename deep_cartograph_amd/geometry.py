"""Geometry analysis of trajectories on the device: RMSD, average structure, per-residue RMSF (hip.superpose) and dRMSD
(hip.featurize).  What the reference does with MDAnalysis, one Python iteration per frame (modules/md/md.py:1397-1574),
restated on the per-frame optimal superposition kernel.

Frames are streamed in chunks (frame_io.py): `Trajectory.span` slices of at most `memory_budget` bytes go to the device
as they are in the file, results come back per chunk.  No CPU fallback: without a device every function
raises DcvError.

Not reproduced: MDAnalysis rounds the aligned positions to float32 before the group RMSD and the RMSF, here they stay
float64; the analyses do not map residues between different topologies (align_trajectory's caller does, sequence.py):
selections are applied to each topology as it is and must select equally many atoms; mass weights are not supported (the reference
fits unweighted too)."""
from __future__ import annotations

import logging
from typing import Optional, Tuple

import numpy as np

from . import frame_io, trajectory
from ._lib import DcvError

logger = logging.getLogger(__name__)

ANGSTROM_TO_NM = 0.1   # PLUMED's length unit: dRMSD values are in nm


def _as_topology(top) -> trajectory.Topology:
    return top if isinstance(top, trajectory.Topology) else trajectory.read_topology(top)


def _as_trajectory(traj, n_atoms: int) -> trajectory.Trajectory:
    if isinstance(traj, trajectory.Trajectory):
        if traj.n_atoms != n_atoms:
            raise ValueError(f"{traj.n_atoms} atoms in the trajectory, {n_atoms} in the topology")
        return traj
    return trajectory.open_trajectory(traj, n_atoms)


def _select(top: trajectory.Topology, selection: str, what: str) -> np.ndarray:
    atoms = trajectory.select_atoms(top, selection)
    if atoms.size == 0:
        raise ValueError(f"{what}: '{selection}' is empty, please review the selection string.")
    return atoms


def _require_device(what: str):
    import torch

    if not torch.cuda.is_available():
        raise DcvError(f"{what} needs an MI355X (cuda) device: the geometry is computed by libdcv.so, there is no CPU fallback")
    return torch


def _chunks(traj: trajectory.Trajectory, per_frame_out: int, memory_budget: Optional[int]):
    """(lo, hi, device buffer, layout) of consecutive chunks of frames that fit the budget."""
    _require_device("analyze_geometry")
    n = traj.n_frames
    if n == 0:
        raise ValueError("the trajectory has no frames")
    chunk, ranges = frame_io.plan_chunks(n, 4 * traj.frame_stride + per_frame_out, frame_io.resolve_budget(memory_budget))
    logger.info(f"Superposing {n} frames in chunks of {chunk} frames")
    return frame_io.stream(traj, ranges)


def rmsd(traj, top, selection: str, fit_selection: str, ref_top=None, memory_budget: Optional[int] = None) -> np.ndarray:
    """float64 [n]: RMSD (Angstrom, unweighted) of the `selection` atoms to the reference structure after fitting every
    frame to it on the `fit_selection` atoms.  The reference structure is `ref_top`'s positions, else the positions of
    the topology itself (what the reference does, whatever its "first frame" log line says).  Selections are applied to
    each topology separately and must select equally many atoms, otherwise ValueError."""
    from . import hip

    top = _as_topology(top)
    ref = top if ref_top is None else _as_topology(ref_top)
    sel, fit = _select(top, selection, "selection"), _select(top, fit_selection, "fit_selection")
    ref_sel, ref_fit = _select(ref, selection, "selection (reference)"), _select(ref, fit_selection, "fit_selection (reference)")
    if len(sel) != len(ref_sel) or len(fit) != len(ref_fit):
        raise ValueError(f"Number of atoms in trajectory ({len(sel)} selected, {len(fit)} to fit) and reference ({len(ref_sel)}, {len(ref_fit)}) "
                         "selections do not match.")
    _require_device("rmsd")
    traj = _as_trajectory(traj, top.n_atoms)
    out = np.empty(traj.n_frames, dtype=np.float64)
    fit_ref, sel_ref = ref.positions[ref_fit].astype(np.float64), ref.positions[ref_sel].astype(np.float64)
    for lo, hi, buf, layout in _chunks(traj, 16, memory_budget):
        got = hip.superpose(buf, top.n_atoms, fit, fit_ref, sel=sel, sel_ref=sel_ref, strides=layout, want=("rmsd",))
        out[lo:hi] = got["rmsd"][:, 1].cpu().numpy()
    return out


MOMENT_LDS_BYTES = 64 * 1024 - 96   # what a workgroup of dcv_superpose has for one staged frame and its moment partials


def _moments(traj, fit, fit_ref, sel, sel_ref, memory_budget) -> np.ndarray:
    """[n_sel, 3, 2] float64: sums over all frames of d and d^2, d = aligned - sel_ref; chunks are added on the host.
    The kernel keeps 48 bytes of moment partials per selected atom in LDS beside one staged frame (12 bytes per atom of
    the union of both sets, at most twice that when a range of atoms is staged as rows), so a large selection is served in
    batches of atoms, each a call of its own on the chunk that is on the device; a batch's sums do not depend on the
    other batches."""
    from . import hip

    batch = (MOMENT_LDS_BYTES - 24 * len(fit)) // (48 + 24)
    if batch < 1:
        raise DcvError(f"{len(fit)} fit atoms leave no room for moments in LDS (at most {MOMENT_LDS_BYTES // 24 - 3})")
    total = np.zeros((len(sel), 3, 2), dtype=np.float64)
    for _, _, buf, layout in _chunks(traj, 0, memory_budget):
        for lo in range(0, len(sel), batch):
            part = hip.superpose(buf, traj.n_atoms, fit, fit_ref, sel=sel[lo:lo + batch], sel_ref=sel_ref[lo:lo + batch], strides=layout,
                                 want=("moments",))
            total[lo:lo + batch] += part["moments"].cpu().numpy()
    return total


def average_structure(traj, top, fit_selection: str, memory_budget: Optional[int] = None) -> np.ndarray:
    """float64 [n_fit, 3]: the mean of the `fit_selection` atoms over the trajectory after fitting every frame to frame 0
    on those atoms (MDAnalysis' AverageStructure with ref_frame=0)."""
    top = _as_topology(top)
    fit = _select(top, fit_selection, "fit_selection")
    _require_device("average_structure")
    traj = _as_trajectory(traj, top.n_atoms)
    first = traj.frames(0, 1)[0][fit].astype(np.float64)
    return first + _moments(traj, fit, first, fit, first, memory_budget)[:, :, 0] / traj.n_frames


def rmsf(traj, top, selection: str, fit_selection: str, memory_budget: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(per-residue mean RMSF in Angstrom, residue numbers ascending): every frame is fitted on the `fit_selection`
    atoms to their average structure (kept in float64); the RMSF of a `selection` atom is sqrt(sum_c var_c) of its aligned
    positions with ddof = 0, and a residue's value is the mean over its selected atoms.  The selection may be as large as one
    frame's staging allows (5 461 atoms with the fit atoms): it is served in batches of atoms.  The fit set is limited to
    2 726 atoms here and in `average_structure` (the moment partials share LDS with the staged frame); `rmsd` takes 5 461."""
    top = _as_topology(top)
    sel, fit = _select(top, selection, "selection"), _select(top, fit_selection, "fit_selection")
    _require_device("rmsf")
    traj = _as_trajectory(traj, top.n_atoms)
    average = average_structure(traj, top, fit_selection, memory_budget)
    # the shift of the moments is arbitrary for a variance: frame 0 is close to every frame's aligned position
    shift = traj.frames(0, 1)[0][sel].astype(np.float64)
    m = _moments(traj, fit, average, sel, shift, memory_budget) / traj.n_frames
    var = np.maximum(m[:, :, 1] - m[:, :, 0] ** 2, 0.0)
    per_atom = np.sqrt(var.sum(axis=1))
    resids = top.resids[sel]
    residues = np.unique(resids)
    return np.asarray([per_atom[resids == r].mean() for r in residues], dtype=np.float64), residues


def align_frame_bytes(traj: trajectory.Trajectory, dcd: bool) -> int:
    """Device bytes one frame of an `align_trajectory` chunk takes: its input record, its output record (DCD image or
    dense row) and its transform row."""
    words_out = 3 * (traj.n_atoms + 2) if dcd else 3 * traj.n_atoms
    return 4 * traj.frame_stride + 4 * words_out + 128


def align_trajectory(traj, top, fit, fit_ref, output_path: str, memory_budget: Optional[int] = None) -> np.ndarray:
    """Fits every frame onto `fit_ref` (n_fit x 3, Angstrom) on the atoms `fit` (unweighted, hip.superpose) and writes
    ALL atoms of every frame, moved by the frame's transform (hip.transform_frames), to `output_path`: a `.dcd` without
    unit-cell blocks or a `.npy` of (n, A, 3) float32.  Returns the aligned first frame, float32 [A, 3].  Frames go
    through the device in chunks that hold their input records and their output image at once, at most `memory_budget`
    bytes (default: a quarter of free device memory, at most 4 GiB), into a frame_io.CoordinateSink: they land under
    `<output_path>.partial` and are renamed at the end.  The fit set is bounded by dcv_superpose's staging limit of 5 461 atoms; the number of atoms
    written is not bounded.  float64 arithmetic with one rounding (MDAnalysis translates, rotates and translates in
    float32)."""
    from . import hip

    _require_device("align_trajectory")
    top = _as_topology(top)
    traj = _as_trajectory(traj, top.n_atoms)
    ext = frame_io.coordinate_format(output_path, "the aligned trajectory")
    fit = np.asarray(fit, dtype=np.int64).reshape(-1)
    fit_ref = np.asarray(fit_ref, dtype=np.float64)
    n, A = traj.n_frames, traj.n_atoms
    if n == 0:
        raise ValueError("the trajectory has no frames")
    chunk, ranges = frame_io.plan_chunks(n, align_frame_bytes(traj, ext == ".dcd"), frame_io.resolve_budget(memory_budget))
    logger.info(f"Aligning {n} frames of {A} atoms on {len(fit)} atoms in chunks of {chunk} frames")
    with frame_io.CoordinateSink(output_path, n, A) as sink:
        for lo, hi, buf, layout in frame_io.stream(traj, ranges):
            transform = hip.superpose(buf, A, fit, fit_ref, strides=layout, want=("transform",))["transform"]
            image = sink.image(hi - lo)
            hip.transform_frames(buf, A, transform, strides=layout, out=image, out_strides=sink.layout())
            sink.append(image)
            del buf, image
    return trajectory.open_trajectory(output_path).frames(0, 1)[0]


def drmsd(traj, top, selection: str, selection_stride: int, ref_top, memory_budget: Optional[int] = None) -> np.ndarray:
    """float64 [n]: sqrt(mean((d - d_ref)^2)) over the reference's distance group of the selection (first = second =
    `selection`, both strides `selection_stride`, pairs in the same or neighbouring residues and bonded pairs skipped),
    d from the trajectory and d_ref from the positions of `ref_top`.  The values are in NANOMETRES, as the reference's are:
    its distances come from PLUMED, whose length unit is nm, and it plots them under an "(A)" label all the same."""
    from . import hip

    top, ref = _as_topology(top), _as_topology(ref_top)
    group = {"first_selection": selection, "second_selection": selection, "first_stride": int(selection_stride),
             "second_stride": int(selection_stride), "skip_neigh_residues": True, "skip_bonded_atoms": True}
    features = {"distance_groups": {"distances": group}}
    names, defs = trajectory.feature_definitions(features, top)
    ref_names, ref_defs = trajectory.feature_definitions(features, ref)
    if names != ref_names:
        raise ValueError("The distances of the trajectory's topology differ from those of the reference topology; translating features "
                         "between topologies is out of scope")
    torch = _require_device("drmsd")
    traj = _as_trajectory(traj, top.n_atoms)
    one = torch.from_numpy(np.ascontiguousarray(ref.positions, dtype=np.float32)[None]).cuda()
    d_ref = hip.featurize(one, ref_defs, ref.n_atoms, unit=ANGSTROM_TO_NM).cpu().numpy()[0].astype(np.float64)
    out = np.empty(traj.n_frames, dtype=np.float64)
    for lo, hi, buf, layout in _chunks(traj, 4 * len(names), memory_budget):
        d = hip.featurize(buf, defs, top.n_atoms, strides=layout, unit=ANGSTROM_TO_NM).cpu().numpy().astype(np.float64)
        out[lo:hi] = np.sqrt(np.mean((d - d_ref) ** 2, axis=1))
    return out
