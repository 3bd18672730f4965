"""Trajectory augmentation on the device: new frames interpolated between the frames of a seed trajectory (a short
morph between two states, for instance), optionally with Gaussian noise, written as a trajectory plus a PDB of the
selection.  What the reference does with MDAnalysis and scipy on the host (modules/md/md.py:1018-1137,
tools/traj_augmentation/traj_augmentation.py), with the interpolation in hip.interpolate (csrc/interp.hip): PCHIP or
modified Akima along the frame axis of every coordinate column, float64 arithmetic, equal to scipy's
PchipInterpolator / Akima1DInterpolator(method="makima") to rounding.

Deliberate departures from the reference:

* ``akima`` extrapolates.  The reference's grid runs half a frame past the last knot and scipy's Akima default does
  not extrapolate, so the reference's last frames are NaN and poison compute_features; here they continue the last
  piece, as PCHIP does in both.
* ``traj_format`` is ``dcd`` (default) or ``npy``; ``xtc``, ``nc`` and ``pdb`` raise a ValueError naming the option
  (no compressed, NetCDF or multi-model PDB writer).
* ``prepare_trajectory: true`` raises likewise: unwrapping and centring need the box.
* The new frame times are float64.  Under NumPy 2 the reference's own grid comes out in float32 (its frame array is
  float32 and ``frames[0] + .5`` keeps that type: an accident of scalar promotion), which moves every time by up to
  2^-24 of its value; that rounding is not reproduced.

    python -m deep_cartograph_amd.augmentation -conf config.yml -traj_data morph.dcd -top_data morph.pdb \
           [-n 4] [-output traj_augmentation] [-v]
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
from pathlib import Path
from typing import Optional, Tuple

import numpy as np

logger = logging.getLogger(__name__)

WRITTEN_FORMATS = ("dcd", "npy")
KINDS = {"pchip": "pchip", "akima": "makima", None: "pchip"}   # interpolation_method -> kind of hip.interpolate


def new_frame_times(n: int, num_frames: int, keep_original_frames: bool) -> np.ndarray:
    """The float64 times of the new frames of a seed trajectory of ``n`` frames (frame k at time k), md.py:1094-1101.
    Originals dropped: ``linspace(0.5, n - 0.5, num_frames)`` -- the reference's grid, which runs half a frame past the
    last knot.  Originals kept: the n original times merged with ``num_frames - n`` new ones spread evenly between the
    first and the last."""
    n, num_frames = int(n), int(num_frames)
    if num_frames < 1:
        raise ValueError(f"num_frames must be at least 1, got {num_frames}")
    frames = np.arange(n, dtype=np.float64)
    if keep_original_frames:
        if num_frames < n:
            raise ValueError(f"num_frames ({num_frames}) is below the {n} frames of the trajectory, which keep_original_frames keeps")
        additional = np.linspace(frames[0], frames[-1], num_frames - n + 2)[1:-1]
        return np.sort(np.concatenate((frames, additional)))
    return np.linspace(frames[0] + 0.5, frames[-1] + 0.5, num_frames)


class NoiseStream:
    """Gaussian noise drawn chunk by chunk in (frame, atom, xyz) order: the stream of the reference's
    ``np.random.seed(seed); np.random.normal(0, std, shape)`` (the legacy generator keeps the spare value of its pair
    method between calls, so chunks of any size continue it bit for bit), without touching NumPy's global state."""

    def __init__(self, seed: int, std: float):
        self.state, self.std = np.random.RandomState(int(seed)), float(std)

    def draw(self, *shape: int) -> np.ndarray:
        return self.state.normal(0, self.std, shape)


def output_paths(trajectory_file: str, interpolation_method: Optional[str], traj_format: str, output_path: Optional[str] = None,
                 suffix: str = "") -> Tuple[str, str]:
    """<stem>_augmented_<method><suffix>.<ext> and .pdb, the reference's names (md.py:1081-1083)."""
    stem = f"{Path(trajectory_file).stem}_augmented_{interpolation_method}{suffix}"
    folder = output_path if output_path else "."
    return os.path.join(folder, f"{stem}.{traj_format}"), os.path.join(folder, f"{stem}.pdb")


def interpolate_trajectory(topology_file: str, trajectory_file: str, num_frames: int, keep_original_frames: bool = True,
                           interpolation_method: Optional[str] = "pchip", noise_std: Optional[float] = None, random_seed: int = 42,
                           atom_selection: str = "all", traj_format: str = "dcd", prepare_trajectory: bool = False,
                           output_path: Optional[str] = None, suffix: str = "", memory_budget: Optional[int] = None) -> Tuple[str, str]:
    """Interpolate the selected atoms of a trajectory to ``num_frames`` frames on the device and write the new
    trajectory and a PDB of the selection; returns (trajectory path, topology path).  Arguments and return value of
    the reference's function (md.py:1018-1137).  Existing outputs are skipped.  ``interpolation_method`` None emits the
    original frames (``num_frames`` is ignored, as in the reference).  The seed trajectory stays on the device as a
    whole -- makima's threshold looks at every knot --; the output frames are streamed in chunks of at most
    ``memory_budget`` bytes of device memory (default: a quarter of what is free, at most 4 GiB).  No CPU fallback."""
    import torch

    from . import frame_io, hip, trajectory
    from ._lib import DcvError

    if interpolation_method not in KINDS:
        raise ValueError(f"interpolation_method '{interpolation_method}' is not supported: use 'akima', 'pchip' or null")
    if traj_format not in WRITTEN_FORMATS:
        raise ValueError(f"traj_format '{traj_format}' is not supported: the augmented trajectory is written as one of {WRITTEN_FORMATS} "
                         "(there is no compressed, NetCDF or multi-model PDB writer)")
    if prepare_trajectory:
        raise ValueError("prepare_trajectory: true is not supported: unwrapping and centring need the box; prepare the trajectory beforehand")
    new_traj_path, new_top_path = output_paths(trajectory_file, interpolation_method, traj_format, output_path, suffix)
    if os.path.exists(new_traj_path) and os.path.exists(new_top_path):
        logger.info(f"Interpolated trajectory and topology already exist at {new_traj_path} and {new_top_path}. Skipping interpolation.")
        return new_traj_path, new_top_path
    if not torch.cuda.is_available():
        raise DcvError("traj_augmentation needs an MI355X (cuda) device: the frames are interpolated by libdcv.so, there is no CPU fallback")

    top = trajectory.read_topology(topology_file)
    sel = trajectory.select_atoms(top, atom_selection)
    if len(sel) == 0:
        raise ValueError(f"Selection '{atom_selection}' matched 0 atoms.")
    traj = trajectory.open_trajectory(trajectory_file, top.n_atoms)
    n = traj.n_frames
    kind = KINDS[interpolation_method]
    if n < (3 if kind == "makima" else 2):
        raise ValueError(f"{trajectory_file}: {n} frames, {interpolation_method} interpolation needs at least {3 if kind == 'makima' else 2}")
    times = np.arange(n, dtype=np.float64) if interpolation_method is None else new_frame_times(n, num_frames, keep_original_frames)
    n_out, ns = len(times), len(sel)
    logger.info(f"Interpolating {ns} atoms of {n} frames of {Path(trajectory_file).name} to {n_out} frames ({interpolation_method})")

    span, layout = traj.span(0, n)
    knots = frame_io.upload(span)
    noise = None if noise_std is None else NoiseStream(random_seed, noise_std)
    os.makedirs(os.path.dirname(new_traj_path) or ".", exist_ok=True)
    trajectory.write_topology(new_top_path, top, sel)
    words = 3 * (ns + 2) if traj_format == "dcd" else 3 * ns
    _, ranges = frame_io.plan_chunks(n_out, 4 * words + (24 * ns if noise else 0), frame_io.resolve_budget(memory_budget))
    with frame_io.CoordinateSink(new_traj_path, n_out, ns) as sink:
        for lo, hi in ranges:
            noise_d = torch.from_numpy(noise.draw(hi - lo, ns, 3)).cuda() if noise else None
            image = sink.image(hi - lo)
            hip.interpolate(knots, top.n_atoms, times[lo:hi], kind=kind, sel=sel, strides=layout, extrapolate=True, noise=noise_d,
                            out=image, out_strides=sink.layout())
            sink.append(image)
    return new_traj_path, new_top_path


def main(argv=None):
    from .common import read_configuration
    from .tools import traj_augmentation

    p = argparse.ArgumentParser("Deep Cartograph: Trajectory Augmentation (MI355X)",
                                description="Augments trajectory samples interpolating the existing frames.")
    p.add_argument("-conf", "-configuration", dest="configuration_path", type=str, required=True, help="Path to configuration file (.yml).")
    p.add_argument("-traj_data", dest="trajectory_data", required=True, nargs="+", help="trajectories to augment (.dcd / .npy; a GROMACS .xtc is imported first)")
    p.add_argument("-top_data", dest="topology_data", required=True, nargs="+", help="topology (.pdb): one for all, or one per trajectory")
    p.add_argument("-n", "-num_replicas", dest="num_replicas", type=int, default=1,
                   help="replicas of each trajectory; they differ by the noise (seed + replica)")
    p.add_argument("-output", dest="output_folder", type=str, default=None, help="Path to the output folder.")
    p.add_argument("-v", "--verbose", dest="verbose", action="store_true", default=False)
    a = p.parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if a.verbose else logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    traj_augmentation(read_configuration(a.configuration_path), a.trajectory_data, a.topology_data, num_replicas=a.num_replicas,
                      output_folder=a.output_folder or "traj_augmentation")


if __name__ == "__main__":
    main(sys.argv[1:])
