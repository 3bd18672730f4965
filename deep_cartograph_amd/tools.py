"""The tools of the CV-fit path with the reference's API (argument names, output tree,
CSV formats): align_trajectories (tools/align_trajectories/align_trajectories.py:70-189), analyze_geometry (tools/analyze_geometry/analyze_geometry.py:13-143), traj_augmentation (tools/traj_augmentation/traj_augmentation.py:23-131), compute_features (tools/compute_features/compute_features.py:25-227), filter_features (tools/filter_features/filter_features.py:22-31), train_colvars (tools/train_colvars/train_colvars.py:20-36), traj_projection
(tools/traj_projection/traj_projection.py:19-27), traj_cluster (tools/traj_cluster/traj_cluster.py:
18-28).  traj_cluster extracts its structures itself: centroid PDBs on the host, the frames of every cluster as GROMACS
.xtc files compressed on the device (trajectory.extract_frames).  Figures and FES estimation (matplotlib) are outside
the accelerated path and are not produced."""
from __future__ import annotations

import logging
import os
import sys
import time
from pathlib import Path
from typing import Dict, List, Literal, Optional, Union

import numpy as np
import pandas as pd

from . import statistics
from .common import merge_configurations, save_list, validate_configuration
from .cv_calculator import CVCalculator, calculator_class
from .schemas import AnalyzeGeometrySchema, ComputeFeaturesSchema, FilterFeaturesSchema, TrainColvarsSchema, TrajAugmentationSchema, TrajClusterSchema, TrajProjectionSchema

logger = logging.getLogger(__name__)


def _as_list(x):
    if x is None:
        return None
    return [x] if isinstance(x, str) else list(x)


def _one_topology_each(trajectories: List[str], topologies) -> List[str]:
    """The topologies as a list, a single one repeated for every trajectory."""
    topologies = _as_list(topologies) or []
    return topologies * len(trajectories) if len(topologies) == 1 else topologies


def _pair_topologies(trajectories: List[str], topologies, others=(), must_exist: bool = True) -> List[str]:
    """One topology per trajectory (one serves all, or one each); with `must_exist` every path given, `others` included,
    is checked (traj_projection leaves that to the calculator, behind its restart check)."""
    topologies = _one_topology_each(trajectories, topologies)
    if len(trajectories) != len(topologies):
        raise ValueError(f"Number of trajectories ({len(trajectories)}) and topologies ({len(topologies)}) do not match.")
    for path in (trajectories + topologies + [p for p in others if p]) if must_exist else []:
        if not os.path.exists(path):
            raise FileNotFoundError(f"File not found: {path}")
    return topologies


ANGSTROM_TO_NM = 0.1   # PLUMED's length unit


def import_trajectories(trajectories: Union[str, List[str]], output_folder: str, traj_format: Literal["dcd", "npy"] = "dcd", traj_stride: int = 1,
                        memory_budget: Optional[int] = None) -> List[str]:
    """GROMACS ``.xtc`` trajectories decoded on the device (hip.xtc_decode) into <out>/<trajectory stem>.dcd (or .npy, (n, A, 3)
    float32), in Angstrom, every `traj_stride`-th frame; returns the paths in the order given.  Inputs that are not
    ``.xtc`` pass through unchanged and a trajectory whose output exists is skipped.  Each file is indexed on the host
    (trajectory.index_xtc), then the compressed bytes of a chunk of frames are uploaded, decoded straight into a device
    image of DCD frame records, downloaded and appended; chunks take at most `memory_budget` bytes of device memory
    (default: a quarter of what is free, at most 4 GiB).  The file is written under a temporary name and renamed at the
    end.  The box, the steps and the times of the frames are not written (xtc.py).  The tools that take trajectories call
    this themselves for ``.xtc`` inputs, into <their output folder>/xtc_import.  No CPU fallback."""
    from . import xtc

    return xtc.import_trajectories(trajectories, output_folder, traj_format, traj_stride, memory_budget)


def _route_xtc(trajectories, output_folder: str, memory_budget: Optional[int] = None):
    """``.xtc`` inputs imported into <output_folder>/xtc_import and replaced by the .dcd; everything else as it came."""
    from . import xtc

    return xtc.route(trajectories, output_folder, memory_budget)


def compute_features(configuration: Dict, trajectory_data: Union[str, List[str]], topology_data: Union[str, List[str]],
                     reference_topology: Optional[str] = None, traj_stride: Optional[int] = None,
                     output_folder: str = "compute_features", memory_budget: Optional[int] = None) -> List[str]:
    """Distances and virtual dihedrals of every trajectory, computed on the device from the coordinates (hip.featurize)
    instead of by a `plumed driver` subprocess.  Writes <out>/<trajectory stem>/colvars.npy + colvars.names.txt (the
    binary fast path of colvars.py), or colvars.dat with `colvars_format: dat`, and returns those paths; a trajectory
    whose output exists is skipped.  One topology serves all trajectories, or one per trajectory; all must give the
    feature names of `reference_topology` (default: the first).  `traj_stride` overrides plumed_settings.traj_stride.
    Frames are streamed in chunks of at most `memory_budget` bytes of device memory (default: a quarter of what is free,
    at most 4 GiB; a chunk's frame records also exist once as a host copy while they are uploaded) and the rows written
    into a memory-mapped .npy, so neither side ever holds a whole matrix twice.  No CPU fallback."""
    import torch

    from . import frame_io, hip, trajectory
    from ._lib import DcvError
    from .colvars import write_colvars

    t0 = time.time()
    trajectories = _route_xtc(_as_list(trajectory_data) or [], output_folder, memory_budget)
    if not trajectories:
        raise ValueError("compute_features: no trajectories given")
    topologies = _pair_topologies(trajectories, topology_data, [reference_topology])
    os.makedirs(output_folder, exist_ok=True)
    configuration = validate_configuration(configuration or {}, ComputeFeaturesSchema, output_folder)
    binary = configuration["colvars_format"] == "npy"
    colvars_paths = [os.path.join(output_folder, Path(t).stem, "colvars.npy" if binary else "colvars.dat") for t in trajectories]
    if all(os.path.exists(p) for p in colvars_paths):
        logger.info(f"Colvars files already exist in {output_folder}. Skipping feature computation.")
        return colvars_paths
    if not torch.cuda.is_available():
        raise DcvError("compute_features needs an MI355X (cuda) device: the features are computed by libdcv.so, there is no CPU fallback")
    stride = int(traj_stride or configuration["plumed_settings"]["traj_stride"])
    if stride < 1:
        raise ValueError(f"traj_stride must be at least 1, got {stride}")
    features_configuration = configuration["plumed_settings"]["features"]
    ref_names, _ = trajectory.feature_definitions(features_configuration, trajectory.read_topology(reference_topology or topologies[0]))
    memory_budget = frame_io.resolve_budget(memory_budget)
    for traj_path, top_path, out_path in zip(trajectories, topologies, colvars_paths):
        if os.path.exists(out_path):
            logger.info(f"Skipping {Path(traj_path).stem}. Colvars file already exists.")
            continue
        top = trajectory.read_topology(top_path)
        names, defs = trajectory.feature_definitions(features_configuration, top)
        if names != ref_names:
            raise ValueError(f"The features of {top_path} differ from those of the reference topology; translating features "
                             "between topologies is out of scope")
        traj = trajectory.open_trajectory(traj_path, top.n_atoms)
        n = traj.layout(0, None, stride)[0]
        if n == 0:
            raise ValueError(f"{traj_path}: no frames")
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        # rows land in a memory-mapped .npy under a temporary name: an interrupted run leaves nothing a restart would take for done
        tmp_path = os.path.join(os.path.dirname(out_path), "colvars.partial.npy")
        rows = np.lib.format.open_memmap(tmp_path, mode="w+", dtype=np.float32, shape=(n, len(names)))
        chunk, ranges = frame_io.plan_chunks(n, 4 * (stride * traj.frame_stride + len(names)), memory_budget)
        logger.info(f"Computing {len(names)} features of {n} frames of {Path(traj_path).name} in chunks of {chunk} frames")
        for lo, hi, buf, layout in frame_io.stream(traj, ranges, stride):
            block = hip.featurize(buf, defs, top.n_atoms, strides=layout, unit=ANGSTROM_TO_NM).cpu().numpy()
            if np.isnan(block).any():
                raise ValueError(f"NaNs in the features of frames {lo * stride}..{(hi - 1) * stride} of {traj_path}: check the coordinates")
            rows[lo:hi] = block
            del buf
        rows.flush()
        if binary:
            del rows
            with open(out_path[:-4] + ".names.txt", "w") as f:
                f.write("\n".join(names) + "\n")
            os.replace(tmp_path, out_path)
        else:
            write_colvars(out_path + ".partial", rows, names)
            del rows
            os.replace(out_path + ".partial", out_path)
            os.remove(tmp_path)
    logger.info("Elapsed time (Compute features): %s", time.strftime("%H h %M min %S s", time.gmtime(time.time() - t0)))
    return colvars_paths


def analyze_geometry(configuration: Dict, trajectories: List[str], topologies: List[str], ref_topologies: Optional[List[str]] = None,
                     output_folder: str = "analyze_geometry", memory_budget: Optional[int] = None) -> Dict[str, str]:
    """RMSD, per-residue RMSF and dRMSD of every trajectory, computed on the device (geometry.py) instead of frame by
    frame with MDAnalysis.  The loop, the keys and the x axes are the reference's: RMSD per trajectory and reference
    (`<traj>first_frame` against the topology's own positions, `<traj>_to_<ref stem>` otherwise) and dRMSD per
    trajectory and reference (the topology when there is none) over arange(n) * dt_per_frame * 1e-3, RMSF per trajectory
    over residue numbers.  Each series goes to a CSV in the format of the reference's save_data (header
    `x_label,y_label`, np.savetxt); the files are named `<analysis name>_<category>_<key>.csv` -- the reference names
    them `<key>.csv`, so two analyses of one trajectory overwrite each other.  No figures.  Returns {file stem: path}
    of what was written (empty with `run: false`).  dRMSD values are in nm under the reference's "(A)" label, as the
    reference's are.  `memory_budget` bounds a chunk of frames on the device.  Limits: fit and selected atoms together
    at most 5 461 per analysis, and an RMSF's fit selection at most 2 726 atoms (geometry.rmsf).  No CPU fallback."""
    import torch

    from . import geometry
    from ._lib import DcvError

    t0 = time.time()
    trajectories = _route_xtc(_as_list(trajectories) or [], output_folder, memory_budget)
    ref_topologies = _as_list(ref_topologies)
    topologies = _pair_topologies(trajectories, topologies, ref_topologies or [])
    os.makedirs(output_folder, exist_ok=True)
    configuration = validate_configuration(configuration or {}, AnalyzeGeometrySchema, output_folder)
    written: Dict[str, str] = {}
    if not configuration["run"]:
        logger.info("Skipping Analyze Geometry step.")
        return written
    if any(configuration["analysis"].values()) and not torch.cuda.is_available():
        raise DcvError("analyze_geometry needs an MI355X (cuda) device: the geometry is computed by libdcv.so, there is no CPU fallback")
    dt_per_frame = float(configuration["dt_per_frame"]) * 1e-3   # ns
    for category, analyses in configuration["analysis"].items():
        for name, params in (analyses or {}).items():
            logger.info(f"Analyzing {category}: {name}")
            y_label = f"{category} (A)"
            x_label = "Residue" if category == "RMSF" else "Time (ns)"
            x_data, y_data = {}, {}
            for traj_path, top_path in zip(trajectories, topologies):
                traj_name = Path(traj_path).stem
                if category == "RMSD":
                    for ref in ref_topologies or [None]:
                        key = traj_name + (f"_to_{Path(ref).stem}" if ref else "first_frame")
                        y_data[key] = geometry.rmsd(traj_path, top_path, params["selection"], params["fit_selection"], ref, memory_budget)
                        x_data[key] = np.arange(len(y_data[key])) * dt_per_frame
                elif category == "RMSF":
                    y_data[traj_name], x_data[traj_name] = geometry.rmsf(traj_path, top_path, params["selection"], params["fit_selection"],
                                                                         memory_budget)
                elif category == "dRMSD":
                    for ref in ref_topologies or [top_path]:
                        key = f"{traj_name}_to_{Path(ref).stem}"
                        y_data[key] = geometry.drmsd(traj_path, top_path, params["selection"], params["selection_stride"], ref, memory_budget)
                        x_data[key] = np.arange(len(y_data[key])) * dt_per_frame
            for key, y in y_data.items():
                stem = f"{name}_{category}_{key}"
                written[stem] = os.path.join(output_folder, stem + ".csv")
                np.savetxt(written[stem], np.column_stack((x_data[key], y)), delimiter=",", header=f"{x_label},{y_label}", comments="")
    logger.info("Elapsed time (Analyze geometry): %s", time.strftime("%H h %M min %S s", time.gmtime(time.time() - t0)))
    return written


def traj_augmentation(configuration: Dict, trajectories: Union[str, List[str]], topologies: Union[str, List[str]], num_replicas: int = 1,
                      output_folder: str = "traj_augmentation", memory_budget: Optional[int] = None):
    """New frames interpolated between the frames of every (seed) trajectory on the device (augmentation.py,
    hip.interpolate) instead of with scipy on the host, `num_replicas` times each: replica r draws its noise with
    `random_seed + r` and, with more than one replica, carries the suffix `_rep<r>` (the reference's rule).  Writes
    <out>/<stem>_augmented_<method><suffix>.<traj_format> and .pdb and returns (trajectories, topologies), as the
    reference's tool does; existing outputs are skipped.  One topology serves all trajectories, or one per trajectory.
    `memory_budget` bounds a chunk of output frames on the device.  No CPU fallback."""
    from . import augmentation

    t0 = time.time()
    trajectories = _route_xtc(_as_list(trajectories) or [], output_folder, memory_budget)
    topologies = _pair_topologies(trajectories, topologies)
    os.makedirs(output_folder, exist_ok=True)
    configuration = validate_configuration(configuration or {}, TrajAugmentationSchema, output_folder)
    augmented_trajectories, augmented_topologies = [], []
    for traj_path, top_path in zip(trajectories, topologies):
        for replica in range(num_replicas):
            new_traj, new_top = augmentation.interpolate_trajectory(
                topology_file=top_path, trajectory_file=traj_path, num_frames=configuration["num_frames"],
                keep_original_frames=configuration["keep_original_frames"], interpolation_method=configuration["interpolation_method"],
                noise_std=configuration["noise_std"], random_seed=configuration["random_seed"] + replica,
                atom_selection=configuration["atom_selection"], traj_format=configuration["traj_format"],
                prepare_trajectory=configuration["prepare_trajectory"], output_path=output_folder,
                suffix=f"_rep{replica}" if num_replicas > 1 else "", memory_budget=memory_budget)
            augmented_trajectories.append(new_traj)
            augmented_topologies.append(new_top)
    logger.info("Elapsed time (Trajectory Augmentation): %s", time.strftime("%H h %M min %S s", time.gmtime(time.time() - t0)))
    return augmented_trajectories, augmented_topologies


def align_trajectories(trajectory_data: Union[str, List[str]], topology_data: Union[str, List[str]], ref_topology: Optional[str] = None,
                       output_folder: str = "align_trajectories", memory_budget: Optional[int] = None):
    """Every trajectory superposed frame by frame onto the reference topology (default: the first topology) and written
    with ALL its atoms, on the device (geometry.align_trajectory: hip.superpose for the fit, hip.transform_frames for
    the atoms) instead of with MDAnalysis' AlignTraj.  The fit atoms are the C-alpha atoms of the residues that a local
    sequence alignment (sequence.py, in place of Biopython) maps from the reference into every topology; they pair up
    in topology order on both sides (MDAnalysis with match_atoms=False), and unequal counts raise ValueError.  Writes
    <out>/<trajectory file name> in the input's format (.dcd or .npy) and <out>/<topology stem>.pdb with all atoms at
    the positions of the first aligned frame, and returns (aligned trajectories, aligned topologies) -- the reference
    returns None.  One topology serves all trajectories, or one per trajectory.  Without common residues an error is
    logged and nothing is written, as in the reference.  Limits: at most 5 461 fit atoms (dcv_superpose's staging), so
    5 461 common residues; any number of atoms is written.  The unit-cell block of an input DCD is not carried over and
    the header times are the writer's.  `memory_budget` bounds a chunk of frames (input and output) on the device.  No
    CPU fallback."""
    import dataclasses

    import torch

    from . import geometry, sequence, trajectory
    from ._lib import DcvError

    t0 = time.time()
    trajectories = _route_xtc(_as_list(trajectory_data) or [], output_folder, memory_budget)
    if not trajectories:
        logger.warning("No trajectories provided. Nothing to align.")
        return [], []
    topologies = _pair_topologies(trajectories, topology_data, [ref_topology])
    if ref_topology is None:
        ref_topology = topologies[0]
        logger.info(f"No reference topology provided. Using first topology as reference: {Path(ref_topology).name}")
    out_trajs = [os.path.join(output_folder, Path(t).name) for t in trajectories]
    out_tops = [os.path.join(output_folder, Path(t).stem + ".pdb") for t in topologies]
    for src, dst in zip(trajectories, out_trajs):
        if os.path.splitext(src)[1].lower() not in (".dcd", ".npy"):
            raise ValueError(f"{src}: unsupported trajectory format (supported: .dcd, .npy)")
        if os.path.realpath(src) == os.path.realpath(dst):
            raise ValueError(f"The aligned trajectory would be written over its input {src}, which is memory-mapped while it is read: "
                             "choose another output folder")
    ref = trajectory.read_topology(ref_topology)
    tops = {p: trajectory.read_topology(p) for p in dict.fromkeys(topologies)}
    common = sequence.common_resids(ref, [tops[p] for p in tops])
    logger.info(f"Found {len(common)} common residues across all topologies.")
    if not common:
        logger.error("No common residues found across topologies. Cannot align trajectories.")
        return [], []
    if not torch.cuda.is_available():
        raise DcvError("align_trajectories needs an MI355X (cuda) device: the frames are fitted and moved by libdcv.so, there is no CPU fallback")
    os.makedirs(output_folder, exist_ok=True)
    for traj_path, top_path, out_traj, out_top in zip(trajectories, topologies, out_trajs, out_tops):
        top = tops[top_path]
        ref_fit, fit = sequence.fit_atoms(ref, top, common, what=top_path)
        fit_ref = ref.positions[ref_fit].astype(np.float64)
        logger.info(f"Aligning trajectory '{Path(traj_path).name}' with topology '{Path(top_path).name}' on {len(fit)} C-alpha atoms")
        first = geometry.align_trajectory(traj_path, top, fit, fit_ref, out_traj, memory_budget)
        trajectory.write_topology(out_top, dataclasses.replace(top, positions=first))
    logger.info("Elapsed time (Align trajectories): %s", time.strftime("%H h %M min %S s", time.gmtime(time.time() - t0)))
    return out_trajs, out_tops


def filter_features(configuration: Dict, colvars_paths: Union[str, List[str]], waypoint_colvars_paths: Optional[List[str]] = None,
                    csv_summary: bool = True, topologies: Optional[List[str]] = None, waypoint_topologies: Optional[List[str]] = None,
                    reference_topology: Optional[str] = None, output_folder: str = "filter_features") -> str:
    """Select the features that carry information about the transitions: Hartigan's dip test, Shannon entropy and
    standard deviation filters over the time series, waypoint filters over a few structures.  Writes
    <out>/all_features.txt, <out>/filter_summary.csv (csv_summary) and <out>/filtered_features.txt and returns the
    path of the latter -- the `features_list` file train_colvars and the CLI's -features accept.  Returns early when
    that file exists."""
    from .features import Filter

    t0 = time.time()
    output_features_path = os.path.join(output_folder, "filtered_features.txt")
    if os.path.exists(output_features_path):
        logger.info(f"Filtered features file already exists: {output_features_path}. Skipping filtering.")
        return output_features_path
    os.makedirs(output_folder, exist_ok=True)
    configuration = validate_configuration(configuration or {}, FilterFeaturesSchema, output_folder)
    colvars_paths = _as_list(colvars_paths)
    for path in colvars_paths:
        if not os.path.exists(path):
            raise FileNotFoundError(f"Colvars file not found: {path}")
    if topologies:
        if reference_topology is None:
            reference_topology = topologies[0]
        elif not os.path.exists(reference_topology):
            logger.error(f"Reference topology file missing: {reference_topology}")
            sys.exit(1)
    filtered_features = Filter(settings=configuration["filter_settings"], colvars_paths=colvars_paths,
                               waypoint_colvars_paths=waypoint_colvars_paths, topologies=topologies,
                               waypoint_topologies=waypoint_topologies, reference_topology=reference_topology,
                               output_dir=output_folder).run(csv_summary)
    save_list(filtered_features, output_features_path)
    logger.info("Elapsed time (Filter features): %s", time.strftime("%H h %M min %S s", time.gmtime(time.time() - t0)))
    return output_features_path


def train_colvars(configuration: Dict, train_colvars_paths: Union[str, List[str]], train_topologies: Optional[List[str]] = None,
                  trajectory_names: Optional[List[str]] = None, val_colvars_paths: Optional[Union[str, List[str]]] = None,
                  val_topologies: Optional[List[str]] = None, sup_topologies: Optional[List[str]] = None,
                  sup_traj_names: Optional[List[str]] = None, waypoint_structures: Optional[List[str]] = None,
                  reference_topology: Optional[str] = None, features_list: Optional[List[str]] = None,
                  dimension: Optional[int] = None,
                  cvs: Optional[List[Literal["pca", "ae", "tica", "htica", "deep_tica", "vae"]]] = None,
                  frames_per_sample: Optional[int] = 1, output_folder: str = "train_colvars") -> Dict[str, List[str]]:
    """Fit every requested CV, project the training frames, write
    <out>/<cv>/model.zip and <out>/<cv>/traj_data/<traj>/projected_trajectory.csv ('%.4f').
    Returns {cv_name: [csv path per training trajectory]}."""
    t0 = time.time()
    os.makedirs(output_folder, exist_ok=True)
    configuration = validate_configuration(configuration, TrainColvarsSchema, output_folder)
    train_colvars_paths = _as_list(train_colvars_paths)
    val_colvars_paths = _as_list(val_colvars_paths)
    if trajectory_names is None:
        trajectory_names = [Path(p).stem for p in train_colvars_paths]
    cvs_list = list(cvs) if cvs else list(configuration["cvs"])
    unsupported = [c for c in cvs_list if calculator_class(c) is None]
    for c in unsupported:
        logger.warning(f"CV '{c}' is outside the accelerated path (umap) and is skipped.")
    cvs_list = [c for c in cvs_list if calculator_class(c) is not None]
    logger.info(f"Collective variables to compute: {cvs_list}")
    output_paths: Dict[str, List[str]] = {}
    for cv_name in cvs_list:
        cv_folder = os.path.join(output_folder, cv_name)
        # restart support: skip a CV whose model and projections already exist (train_colvars_workflow.py:184-199)
        expected = [os.path.join(cv_folder, "traj_data", n, "projected_trajectory.csv") for n in trajectory_names]
        if os.path.exists(os.path.join(cv_folder, "model.zip")) and all(os.path.exists(p) for p in expected):
            logger.info(f"{cv_name}: already computed, skipping.")
            output_paths[cv_name] = expected
            continue
        merged = merge_configurations(configuration["common"], configuration.get(cv_name, {}))
        calc = calculator_class(cv_name)(configuration=merged, output_path=output_folder)
        calc.load_training_data(train_colvars_paths, train_topologies, reference_topology, features_list)
        if val_colvars_paths:
            calc.load_validation_data(val_colvars_paths, val_topologies, reference_topology, features_list)
        df = calc.run(dimension)
        if df is None:
            logger.warning(f"Projected colvars dataframe is empty for {cv_name}. Skipping this CV.")
            continue
        df["traj_label"] = calc.training_data_labels
        paths = []
        # under torch.distributed every rank holds the projection of all frames (run() gathers it): rank 0 writes
        writer = calc.comm.rank == 0
        for i, name in enumerate(trajectory_names):
            traj_folder = os.path.join(cv_folder, "traj_data", name)
            p = os.path.join(traj_folder, "projected_trajectory.csv")
            if writer:
                os.makedirs(traj_folder, exist_ok=True)
                topology = train_topologies[i] if train_topologies else None
                calc.write_plumed_files(topology, os.path.join(traj_folder, "plumed_inputs"), waypoint_structures)
                df_i = df[df["traj_label"] == i].drop("traj_label", axis=1)
                df_i.to_csv(p, index=False, float_format="%.4f")
            paths.append(p)
        calc.comm.barrier()
        output_paths[cv_name] = paths
    logger.info("Elapsed time (Train colvars): %s", time.strftime("%H h %M min %S s", time.gmtime(time.time() - t0)))
    return output_paths


def traj_projection(configuration: Dict, colvars_paths: List[str], topologies: List[str] = None, trajectory_names: List[str] = None,
                    model_paths: List[str] = None, model_traj_paths: Optional[List[List[str]]] = None,
                    output_folder: Optional[str] = "traj_projection", *, trajectories: Optional[List[str]] = None) -> Dict[str, List[str]]:
    """Project new colvars files onto saved models: <out>/<cv>/<traj>/projected_trajectory.csv.  With `trajectories`
    (.dcd / .npy; a GROMACS .xtc is imported first) instead of `colvars_paths` every model projects the coordinates themselves (project_trajectory): the
    features it needs are recomputed on the device from its own feature names and the topology (`topologies`: one for
    all trajectories, or one each), no colvars file and no features configuration involved."""
    colvars_paths, trajectories = _as_list(colvars_paths) or [], _route_xtc(_as_list(trajectories), output_folder)
    from_coordinates = trajectories is not None
    if from_coordinates:
        import torch

        from ._lib import DcvError

        if colvars_paths:
            raise ValueError("traj_projection: give either colvars_paths or trajectories, not both")
        topologies = _pair_topologies(trajectories, topologies, must_exist=False)
        if not torch.cuda.is_available():
            raise DcvError("traj_projection of trajectories needs an MI355X (cuda) device: the features are computed by libdcv.so, "
                           "there is no CPU fallback")
    os.makedirs(output_folder, exist_ok=True)
    validate_configuration(configuration or {}, TrajProjectionSchema, output_folder)
    inputs = trajectories if from_coordinates else colvars_paths
    if trajectory_names is None:
        trajectory_names = [Path(p).stem for p in inputs]
    out: Dict[str, List[str]] = {}
    for model_path in model_paths or []:
        calc = CVCalculator.load(model_path, output_folder)
        paths = []
        for i, (cp, name) in enumerate(zip(inputs, trajectory_names)):
            folder = os.path.join(output_folder, calc.cv_name, name)
            p = os.path.join(folder, "projected_trajectory.csv")
            if os.path.exists(p):  # traj_projection_workflow.py:235-238
                paths.append(p)
                continue
            if from_coordinates:
                df = calc.project_trajectory(cp, topologies[i])
            else:
                df = calc.project_colvars([cp], [topologies[i]] if topologies else None)
            if df is None:
                continue
            os.makedirs(folder, exist_ok=True)
            df.to_csv(p, index=False, float_format="%.4f")
            paths.append(p)
        out[calc.cv_name] = paths
    return out


def _read_cv_traj(paths: List[str]) -> pd.DataFrame:
    data = []
    for i, p in enumerate(paths):
        df = pd.read_csv(p)
        df["traj_label"] = i
        data.append(df)
    return pd.concat(data, ignore_index=True)


def _extract_centroids(cv_data: pd.DataFrame, trajectories: List[str], topologies: List[str], folder: str) -> None:
    """<folder>/cluster_<label>.pdb for every row marked as a centroid: the topology with the positions of that frame, read
    on the host (one frame each), without bonds (reference traj_cluster_workflow.py:140-168, md.py extract_PDB)."""
    import dataclasses

    from . import trajectory

    logger.info("Extracting centroids from the trajectories...")
    for _, row in cv_data[cv_data["centroid"] == True].iterrows():   # noqa: E712 -- the column may hold objects
        i, frame, label = int(row["traj_label"]), int(row["frame"]), int(row["cluster"])
        top = trajectory.read_topology(topologies[i])
        traj = trajectory.open_trajectory(trajectories[i], top.n_atoms)
        if not 0 <= frame < traj.n_frames:
            raise ValueError(f"{trajectories[i]}: frame {frame} asked for, the trajectory has frames 0 to {traj.n_frames - 1}")
        os.makedirs(folder, exist_ok=True)
        logger.info(f"Extracting centroid for cluster {label} from trajectory {Path(trajectories[i]).name} at frame {frame}.")
        trajectory.write_topology(os.path.join(folder, f"cluster_{label}.pdb"),
                                  dataclasses.replace(top, positions=traj.frames(frame, frame + 1)[0], bonds=None))


def traj_cluster(configuration: Dict, cv_traj_paths: Union[str, List[str]], trajectories: Optional[List[str]] = None,
                 topologies: Optional[List[str]] = None, sup_cv_traj_paths: Optional[List[str]] = None,
                 sup_trajectories: Optional[List[str]] = None, sup_topologies: Optional[List[str]] = None,
                 frames_per_sample: Optional[int] = 1, output_folder: str = "traj_cluster", memory_budget: Optional[int] = None) -> Dict[str, List[str]]:
    """Cluster the CV trajectories (CSV in, CSV with cluster / centroid / frame columns out).  With `trajectories` and
    `topologies` (one PDB for all, or one per trajectory; .dcd / .npy, a GROMACS .xtc is imported first into
    <out>/xtc_import) and `output_structures` "centroids" or "all", <out>/centroids/cluster_<label>.pdb holds the frame of
    every centroid (the topology's atoms with that frame's positions, no CONECT records, as the reference strips them);
    with "all", <out>/<trajectory>/cluster_<label>.xtc holds the frames of every cluster of every trajectory in ascending
    order, HDBSCAN's noise label -1 included (reference traj_cluster_workflow.py:140-194), compressed on the device
    (trajectory.extract_frames) in chunks of at most `memory_budget` bytes.  The returned dictionary names the CSV files."""
    os.makedirs(output_folder, exist_ok=True)
    configuration = validate_configuration(configuration or {}, TrajClusterSchema, output_folder)
    if configuration["run"] is False:
        logger.info("traj_cluster workflow set to not run. Exiting...")
        return {}
    cv_traj_paths = _as_list(cv_traj_paths)
    trajectories, topologies = _as_list(trajectories), _as_list(topologies)
    extract = configuration["output_structures"] in ("centroids", "all") and bool(trajectories) and bool(topologies)
    if extract:
        topologies = _one_topology_each(trajectories, topologies)   # the count error below names the CV trajectories too
        if len(trajectories) != len(cv_traj_paths) or len(topologies) != len(trajectories):
            raise ValueError(f"traj_cluster: {len(trajectories)} trajectories and {len(topologies)} topologies for {len(cv_traj_paths)} "
                             "CV trajectories (one topology for all, or one per trajectory)")
        trajectories = _route_xtc(trajectories, output_folder, memory_budget)
    cv_data = _read_cv_traj(cv_traj_paths)
    cv_labels = cv_data.columns[:-1].tolist()
    labels, centroids = statistics.optimize_clustering(cv_data[cv_labels].to_numpy(), configuration)
    cv_data["cluster"] = labels
    cv_data = statistics.find_centroids(cv_data, centroids, cv_labels)
    frames = []
    for i in range(len(cv_traj_paths)):
        n = int((cv_data["traj_label"] == i).sum())
        frames.extend(np.arange(0, n * frames_per_sample, frames_per_sample))
    cv_data["frame"] = frames
    out: Dict[str, List[str]] = {}
    for i in range(len(cv_traj_paths)):
        name = Path(trajectories[i]).stem if trajectories else f"traj_{i}"
        folder = os.path.join(output_folder, name)
        os.makedirs(folder, exist_ok=True)
        p = os.path.join(folder, "projected_trajectory.csv")
        cv_data[cv_data["traj_label"] == i].to_csv(p, index=False)
        out[name] = [p]
    if configuration["output_structures"] in ("centroids", "all"):
        if extract:
            _extract_centroids(cv_data, trajectories, topologies, os.path.join(output_folder, "centroids"))
        else:
            logger.warning("Trajectory and/or topology files not provided. Skipping extraction of centroids from the trajectory.")
    if configuration["output_structures"] == "all":
        if extract:
            for i in range(len(cv_traj_paths)):
                rows = cv_data[cv_data["traj_label"] == i]
                for label in rows["cluster"].unique():
                    from . import trajectory

                    trajectory.extract_frames(trajectories[i], topologies[i], rows.loc[rows["cluster"] == label, "frame"].to_numpy(),
                                              os.path.join(output_folder, Path(trajectories[i]).stem, f"cluster_{int(label)}.xtc"), memory_budget)
        else:
            logger.warning("Trajectory and/or topology files not provided. Skipping extraction of cluster ensembles from the trajectory.")
    if sup_cv_traj_paths:
        sup = _read_cv_traj(_as_list(sup_cv_traj_paths))
        if sup.shape[1] - 1 != len(cv_labels):
            logger.error("Dimensionality of supplementary collective variable data does not match the original data. Exiting...")
            sys.exit(1)
        sup["cluster"] = statistics.assign_closest_cluster(cv_data[cv_labels].to_numpy(), cv_data["cluster"].to_numpy(),
                                                           sup[cv_labels].to_numpy())
        for i in range(len(sup_cv_traj_paths)):
            name = f"sup_{Path(sup_trajectories[i]).stem}" if sup_trajectories else f"sup_traj_{i}"
            folder = os.path.join(output_folder, name)
            os.makedirs(folder, exist_ok=True)
            p = os.path.join(folder, "projected_trajectory.csv")
            sup[sup["traj_label"] == i].to_csv(p, index=False)
            out[name] = [p]
    return out
