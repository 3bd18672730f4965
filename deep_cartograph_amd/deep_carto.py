"""`deep_carto`-style entry point for the accelerated part of the workflow:
(analyze_geometry) -> (traj_augmentation) -> (compute_features) -> (filter_features) -> train_colvars -> (traj_projection of supplementary data) -> traj_cluster,
starting from trajectories (.dcd / .npy coordinates, or GROMACS .xtc files that are decoded first into <out>/xtc_import, plus a PDB topology: distances and virtual dihedrals are computed
on the device) or from pre-computed feature matrices (PLUMED COLVAR text or the binary .npy fast path).
With trajectories and an `analyze_geometry` section in the YAML, RMSD / RMSF / dRMSD are computed first (on the device,
geometry.py) into <out>/analyze_geometry.  With seed trajectories (-seed_traj / -seed_top: a short morph between two
states, for instance) the reference's augmentation step (deep_carto.py:202-215) runs next, on the device
(augmentation.py), into <out>/traj_augmentation with the `traj_augmentation` section of the YAML, and the augmented
trajectories join the training trajectories; seeds alone, without -traj, are allowed, as in the reference.  The
reference's PLUMED featurisation is replaced by `compute_features` for the feature kinds trajectory.py documents.
The YAML keeps the reference's `traj_augmentation` / `compute_features` / `filter_features` / `train_colvars` /
`traj_cluster` sections.
Feature filtering needs only the feature matrices: it runs when the YAML has a `filter_features` section and no
-features file is given.

    python -m deep_cartograph_amd.deep_carto -conf config.yml -traj a.dcd b.dcd -top a.pdb -out run1 \
           [-seed_traj morph.dcd -seed_top morph.pdb] [-sup_traj c.dcd] [-dim 2] [-cvs pca tica deep_tica] [-features feats.txt] [-restart]
    python -m deep_cartograph_amd.deep_carto -conf config.yml -colvars a.dat b.dat -out run1 [-sup_colvars c.dat] ...
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
import time
from typing import Dict, List, Optional

from . import xtc
from .common import get_unique_path, read_configuration, read_features_list
from .tools import analyze_geometry, compute_features, filter_features, traj_augmentation, traj_cluster, traj_projection, train_colvars

logger = logging.getLogger("deep_cartograph")


def deep_cartograph(configuration: Dict, colvars_paths: List[str], sup_colvars_paths: Optional[List[str]] = None,
                    features_list: Optional[List[str]] = None, dimension: Optional[int] = None, cvs: Optional[List[str]] = None,
                    restart: bool = False, output_folder: Optional[str] = None, trajectory_data: Optional[List[str]] = None,
                    topology_data: Optional[List[str]] = None, sup_trajectory_data: Optional[List[str]] = None,
                    seed_trajectory_data: Optional[List[str]] = None, seed_topology_data: Optional[List[str]] = None) -> Dict[str, Dict]:
    """(analyze_geometry) -> (compute_features) -> (filter_features) -> train_colvars -> traj_projection (supplementary
    colvars) -> traj_cluster per CV (reference deep_carto.py:292-361).  With `trajectory_data` and an `analyze_geometry`
    section in the configuration that tool runs first, into <out>/analyze_geometry.  With `trajectory_data` (and `topology_data`: one PDB for all, or one per
    trajectory) the `compute_features` section runs first and its outputs become `colvars_paths`; `sup_trajectory_data`
    likewise become `sup_colvars_paths`, always with the FIRST topology.  Giving both is an error.  A `filter_features` section in the configuration selects
    the features first unless `features_list` is given.  `restart` reuses the output folder and skips what exists.
    With `seed_trajectory_data` (and `seed_topology_data`: one PDB for all, or one per seed) the `traj_augmentation`
    section runs after analyze_geometry, into <out>/traj_augmentation, and its trajectories and topologies are appended
    to the ones `compute_features` reads (reference deep_carto.py:202-215); `trajectory_data` may then be empty.
    A run that started from trajectories hands them, their topologies and `compute_features.plumed_settings.traj_stride`
    on to `traj_cluster`, which then leaves `traj_cluster/<cv>/centroids/cluster_<k>.pdb` and, with
    `traj_cluster: {output_structures: all}`, `traj_cluster/<cv>/<trajectory>/cluster_<k>.xtc` (reference :350-360)."""
    t0 = time.time()
    output_folder = output_folder or "deep_cartograph"
    if not restart:
        output_folder = get_unique_path(output_folder)
    os.makedirs(output_folder, exist_ok=True)
    # GROMACS .xtc inputs are decoded once, into <out>/xtc_import, and every step below reads the .dcd (xtc.py)
    trajectory_data, sup_trajectory_data, seed_trajectory_data = (xtc.route(t, output_folder) for t in
                                                                  (trajectory_data, sup_trajectory_data, seed_trajectory_data))
    trajectory_names = None
    if trajectory_data and colvars_paths:
        raise ValueError("give either colvars_paths or trajectory_data, not both: the computed features would replace the given ones")
    as_list = lambda x: [x] if isinstance(x, str) else list(x or [])
    seed_trajectory_data = as_list(seed_trajectory_data)
    if seed_trajectory_data and colvars_paths:
        raise ValueError("give either colvars_paths or seed_trajectory_data, not both: the computed features would replace the given ones")
    if seed_trajectory_data and not seed_topology_data:
        raise ValueError("seed_trajectory_data needs seed_topology_data (a PDB file)")
    if trajectory_data or seed_trajectory_data:
        trajectory_data = as_list(trajectory_data)
        if trajectory_data and not topology_data:
            raise ValueError("trajectory_data needs topology_data (a PDB file)")
        topology_data = as_list(topology_data)
        sup_trajectory_data = [sup_trajectory_data] if isinstance(sup_trajectory_data, str) else sup_trajectory_data
        if "analyze_geometry" in configuration and trajectory_data:
            analyze_geometry(configuration=configuration["analyze_geometry"] or {}, trajectories=trajectory_data, topologies=topology_data,
                             output_folder=os.path.join(output_folder, "analyze_geometry"))
        if seed_trajectory_data:
            augmented_trajs, augmented_tops = traj_augmentation(configuration=configuration.get("traj_augmentation") or {},
                                                                trajectories=seed_trajectory_data, topologies=as_list(seed_topology_data),
                                                                output_folder=os.path.join(output_folder, "traj_augmentation"))
            if len(topology_data) == 1:   # one topology for all: spell it out, the augmented ones follow
                topology_data = topology_data * len(trajectory_data)
            trajectory_data, topology_data = trajectory_data + augmented_trajs, topology_data + augmented_tops
        cf = configuration.get("compute_features") or {}
        colvars_paths = compute_features(configuration=cf, trajectory_data=trajectory_data, topology_data=topology_data,
                                         output_folder=os.path.join(output_folder, "compute_features"))
        trajectory_names = [os.path.basename(os.path.dirname(p)) for p in colvars_paths]
        if sup_trajectory_data:
            sup_colvars_paths = compute_features(configuration=cf, trajectory_data=sup_trajectory_data, topology_data=topology_data[:1],
                                                 output_folder=os.path.join(output_folder, "compute_features_sup"))
    elif sup_trajectory_data:
        raise ValueError("sup_trajectory_data needs trajectory_data: supplementary features must be the training features")
    if "filter_features" in configuration and not features_list:
        features_path = filter_features(configuration=configuration["filter_features"] or {}, colvars_paths=colvars_paths,
                                        output_folder=os.path.join(output_folder, "filter_features"))
        features_list = read_features_list(features_path)
    tc_out = os.path.join(output_folder, "train_colvars")
    cv_paths = train_colvars(configuration=configuration.get("train_colvars", {}), train_colvars_paths=colvars_paths,
                             trajectory_names=trajectory_names, features_list=features_list, dimension=dimension, cvs=cvs,
                             output_folder=tc_out)
    sup_paths: Dict[str, List[str]] = {}
    if sup_colvars_paths:
        models = [os.path.join(tc_out, cv, "model.zip") for cv in cv_paths]
        sup_names = [os.path.basename(os.path.dirname(p)) for p in sup_colvars_paths] if sup_trajectory_data else None
        sup_paths = traj_projection(configuration=configuration.get("traj_projection", {}), colvars_paths=sup_colvars_paths,
                                    trajectory_names=sup_names, model_paths=models,
                                    output_folder=os.path.join(output_folder, "traj_projection"))
    clusters = {}
    for cv, paths in cv_paths.items():
        # started from trajectories: traj_cluster extracts the centroid structures and the cluster ensembles from them
        # (reference deep_carto.py:350-360); a sample of the CV trajectory is every traj_stride-th frame
        from_trajectories = dict(trajectories=trajectory_data, topologies=topology_data, frames_per_sample=int(
            ((configuration.get("compute_features") or {}).get("plumed_settings") or {}).get("traj_stride", 1))) if trajectory_data else {}
        clusters[cv] = traj_cluster(configuration=configuration.get("traj_cluster", {}), cv_traj_paths=paths,
                                    sup_cv_traj_paths=sup_paths.get(cv), output_folder=os.path.join(output_folder, "traj_cluster", cv),
                                    **from_trajectories)
    logger.info("Total elapsed time: %s", time.strftime("%H h %M min %S s", time.gmtime(time.time() - t0)))
    return {"train_colvars": cv_paths, "traj_projection": sup_paths, "traj_cluster": clusters}


def main(argv=None):
    p = argparse.ArgumentParser("deep_carto (MI355X CV-fit path)")
    p.add_argument("-conf", "-configuration", dest="configuration_path", required=True, help="YAML configuration")
    p.add_argument("-colvars", dest="colvars", nargs="+", default=None, help="training feature matrices (COLVAR text or .npy)")
    p.add_argument("-traj", "-traj_data", dest="traj", nargs="+", default=None, help="training trajectories (.dcd / .npy; a GROMACS .xtc is imported first, into <out>/xtc_import); replaces -colvars")
    p.add_argument("-top", "-top_data", dest="top", nargs="+", default=None, help="topology (.pdb): one for all -traj files, or one per -traj file in the same order")
    p.add_argument("-seed_traj", "-seed_traj_data", dest="seed_traj", nargs="+", default=None, help="seed trajectories (.dcd / .npy / .xtc) to augment by interpolation; the augmented trajectories join the training trajectories")
    p.add_argument("-seed_top", "-seed_top_data", dest="seed_top", nargs="+", default=None, help="topology (.pdb) of the seed trajectories: one for all, or one per -seed_traj file")
    p.add_argument("-sup_traj", "-sup_traj_data", dest="sup_traj", nargs="*", default=None, help="supplementary trajectories to project; they are read with the first -top file")
    p.add_argument("-sup_colvars", dest="sup_colvars", nargs="*", default=None, help="supplementary feature matrices to project")
    p.add_argument("-features", dest="features_path", default=None, help="file with the feature names to use (one per line)")
    p.add_argument("-dim", "-dimension", dest="dimension", type=int, default=None)
    p.add_argument("-cvs", nargs="+", default=None)
    p.add_argument("-restart", action="store_true")
    p.add_argument("-out", "-output", dest="output_folder", default=None)
    p.add_argument("-v", "-verbose", dest="verbose", action="store_true")
    a = p.parse_args(argv)
    if not a.traj and not a.colvars and not a.seed_traj:
        p.error("one of -colvars or -traj is required (or seed trajectories alone: -seed_traj with -seed_top)")
    if a.seed_traj and not a.seed_top:
        p.error("-seed_traj needs -seed_top")
    if a.traj and not a.top:
        p.error("-traj needs -top")
    logging.basicConfig(level=logging.DEBUG if a.verbose else logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    cfg = read_configuration(a.configuration_path)
    deep_cartograph(cfg, a.colvars or [], a.sup_colvars, read_features_list(a.features_path), a.dimension, a.cvs, a.restart, a.output_folder,
                    trajectory_data=a.traj, topology_data=a.top, sup_trajectory_data=a.sup_traj,
                    seed_trajectory_data=a.seed_traj, seed_topology_data=a.seed_top)


if __name__ == "__main__":
    main(sys.argv[1:])
