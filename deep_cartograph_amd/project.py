"""Command line of tools.traj_projection on trajectories: every saved model projects every trajectory straight from
its coordinates (CVCalculator.project_trajectory) -- no colvars file, no features configuration; the model's own
feature names and the topology say which atoms to read.

    python -m deep_cartograph_amd.project -traj a.dcd b.dcd -top a.pdb [b.pdb] -model pca/model.zip [tica/model.zip ...] \
           [-out traj_projection] [-v]

Writes <out>/<cv>/<trajectory stem>/projected_trajectory.csv (%.4f); an existing file is kept.
"""
from __future__ import annotations

import argparse
import logging
import sys


def main(argv=None):
    from .tools import traj_projection

    p = argparse.ArgumentParser("Deep Cartograph: Project Trajectories (MI355X)",
                                description="Projects trajectories onto saved collective-variable models from their coordinates.")
    p.add_argument("-traj", dest="trajectories", required=True, nargs="+", help="trajectories to project (.dcd / .npy; a GROMACS .xtc is imported first)")
    p.add_argument("-top", dest="topologies", required=True, nargs="+", help="topology (.pdb): one for all, or one per trajectory")
    p.add_argument("-model", dest="model_paths", required=True, nargs="+", help="model.zip files written by train_colvars")
    p.add_argument("-out", dest="output_folder", type=str, default=None, help="Path to the output folder.")
    p.add_argument("-v", "--verbose", dest="verbose", action="store_true", default=False)
    a = p.parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if a.verbose else logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    traj_projection({}, None, topologies=a.topologies, model_paths=a.model_paths, output_folder=a.output_folder or "traj_projection",
                    trajectories=a.trajectories)


if __name__ == "__main__":
    main(sys.argv[1:])
