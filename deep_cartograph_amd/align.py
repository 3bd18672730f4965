"""Command line of tools.align_trajectories: every trajectory superposed onto a reference topology on the C-alpha atoms
of the residues common to all topologies, all atoms written.  The reference's arguments
(tools/align_trajectories/align_trajectories.py:242-293); like the reference's, the tool is not part of deep_carto.

    python -m deep_cartograph_amd.align -traj_data a.dcd b.dcd -top_data a.pdb b.pdb [-ref_top ref.pdb] \
           [-output align_trajectories] [-v]
"""
from __future__ import annotations

import argparse
import logging
import sys


def main(argv=None):
    from .tools import align_trajectories

    p = argparse.ArgumentParser("Deep Cartograph: Align Trajectories (MI355X)",
                                description="Aligns trajectories and topologies to a reference topology.")
    p.add_argument("-traj_data", dest="trajectory_data", required=True, nargs="+", help="trajectories to align (.dcd / .npy; a GROMACS .xtc is imported first)")
    p.add_argument("-top_data", dest="topology_data", required=True, nargs="+", help="topology (.pdb): one for all, or one per trajectory")
    p.add_argument("-ref_top", dest="reference_topology", type=str, default=None,
                   help="reference topology (.pdb); defaults to the first topology of -top_data")
    p.add_argument("-output", dest="output_folder", type=str, default=None, help="Path to the output folder.")
    p.add_argument("-v", "--verbose", dest="verbose", action="store_true", default=False)
    a = p.parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if a.verbose else logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    align_trajectories(a.trajectory_data, a.topology_data, ref_topology=a.reference_topology,
                       output_folder=a.output_folder or "align_trajectories")


if __name__ == "__main__":
    main(sys.argv[1:])
