"""Generate tests/golden/xtc_golden.npz from the reference's OWN GROMACS trajectories.

Run in the build container only (it reads /root/reference, which never travels):

    python tests/golden/make_golden_xtc.py

What is stored is *data*, never reference source:

* ``aladip_xtc``   the bytes of the first 200 frames of data/alanine_dipeptide/input/300K/trajectory.xtc (22 atoms);
* ``aladip_phi_psi``  the matching 200 rows (time, phi, psi) of the phi_psi.dat PLUMED wrote next to it;
* ``aladip_pdb``   the text of data/alanine_dipeptide/input/topology.pdb;
* ``protein_xtc``  the bytes of the first 24 frames of the traj_augmentation notebook's 457-C-alpha trajectory;
* ``protein_pdb``  the text of its .pdb (a topology, not frame 0).

It also prints the worst deviation of the torsions of the oracle's decode (tests/xtc_oracle.py) from PLUMED's rows: 1.5
times that is the bound of tests/test_xtc_cpu.py::test_torsions_against_plumed.
"""
import os
import sys

import numpy as np

REF = "/root/reference"
ALADIP = os.path.join(REF, "deep_cartograph", "data", "alanine_dipeptide", "input")
NOTEBOOK = os.path.join(REF, "examples", "notebooks", "6.traj_augmentation", "traj_augmentation_output")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))


def head(path, n_frames):
    """The bytes of the first ``n_frames`` frames of an XTC file."""
    from tests import xtc_oracle as xo

    with open(path, "rb") as f:
        data = f.read()
    frames = xo.frames(data)
    last = frames[n_frames - 1]
    return np.frombuffer(data[:last["offset"] + (last["nbytes"] + 3) // 4 * 4], dtype=np.uint8)


def main():
    from tests import test_xtc_cpu as tx
    from tests import xtc_oracle as xo

    aladip = head(os.path.join(ALADIP, "300K", "trajectory.xtc"), 200)
    phi_psi = np.loadtxt(os.path.join(ALADIP, "300K", "phi_psi.dat"), comments="#", dtype=np.float64)[:200]
    with open(os.path.join(ALADIP, "topology.pdb")) as f:
        aladip_pdb = f.read()
    protein = head(os.path.join(NOTEBOOK, "GOdMD_6IRS_7DSQ_augmented_pchip.xtc"), 24)
    with open(os.path.join(NOTEBOOK, "GOdMD_6IRS_7DSQ_augmented_pchip.pdb")) as f:
        protein_pdb = f.read()
    assert phi_psi.shape == (200, 3) and protein.size == 49824, (phi_psi.shape, protein.size)
    path = os.path.join(OUT, "xtc_golden.npz")
    np.savez_compressed(path, aladip_xtc=aladip, aladip_phi_psi=phi_psi, aladip_pdb=np.array(aladip_pdb), protein_xtc=protein,
                        protein_pdb=np.array(protein_pdb))
    print("xtc_golden.npz:", aladip.size, "+", protein.size, "XTC bytes,", os.path.getsize(path), "bytes")
    _, xyz, status = xo.decode(aladip.tobytes())
    assert not status.any()
    dev = tx.torsion_deviation(xyz, aladip_pdb, phi_psi)
    print("worst torsion deviation of the oracle's decode from PLUMED over 200 frames: %.6f rad (bound: 1.5 x = %.6f)" % (dev, 1.5 * dev))


if __name__ == "__main__":
    main()
