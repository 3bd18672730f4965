"""Generate tests/golden/compute_features_golden.npz from the reference's OWN compute_features test data.

Run in the build container only (it reads /root/reference, which never travels):

    python tests/golden/make_golden_compute_features.py

What is stored is *data*, never reference source:

* ``dcd``        the bytes of tests/data/input/trajectory/CA_example.dcd (164 frames, 104 CA atoms);
* ``pdb``        the text of tests/data/input/topology/CA_example.pdb;
* ``distances`` / ``distance_names``  the 164 x 1078 float32 matrix of the PLUMED-produced
                 tests/data/reference/compute_features/distances.dat (every feature column, in file order) and its
                 column names;
* ``schema_defaults``  JSON of model_dump() of the reference's ComputeFeaturesSchema.

The PLUMED-produced virtual_dihedrals.dat of the same trajectory is already in filter_golden.npz (``X``, ``names``).
"""
import json
import os
import sys

import numpy as np
import pandas as pd

REF = "/root/reference"
DATA = os.path.join(REF, "deep_cartograph", "tests", "data")
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    with open(os.path.join(DATA, "input", "trajectory", "CA_example.dcd"), "rb") as f:
        dcd = np.frombuffer(f.read(), dtype=np.uint8)
    with open(os.path.join(DATA, "input", "topology", "CA_example.pdb")) as f:
        pdb = f.read()
    colvars = os.path.join(DATA, "reference", "compute_features", "distances.dat")
    with open(colvars) as f:
        columns = f.readline().split()[2:]
    df = pd.read_csv(colvars, sep=r"\s+", dtype=np.float32, comment="#", header=None, names=columns)
    names = [c for c in columns if c != "time"]
    X = np.ascontiguousarray(df[names].to_numpy(dtype=np.float32))
    assert X.shape == (164, 1078), X.shape

    sys.path.insert(0, REF)
    from deep_cartograph.yaml_schemas.compute_features import ComputeFeaturesSchema

    path = os.path.join(OUT, "compute_features_golden.npz")
    np.savez_compressed(path, dcd=dcd, pdb=np.array(pdb), distances=X, distance_names=np.array(names),
                        schema_defaults=np.array(json.dumps(ComputeFeaturesSchema().model_dump())))
    print("compute_features_golden.npz:", X.shape, dcd.size, "DCD bytes,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
