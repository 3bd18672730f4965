"""Generate tests/golden/filter_golden.npz from the reference's OWN filter_features test data.

Run in the build container only (it reads /root/reference, which never travels):

    python tests/golden/make_golden_filter.py

What is stored is *data*, never reference source:

* ``X``          the 164 x 202 float32 matrix of tests/data/reference/compute_features/virtual_dihedrals.dat
                 (every feature column, in file order) and ``names``, its column names: the same set as
                 reference/filter_features/all_virtual_dihedrals.txt, which lists them in another order;
* ``filtered``   reference/filter_features/filtered_virtual_dihedrals.txt, in order;
* ``summary_names`` / ``summary_pass`` / ``summary_hdtp``  the columns of
                 reference/filter_features/virtual_dihedral_filtering_summary.csv (in that file's order);
* ``schema_defaults``  JSON of model_dump() of the reference's FilterFeaturesSchema.
"""
import json
import os
import sys

import numpy as np
import pandas as pd

REF = "/root/reference"
DATA = os.path.join(REF, "deep_cartograph", "tests", "data", "reference")
OUT = os.path.dirname(os.path.abspath(__file__))


def read_list(path):
    with open(path) as f:
        return [line.strip() for line in f if line.strip()]


def main():
    colvars = os.path.join(DATA, "compute_features", "virtual_dihedrals.dat")
    with open(colvars) as f:
        columns = f.readline().split()[2:]
    df = pd.read_csv(colvars, sep=r"\s+", dtype=np.float32, comment="#", header=None, names=columns)
    names = [c for c in columns if c != "time"]
    all_features = read_list(os.path.join(DATA, "filter_features", "all_virtual_dihedrals.txt"))
    assert sorted(names) == sorted(all_features), "the colvars columns are not the reference's all-features list"
    X = np.ascontiguousarray(df[names].to_numpy(dtype=np.float32))
    assert X.shape == (164, 202), X.shape
    filtered = read_list(os.path.join(DATA, "filter_features", "filtered_virtual_dihedrals.txt"))
    summary = pd.read_csv(os.path.join(DATA, "filter_features", "virtual_dihedral_filtering_summary.csv"))
    assert list(summary.columns) == ["name", "pass", "hdtp"]

    sys.path.insert(0, REF)
    from deep_cartograph.yaml_schemas.filter_features import FilterFeaturesSchema

    np.savez_compressed(
        os.path.join(OUT, "filter_golden.npz"),
        X=X, names=np.array(names), filtered=np.array(filtered),
        summary_names=np.array(summary["name"].tolist()), summary_pass=summary["pass"].to_numpy(dtype=bool),
        summary_hdtp=summary["hdtp"].to_numpy(dtype=np.float64),
        schema_defaults=np.array(json.dumps(FilterFeaturesSchema().model_dump())))
    print("filter_golden.npz:", X.shape, len(filtered), "filtered")


if __name__ == "__main__":
    main()
