"""Generate tests/golden/hdbscan_golden.npz: HDBSCAN's core distances and mutual-reachability minimum spanning trees
on the seeded point sets of tests/hdbscan_oracle.py.  Runs on the CPU:

    python tests/golden/make_golden_hdbscan.py

Per point set <s> (the points are rebuilt from their seed; ``<s>.digest`` is the SHA-256 of their float64 bytes) and
per min_samples <k> in 1, 3, 16:

* ``<s>.k<k>.core``                    the core distances (float64);
* ``<s>.k<k>.src`` / ``.dst`` / ``.w``   the edges of the MST IN PRIM ORDER (int32, int32, float64).

These are platform independent.  Labels are NOT stored: they depend on the default argsort of the numpy build when
edge weights tie, which they do in every set.

Before anything is written the NumPy restatement (tests/hdbscan_oracle.py) is asserted equal, bit for bit, to the
live scikit-learn internals it restates: NearestNeighbors(algorithm="kd_tree").kneighbors and
sklearn.cluster._hdbscan._linkage.mst_from_data_matrix.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    from sklearn.cluster._hdbscan._linkage import mst_from_data_matrix
    from sklearn.metrics import DistanceMetric
    from sklearn.neighbors import NearestNeighbors

    from tests import hdbscan_oracle as ho

    g = {}
    for name in ho.POINT_SETS:
        P = ho.points(name)
        g[f"{name}.digest"] = np.array(ho.digest(P))
        for k in ho.KS:
            core = ho.core_distances(P, k)
            live = NearestNeighbors(n_neighbors=k, algorithm="kd_tree", leaf_size=40, metric="euclidean").fit(P).kneighbors(P, k)[0][:, -1]
            assert np.array_equal(core, live), (name, k, "core distances")
            src, dst, w = ho.prim(P, core)
            mst = mst_from_data_matrix(P, np.ascontiguousarray(live), DistanceMetric.get_metric("euclidean"), 1.0)
            assert np.array_equal(src, mst["current_node"]) and np.array_equal(dst, mst["next_node"]), (name, k, "MST nodes")
            assert np.array_equal(w, mst["distance"]), (name, k, "MST weights")
            ties = len(w) - len(np.unique(w))
            print(f"{name:12s} k={k:2d}  n={len(P):5d}  tied edge weights {ties}")
            g[f"{name}.k{k}.core"] = core
            g[f"{name}.k{k}.src"] = src.astype(np.int32)
            g[f"{name}.k{k}.dst"] = dst.astype(np.int32)
            g[f"{name}.k{k}.w"] = w
    path = os.path.join(OUT, "hdbscan_golden.npz")
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
