"""Generate tests/golden/linkage_golden.npz: scipy's linkage matrices and the reference's hierarchical labels on
the seeded point sets of tests/linkage_oracle.py.

Needs a checkout of the reference package (it is imported, never copied) and runs on the CPU:

    python tests/golden/make_golden_linkage.py <path to the reference checkout>

What is stored is *data*, never reference source.  Per point set <s> (the points themselves are rebuilt from their
seed; ``<s>.digest`` is the SHA-256 of their float64 bytes) and per method <m> in complete / average / ward:

* ``<s>.<m>.children`` / ``.heights`` / ``.sizes``   the columns of scipy.cluster.hierarchy.linkage(P, m, "euclidean");
* ``<s>.<m>.labels``    3 x n: the labels of the reference's statistics.cluster_data (hierarchical, linkage m) at
                        k = 3, 6, 10; ``<s>.<m>.centroids_k6`` its centroids at k = 6;
* ``<s>.opt_labels`` / ``<s>.opt_centroids``   statistics.optimize_clustering with the schema defaults.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DCV_REFERENCE")
    if not ref:
        sys.exit(__doc__)
    sys.path.insert(0, ref)
    from deep_cartograph.modules.statistics import statistics as ref_stats
    from deep_cartograph.yaml_schemas.traj_cluster import TrajClusterSchema
    from scipy.cluster import hierarchy

    from tests import linkage_oracle as lo

    g = {}
    for name in lo.POINT_SETS:
        P = lo.points(name)
        n = len(P)
        g[f"{name}.digest"] = np.array(lo.digest(P))
        for m in lo.METHODS:
            Z = hierarchy.linkage(P, method=m, metric="euclidean")
            assert np.array_equal(Z[:, :2], Z[:, :2].astype(np.int32)) and np.array_equal(Z[:, 3], Z[:, 3].astype(np.int32))
            g[f"{name}.{m}.children"] = Z[:, :2].astype(np.int32)
            g[f"{name}.{m}.heights"] = Z[:, 2].copy()
            g[f"{name}.{m}.sizes"] = Z[:, 3].astype(np.int32)
            labels = []
            for k in lo.CUTS:
                lab, cen = ref_stats.cluster_data(P.copy(), {"algorithm": "hierarchical", "linkage": m, "num_clusters": k})
                labels.append(lab.astype(np.int8))
                if k == 6:
                    g[f"{name}.{m}.centroids_k6"] = cen
            g[f"{name}.{m}.labels"] = np.stack(labels)
            ties = n - 1 - len(np.unique(Z[:, 2]))
            print(name, m, "n", n, "tied heights", ties, flush=True)
        lab, cen = ref_stats.optimize_clustering(P.copy(), TrajClusterSchema().model_dump())
        g[f"{name}.opt_labels"] = lab.astype(np.int8)
        g[f"{name}.opt_centroids"] = cen
        print(name, "optimize_clustering: k =", len(cen), flush=True)
    path = os.path.join(OUT, "linkage_golden.npz")
    np.savez_compressed(path, **g)
    print("linkage_golden.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
