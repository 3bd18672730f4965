"""NumPy restatement of what hip.core_distances / hip.mr_mst reproduce (test helper, no GPU): the core distances of
NearestNeighbors(algorithm="kd_tree").kneighbors and Prim's scan of sklearn's mst_from_data_matrix (Euclidean,
alpha = 1).  Also the seeded point sets of tests/golden/hdbscan_golden.npz, which stores a digest rather than the
points."""
import numpy as np

from tests import linkage_oracle as lo

KS = (1, 3, 16)   # min_samples stored in the fixture


def _cont2d(rng):
    c = rng.uniform(-0.8, 0.8, (5, 2))
    return c[rng.integers(0, 5, 700)] + 0.09 * rng.standard_normal((700, 2))   # continuous: nothing rounded


def _mix16d(rng):
    c = rng.uniform(-0.8, 0.8, (4, 16))
    return np.round(c[rng.integers(0, 4, 300)] + 0.1 * rng.standard_normal((300, 16)), 4)


_OWN = {"cont2d_700": (21, _cont2d), "mix16d_300": (22, _mix16d)}
POINT_SETS = ("mix2d_3k", "mix4d_3k", "lattice", "dups", "cont2d_700", "mix16d_300")

digest = lo.digest


def points(name):
    if name in _OWN:
        seed, build = _OWN[name]
        return np.ascontiguousarray(build(np.random.Generator(np.random.PCG64(seed))), dtype=np.float64)
    return lo.points(name)


def fresh_points(n, d):
    """Seeded sets for the shape sweeps: 4 decimals, three shifted copies, so tied distances are the normal case."""
    rng = np.random.Generator(np.random.PCG64(7000 * n + d))
    return np.round(rng.uniform(-1, 1, (n, d)) + (rng.integers(0, 3, (n, 1)) - 1) * 0.5, 4)


def _sq_sums(P, rows):
    """sum_c (P[i][c] - P[j][c])^2 for i in rows and every j, the squares added one coordinate after the other."""
    acc = np.zeros((len(rows), len(P)))
    for c in range(P.shape[1]):
        diff = P[rows, None, c] - P[None, :, c]
        acc += diff * diff
    return acc


def core_distances(P, k):
    """The k-th smallest distance from every point to all points, itself included: the sqrt of the k-th smallest
    squared sum (sqrt is monotone; the k-th value does not depend on how ties are ordered)."""
    n = len(P)
    out = np.empty(n)
    for r in range(0, n, 512):
        rows = np.arange(r, min(r + 512, n))
        out[rows] = np.sqrt(np.partition(_sq_sums(P, rows), k - 1, axis=1)[:, k - 1])
    return out


def prim(P, core):
    """mst_from_data_matrix: (src, dst, w) of the n - 1 edges in Prim order from node 0."""
    n = len(P)
    in_tree = np.zeros(n, dtype=bool)
    min_reach = np.full(n, np.inf)
    source = np.ones(n, dtype=np.int64)
    src, dst, w = np.empty(n - 1, dtype=np.int64), np.empty(n - 1, dtype=np.int64), np.empty(n - 1)
    cur = 0
    for i in range(n - 1):
        in_tree[cur] = True
        dist = np.sqrt(_sq_sums(P, np.array([cur]))[0])
        m = np.maximum(np.maximum(core[cur], core), dist)
        upd = ~in_tree & (m < min_reach)   # strict: an equal value keeps the older source
        min_reach[upd] = m[upd]
        source[upd] = cur
        cand = np.where(in_tree, np.inf, min_reach)
        new = int(np.argmin(cand))   # the first index of the minimum: scikit-learn scans upwards with a strict '<'
        assert cand[new] < np.finfo(np.float64).max
        src[i], dst[i], w[i] = source[new], new, cand[new]
        cur = new
    return src, dst, w
