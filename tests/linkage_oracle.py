"""NumPy restatement of what hip.linkage / statistics.cut_tree reproduce (test helper, no GPU): the nearest-neighbour
chain of scipy.cluster.hierarchy.linkage for complete / average / ward over Euclidean distances, scipy's sort and
relabelling of the merges, and scikit-learn's cut of the tree.  Also the seeded point sets of
tests/golden/linkage_golden.npz, which stores their seeds and a digest rather than the points."""
import hashlib
import heapq

import numpy as np

METHODS = ("complete", "average", "ward")
CUTS = (3, 6, 10)


# ------------------------------------------------------------------------------------------------ point sets
def _mixture(rng, n, d, centres=6, spread=0.07):
    c = rng.uniform(-0.8, 0.8, (centres, d))
    P = c[rng.integers(0, centres, n)] + spread * rng.standard_normal((n, d))
    return np.round(np.clip(P, -1, 1), 4)   # 4 decimals: what survives the CSV between traj_projection and traj_cluster


# name -> (seed, builder)
POINT_SETS = {
    "mix2d_3k": (11, lambda rng: _mixture(rng, 3000, 2)),
    "mix4d_3k": (12, lambda rng: _mixture(rng, 3000, 4)),
    "mix2d_8k": (13, lambda rng: _mixture(rng, 8000, 2)),
    "mix4d_8k": (14, lambda rng: _mixture(rng, 8000, 4)),
    "lattice": (15, lambda rng: np.round(rng.uniform(-1, 1, (500, 2)), 2)),      # coarse: many tied heights
    "dups": (16, lambda rng: np.round(rng.uniform(-1, 1, (300, 2)), 1)),         # duplicate points: zero distances
}


def points(name):
    seed, build = POINT_SETS[name]
    return np.ascontiguousarray(build(np.random.Generator(np.random.PCG64(seed))), dtype=np.float64)


def digest(P):
    return hashlib.sha256(np.ascontiguousarray(P, dtype=np.float64).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ the chain
def pdist_square(P):
    """D[i][j] = sqrt(sum_c (P[i][c] - P[j][c])^2), the squares added one coordinate after the other."""
    n, d = P.shape
    D = np.empty((n, n))
    for r in range(0, n, 1024):
        acc = np.zeros((min(1024, n - r), n))
        for c in range(d):
            diff = P[r:r + 1024, None, c] - P[None, :, c]
            acc += diff * diff
        D[r:r + 1024] = np.sqrt(acc)
    return D


def nn_chain(P, method):
    """scipy's linkage matrix Z ((n - 1) x 4) for `method`, and the number of row searches the chain ran."""
    n = P.shape[0]
    D = pdist_square(P)
    size = np.ones(n, dtype=np.int64)
    Z = np.zeros((n - 1, 4))
    chain, searches, cursor = [], 0, 0
    for k in range(n - 1):
        if not chain:
            while size[cursor] == 0:
                cursor += 1
            chain.append(cursor)
        while True:
            x = chain[-1]
            row = np.where(size > 0, D[x], np.inf)
            row[x] = np.inf
            searches += 1
            i = int(np.argmin(row))   # the first index of the minimum: scipy scans upwards with a strict '<'
            if len(chain) > 1 and not row[i] < D[x, chain[-2]]:
                y = chain[-2]         # the previous element wins unless something is strictly closer
                break
            chain.append(i)
        h = D[x, y]
        chain.pop()
        chain.pop()
        if x > y:
            x, y = y, x
        nx, ny = int(size[x]), int(size[y])
        Z[k] = x, y, h, nx + ny
        size[x] = 0
        size[y] = nx + ny
        if method == "complete":
            new = np.maximum(D[x], D[y])
        elif method == "average":
            new = (nx * D[x] + ny * D[y]) / (nx + ny)
        else:
            ni = size.astype(np.float64)
            t = 1.0 / (nx + ny + ni)
            with np.errstate(invalid="ignore"):
                new = np.sqrt((ni + nx) * t * D[x] * D[x] + (ni + ny) * t * D[y] * D[y] - ni * t * h * h)
        live = size > 0
        live[y] = False
        D[y, live] = new[live]
        D[live, y] = new[live]
    # scipy: stable sort by height, then name the i-th sorted merge n + i (union-find), smaller id first
    Z = Z[np.argsort(Z[:, 2], kind="mergesort")]
    parent = list(range(2 * n - 1))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i in range(n - 1):
        a, b = find(int(Z[i, 0])), find(int(Z[i, 1]))
        Z[i, 0], Z[i, 1] = min(a, b), max(a, b)
        parent[a] = parent[b] = n + i
    return Z, searches


def hc_cut(children, k):
    """scikit-learn's cut of the tree into k clusters (a max-heap walk from the root)."""
    children = np.asarray(children).astype(np.int64).tolist()
    n = len(children) + 1
    nodes = [-(max(children[-1]) + 1)]
    for _ in range(k - 1):
        a, b = children[-nodes[0] - n]
        heapq.heappush(nodes, -a)
        heapq.heappushpop(nodes, -b)
    lab = np.zeros(n, dtype=np.int64)
    for i, node in enumerate(nodes):
        stack, leaves = [-node], []
        while stack:
            a = stack.pop()
            if a < n:
                leaves.append(a)
            else:
                stack.extend(children[a - n])
        lab[leaves] = i
    return lab
