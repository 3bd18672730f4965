"""Host finish of HDBSCAN: from the minimum spanning tree of the mutual-reachability graph (hip.mr_mst, in Prim
order) to labels, membership probabilities and centroids -- a NumPy / Python restatement of what
sklearn.cluster.HDBSCAN does after mst_from_data_matrix (sklearn/cluster/_hdbscan/hdbscan.py::_process_mst,
_linkage.pyx::make_single_linkage, _tree.pyx::tree_to_labels, HDBSCAN._weighted_cluster_center), with
allow_single_cluster=False as the reference fixes it.  No GPU work: one argsort and O(n) tree walks.

Everything whose ORDER scikit-learn's result depends on is kept: the default-kind argsort of the weights (ties are
the normal case: a fifth of the edges of a continuous 2-D set share their weight through the core distances), the
row order of the condensed tree (breadth first), the accumulation order of the stabilities, the union-by-rank of the
labelling pass, and the iteration order of the Python sets of the epsilon search."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

# sklearn's MST_edge_dtype: argsort is called on the strided 'distance' field of such an array, as scikit-learn calls it
MST_EDGE_DTYPE = np.dtype([("current_node", np.int64), ("next_node", np.int64), ("distance", np.float64)])


def check_parameters(n: int, min_cluster_size, min_samples) -> int:
    """The two parameter errors HDBSCAN.fit raises, with its texts.  Returns the effective min_samples."""
    if n == 1:
        raise ValueError("n_samples=1 while HDBSCAN requires more than one sample")
    ms = min_cluster_size if min_samples is None else min_samples
    if ms > n:
        raise ValueError(f"min_samples ({ms}) must be at most the number of samples in X ({n})")
    return ms


def single_linkage(src: np.ndarray, dst: np.ndarray, w: np.ndarray):
    """_process_mst: sort the edges by weight (numpy's default argsort, exactly scikit-learn's call) and name merge i
    node n + i.  Returns (left, right, value, size) of the n - 1 merges: lists, value as float64 array."""
    m = len(w)
    n = m + 1
    mst = np.empty(m, dtype=MST_EDGE_DTYPE)
    mst["current_node"] = src
    mst["next_node"] = dst
    mst["distance"] = w
    order = np.argsort(mst["distance"])
    mst = mst[order]
    a_l, b_l = mst["current_node"].tolist(), mst["next_node"].tolist()
    parent = [-1] * (2 * n - 1)
    size = [1] * n + [0] * (n - 1)
    left, right, sizes = [0] * m, [0] * m, [0] * m
    nxt = n
    for i in range(m):
        a = p = a_l[i]
        while parent[a] != -1:
            a = parent[a]
        while p != a and parent[p] != a:
            p, parent[p] = parent[p], a
        b = p = b_l[i]
        while parent[b] != -1:
            b = parent[b]
        while p != b and parent[p] != b:
            p, parent[p] = parent[p], b
        left[i], right[i] = a, b
        sizes[i] = size[nxt] = size[a] + size[b]
        parent[a] = parent[b] = nxt
        nxt += 1
    return left, right, np.ascontiguousarray(mst["distance"]), sizes


def _bfs_hierarchy(left, right, n, root):
    """Breadth-first node list below `root` (level by level, left before right)."""
    result, queue = [], [root]
    while queue:
        result.extend(queue)
        nxt = []
        for x in queue:
            if x >= n:
                nxt.append(left[x - n])
                nxt.append(right[x - n])
        queue = nxt
    return result


def condense_tree(left, right, value, sizes, min_cluster_size: int):
    """_condense_tree: rows (parent, child, lambda, size) in scikit-learn's order, as four lists."""
    m = len(left)
    n = m + 1
    root = 2 * m
    next_label = n + 1
    relabel = [0] * (root + 1)
    relabel[root] = n
    ignore = bytearray(root + 1)
    val = value.tolist()
    inf = float("inf")
    P, C, L, S = [], [], [], []
    for node in _bfs_hierarchy(left, right, n, root):
        if node < n or ignore[node]:
            continue
        a, b, dist = left[node - n], right[node - n], val[node - n]
        lam = 1.0 / dist if dist > 0.0 else inf
        ca = sizes[a - n] if a >= n else 1
        cb = sizes[b - n] if b >= n else 1
        me = relabel[node]
        if ca >= min_cluster_size and cb >= min_cluster_size:
            relabel[a] = next_label
            next_label += 1
            P.append(me); C.append(relabel[a]); L.append(lam); S.append(ca)
            relabel[b] = next_label
            next_label += 1
            P.append(me); C.append(relabel[b]); L.append(lam); S.append(cb)
            continue
        if ca < min_cluster_size and cb < min_cluster_size:
            fall = (a, b)
        elif ca < min_cluster_size:
            relabel[b] = me
            fall = (a,)
        else:
            relabel[a] = me
            fall = (b,)
        for side in fall:
            for sub in _bfs_hierarchy(left, right, n, side):
                if sub < n:
                    P.append(me); C.append(sub); L.append(lam); S.append(1)
                ignore[sub] = 1
    return P, C, L, S


def _stabilities(P, C, L, S):
    """_compute_stability: {cluster: sum over its rows of (lambda - birth) * size}, accumulated in row order."""
    smallest = min(P)
    births = {c: lam for c, lam in zip(C, L)}
    births[smallest] = 0.0
    result = np.zeros(max(P) - smallest + 1, dtype=np.float64)
    lam_a = np.asarray(L, dtype=np.float64)
    birth_a = np.asarray([births.get(p, np.nan) for p in P], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        term = ((lam_a - birth_a) * np.asarray(S, dtype=np.float64)).tolist()   # elementwise: the float64 operations scikit-learn does
    acc = result.tolist()
    for p, t in zip(P, term):
        acc[p - smallest] += t
    return {i + smallest: v for i, v in enumerate(acc)}


class _ClusterTree:
    """The rows of the condensed tree whose child is a cluster (size > 1), with the look-ups the selection needs."""

    def __init__(self, P, C, L, S):
        self.rows = [(p, c, lam, s) for p, c, lam, s in zip(P, C, L, S) if s > 1]
        self.children = {}
        self.parent, self.value, self.size = {}, {}, {}
        for p, c, lam, s in self.rows:
            self.children.setdefault(p, []).append(c)
            self.parent[c], self.value[c], self.size[c] = p, lam, s
        self.root = min(p for p, _, _, _ in self.rows) if self.rows else None

    def below(self, node):
        """node and every cluster under it (bfs_from_cluster_tree; only membership is used)."""
        out, stack = [node], [node]
        while stack:
            for c in self.children.get(stack.pop(), ()):
                out.append(c)
                stack.append(c)
        return out

    def leaves(self):
        """get_cluster_tree_leaves: depth first from the root, children in row order."""
        if not self.rows:
            return []
        out, stack = [], [self.root]
        while stack:
            node = stack.pop()
            ch = self.children.get(node)
            if ch:
                stack.extend(reversed(ch))
            else:
                out.append(node)
        return out


def _traverse_upwards(tree: _ClusterTree, eps: float, leaf: int) -> int:
    while True:
        parent = tree.parent[leaf]
        if parent == tree.root:
            return leaf   # allow_single_cluster=False: the node closest to the root
        if np.float64(1.0) / np.float64(tree.value[parent]) > eps:
            return parent
        leaf = parent


def _epsilon_search(leaves: set, tree: _ClusterTree, eps: float) -> set:
    selected, processed = [], set()
    for leaf in leaves:   # the iteration order of a Python set of ints, as in scikit-learn
        if np.float64(1.0) / np.float64(tree.value[leaf]) < eps:
            if leaf not in processed:
                top = _traverse_upwards(tree, eps, leaf)
                selected.append(top)
                for sub in tree.below(top):
                    if sub != top:
                        processed.add(sub)
        else:
            selected.append(leaf)
    return set(selected)


def _select_clusters(P, C, L, S, stability, method: str, eps: float, max_cluster_size: Optional[int], n: int):
    tree = _ClusterTree(P, C, L, S)
    node_list = sorted(stability.keys(), reverse=True)[:-1]   # the root is never a cluster
    is_cluster = {c: True for c in node_list}
    if max_cluster_size is None:
        max_cluster_size = n + 1
    if method == "eom":
        for node in node_list:
            subtree = np.sum([stability[c] for c in tree.children.get(node, ())])
            if subtree > stability[node] or tree.size[node] > max_cluster_size:
                is_cluster[node] = False
                stability[node] = subtree
            else:
                for sub in tree.below(node):
                    if sub != node:
                        is_cluster[sub] = False
        if eps != 0.0 and tree.rows:
            eom = [c for c in is_cluster if is_cluster[c]]
            if len(eom) == 1 and eom[0] == tree.root:
                selected = []
            else:
                selected = _epsilon_search(set(eom), tree, eps)
            for c in is_cluster:
                is_cluster[c] = c in selected
    elif method == "leaf":
        leaves = set(tree.leaves())
        if len(leaves) == 0:
            for c in is_cluster:
                is_cluster[c] = False
            is_cluster[min(P)] = True
        selected = _epsilon_search(leaves, tree, eps) if eps != 0.0 else leaves
        for c in is_cluster:
            is_cluster[c] = c in selected
    else:
        raise ValueError(f"cluster_selection_method {method!r}: 'eom' or 'leaf'")
    return set(c for c in is_cluster if is_cluster[c])


def _do_labelling(P, C, clusters: set, label_of: dict, n: int) -> np.ndarray:
    """_do_labelling with allow_single_cluster=False: scikit-learn's union by rank over the rows in order."""
    size = max(P) + 1
    up = list(range(size))
    rank = [0] * size

    def find(x):
        r = x
        while up[r] != r:
            r = up[r]
        while up[x] != r:
            x, up[x] = up[x], r
        return r

    for p, c in zip(P, C):
        if c in clusters:
            continue
        x, y = find(p), find(c)
        if rank[x] < rank[y]:
            up[x] = y
        elif rank[x] > rank[y]:
            up[y] = x
        else:
            up[y] = x
            rank[x] += 1
    root = min(P)
    labels = np.empty(root, dtype=np.intp)
    out = [-1] * root
    for i in range(root):
        c = find(i)
        if c != root:
            out[i] = label_of[c]
    labels[:] = out
    return labels


def _max_lambdas(P, L):
    """max_lambdas: the maximum over each RUN of equal parents; a later run of the same parent replaces the earlier."""
    deaths = {}
    cur, mx = P[0], L[0]
    for p, lam in zip(P[1:], L[1:]):
        if p == cur:
            if lam > mx:
                mx = lam
        else:
            deaths[cur] = mx
            cur, mx = p, lam
    deaths[cur] = mx
    return deaths


def _probabilities(P, C, L, labels: np.ndarray, cluster_of: dict) -> np.ndarray:
    deaths = _max_lambdas(P, L)
    root = min(P)
    child = np.asarray(C, dtype=np.intp)
    lam = np.asarray(L, dtype=np.float64)
    pts = child < root
    child, lam = child[pts], lam[pts]
    lab = labels[child]
    keep = lab != -1
    child, lam, lab = child[keep], lam[keep], lab[keep]
    result = np.zeros(len(labels), dtype=np.float64)
    if len(child):
        k = len(cluster_of)
        death_by_label = np.asarray([deaths.get(cluster_of[i], 0.0) for i in range(k)], dtype=np.float64)
        mx = death_by_label[lab]
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.minimum(lam, mx) / mx
        result[child] = np.where((mx == 0.0) | np.isinf(lam), 1.0, ratio)
    return result


def tree_to_labels(left, right, value, sizes, min_cluster_size: int, cluster_selection_method: str = "eom",
                   cluster_selection_epsilon: float = 0.0, max_cluster_size: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """tree_to_labels(single_linkage_tree, ..., allow_single_cluster=False): (labels intp, probabilities float64)."""
    n = len(left) + 1
    P, C, L, S = condense_tree(left, right, value, sizes, int(min_cluster_size))
    stability = _stabilities(P, C, L, S)
    clusters = _select_clusters(P, C, L, S, stability, cluster_selection_method, float(cluster_selection_epsilon), max_cluster_size, n)
    label_of = {c: i for i, c in enumerate(sorted(clusters))}
    cluster_of = {i: c for c, i in label_of.items()}
    labels = _do_labelling(P, C, clusters, label_of, n)
    return labels, _probabilities(P, C, L, labels, cluster_of)


def weighted_centroids(X: np.ndarray, labels: np.ndarray, probabilities: np.ndarray) -> np.ndarray:
    """HDBSCAN._weighted_cluster_center(store_centers="centroid")."""
    k = len(set(labels.tolist()) - {-1, -2})
    cents = np.empty((k, X.shape[1]), dtype=np.float64)
    for idx in range(k):
        mask = labels == idx
        cents[idx] = np.average(X[mask], weights=probabilities[mask], axis=0)
    return cents


def finish(X: np.ndarray, src: np.ndarray, dst: np.ndarray, w: np.ndarray, min_cluster_size: int,
           cluster_selection_method: str = "eom", cluster_selection_epsilon: float = 0.0,
           max_cluster_size: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(labels_, probabilities_, centroids_) of HDBSCAN(..., store_centers="centroid", allow_single_cluster=False)
    from the points and their mutual-reachability MST in Prim order."""
    left, right, value, sizes = single_linkage(src, dst, w)
    labels, prob = tree_to_labels(left, right, value, sizes, min_cluster_size, cluster_selection_method,
                                  cluster_selection_epsilon, max_cluster_size)
    return labels, prob, weighted_centroids(np.asarray(X, dtype=np.float64), labels, prob)
