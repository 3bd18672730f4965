"""NumPy float64 restatement of what the score kernels of scores.hip and the 1-NN transfer of kmeans.hip compute (test
helper, no GPU): per-label sums and dispersions, the summed Euclidean distance of every query to every cluster in its
direct form, the silhouette sample values with the kernels' conventions, and from those Calinski-Harabasz,
Davies-Bouldin and the mean silhouette.  Long sums go through math.fsum, so the reference carries the rounding of its
terms only.  Also the seeded inputs the CPU and the GPU tests share."""
import math

import numpy as np

U = 2.0 ** -53   # unit roundoff of float64


# ------------------------------------------------------------------------------------------------ the kernels, restated
def label_stats(P, labels, k, centers=None):
    """[sums k*d | counts k | sum ||x - c_label||^2 k | sum ||x - c_label|| k]; labels outside [0, k) are skipped; the
    last two groups are zero without centres."""
    P = np.asarray(P, dtype=np.float64)
    labels = np.asarray(labels)
    d = P.shape[1]
    out = np.zeros(k * d + 3 * k)
    for lab in range(k):
        rows = P[labels == lab]
        out[k * d + lab] = len(rows)
        for c in range(d):
            out[lab * d + c] = math.fsum(rows[:, c])
        if centers is not None and len(rows):
            ss = ((rows - np.asarray(centers, dtype=np.float64)[lab]) ** 2).sum(axis=1)
            out[k * d + k + lab] = math.fsum(ss)
            out[k * d + 2 * k + lab] = math.fsum(np.sqrt(ss))
    return out


def pair_distances(q, P):
    """||q - p|| for every row p of P, direct form: sqrt(((q - p)**2).sum())."""
    return np.sqrt(((np.asarray(q)[None, :] - P) ** 2).sum(axis=1))


def cluster_dist_sums(Q, P_sorted, start):
    """S[i][c] = sum over the rows j in [start[c], start[c+1]) of ||Q_i - P_sorted_j||."""
    k = len(start) - 1
    S = np.zeros((len(Q), k))
    for i, q in enumerate(Q):
        dist = pair_distances(q, P_sorted)
        for c in range(k):
            S[i, c] = math.fsum(dist[start[c]:start[c + 1]])
    return S


def silhouette_samples(S, qlabels, start):
    """Sample values from S with the kernel's conventions: a = S[own] / (n_own - 1), b = the smallest S[c] / n_c over the
    other populated clusters, s = (b - a) / max(a, b); 0 for a singleton cluster, for a label outside [0, k), when no
    other cluster is populated and when max(a, b) == 0."""
    S = np.asarray(S, dtype=np.float64)
    k = S.shape[1]
    sizes = np.diff(np.asarray(start)).astype(np.float64)
    out = np.zeros(len(S))
    for i, own in enumerate(np.asarray(qlabels)):
        if own < 0 or own >= k or sizes[own] <= 1:
            continue
        others = [S[i, c] / sizes[c] for c in range(k) if c != own and sizes[c] > 0]
        if not others:
            continue
        a, b = S[i, own] / (sizes[own] - 1.0), min(others)
        if max(a, b) > 0:
            out[i] = (b - a) / max(a, b)
    return out


def sort_by_cluster(P, labels, k):
    """(rows with a label in [0, k) stably sorted by label, start[k + 1])."""
    labels = np.asarray(labels)
    keep = np.flatnonzero((labels >= 0) & (labels < k))
    order = keep[np.argsort(labels[keep], kind="stable")]
    start = np.zeros(k + 1, dtype=np.int64)
    start[1:] = np.cumsum(np.bincount(labels[keep], minlength=k))
    return np.ascontiguousarray(P[order]), start


def scores_and_samples(P, labels):
    """(Calinski-Harabasz, Davies-Bouldin, mean silhouette, silhouette sample values) over the points with labels >= 0:
    noise is left out of all three scores, which is sklearn.metrics on the filtered set.  The sample values are in the
    order of the kept points."""
    P = np.asarray(P, dtype=np.float64)
    labels = np.asarray(labels)
    keep = labels >= 0
    P, labels = P[keep], labels[keep]
    n, d = P.shape
    k = int(labels.max()) + 1
    acc = label_stats(P, labels, k)
    counts = acc[k * d: k * d + k]
    present = counts > 0
    means = np.zeros((k, d))
    means[present] = acc[: k * d].reshape(k, d)[present] / counts[present, None]
    acc = label_stats(P, labels, k, means)
    ss, sd = acc[k * d + k: k * d + 2 * k], acc[k * d + 2 * k:]
    n_labels = int(present.sum())
    mean_all = np.array([math.fsum(P[:, c]) for c in range(d)]) / n
    extra = math.fsum(counts * ((means - mean_all) ** 2).sum(axis=1))
    intra = math.fsum(ss)
    ch = 1.0 if intra == 0.0 else extra * (n - n_labels) / (intra * (n_labels - 1.0))
    mp, sp = means[present], sd[present] / counts[present]
    cd = np.sqrt(((mp[:, None, :] - mp[None, :, :]) ** 2).sum(axis=2))
    if np.allclose(sp, 0) or np.allclose(cd, 0):
        db = 0.0
    else:
        cd[cd == 0] = np.inf
        db = float(np.mean(np.max((sp[:, None] + sp[None, :]) / cd, axis=1)))
    P_sorted, start = sort_by_cluster(P, labels, k)
    samples = silhouette_samples(cluster_dist_sums(P, P_sorted, start), labels, start)
    return float(ch), float(db), math.fsum(samples) / n, samples


def scores(P, labels):
    return scores_and_samples(P, labels)[:3]


def nearest_point(train, sup):
    """(index of the nearest training row per query, first index on ties; gap between the two smallest distinct squared
    distances per query, inf where there is one value only).  The squares are added one coordinate after the other."""
    train, sup = np.asarray(train, dtype=np.float64), np.asarray(sup, dtype=np.float64)
    acc = np.zeros((len(sup), len(train)))
    for c in range(train.shape[1]):
        diff = sup[:, None, c] - train[None, :, c]
        acc += diff * diff
    nn = np.argmin(acc, axis=1)
    best = acc[np.arange(len(sup)), nn]
    gap = np.where(acc > best[:, None], acc, np.inf).min(axis=1) - best
    return nn.astype(np.int64), gap


# ------------------------------------------------------------------------------------------------ shared inputs
def rounded(rng, shape, scale=1.0):
    """Points as the pipeline hands them over: 4 decimals."""
    return np.round(scale * rng.standard_normal(shape), 4)


def _sizes_d16():
    s = [7 + (5 * c) % 23 for c in range(64)]
    s[0], s[13], s[63], s[40] = 0, 0, 0, 1100   # empty first, middle and last cluster, one of more than a tile
    return s


# (d, cluster sizes, nq) of the cluster_dist_sums sweep
DIST_SUM_CASES = [
    (1, [1, 1023, 1024, 1025], 257),    # tile boundary on both sides, block boundary of the queries
    (2, [0, 2049, 3, 0], 1),            # empty first and last cluster, three tiles, one query
    (3, [20] * 64, 256),                # k = 64
    (4, [1025, 5], 300),                # last specialised instantiation
    (5, [1024, 1, 1030], 255),          # generic kernel at its smallest d
    (11, [2500, 40], 513),              # generic kernel, odd d
    (16, _sizes_d16(), 300),            # generic kernel at both limits
]


def dist_sum_case(d, sizes, nq):
    """(Q, P_sorted, start): cluster c around its own centre; every other query is a row of P_sorted (an exact zero
    term), the rest are independent points."""
    rng = np.random.Generator(np.random.PCG64(9000 + 100 * d + len(sizes)))
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    centres = rng.uniform(-2, 2, (len(sizes), d))
    P = np.round(np.repeat(centres, sizes, axis=0) + 0.3 * rng.standard_normal((start[-1], d)), 4)
    Q = np.round(rng.uniform(-2.5, 2.5, (nq, d)), 4)
    rows = rng.integers(0, len(P), nq)
    Q[::2] = P[rows[::2]]
    return np.ascontiguousarray(Q), np.ascontiguousarray(P), start


def dist_sum_bound(m, d):
    """Relative distance of a float64 sum of m non-negative terms ||q - p|| in d dimensions, in any order, from the
    fsum of the terms as this module computes them: the sum is within (m - 1) u of the exact sum of its own terms, each
    term carries at most d + 2 roundings (difference, square, d - 1 additions, square root), and the factor 2 covers
    the same roundings of the reference's terms."""
    return 2.0 * (m + d + 4) * U


def mixture(seed, n, d, k, spread=0.35):
    """(points, labels 0..k-1 with every label used, int32)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    centres = rng.uniform(-2, 2, (k, d))
    lab = np.concatenate([np.arange(k), rng.integers(0, k, n - k)]).astype(np.int32)
    rng.shuffle(lab)
    return np.ascontiguousarray(np.round(centres[lab] + spread * rng.standard_normal((n, d)), 4)), lab
