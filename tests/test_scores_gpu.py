"""The score kernels of scores.hip (label_stats, cluster_dist_sums, silhouette_sum, linear_binning), the 1-NN transfer
of kmeans.hip and statistics.clustering_scores on top of them against the float64 oracle of tests/scores_oracle.py, at
the sizes where the kernels change path: the 1024-row tile of the distance sums, their generic instantiation (d = 5..16),
k = 64, empty and singleton clusters, noise labels, the LDS / global switch of the 1-D binning and the 256-row tile of
the 1-NN search.  Points are what the pipeline hands over: seeded PCG64, rounded to 4 decimals."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import fes as ofes
from tests import scores_oracle as so

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ cluster_dist_sums
@pytest.mark.parametrize("d,sizes,nq", so.DIST_SUM_CASES, ids=[f"d{c[0]}" for c in so.DIST_SUM_CASES])
def test_cluster_dist_sums_match_oracle(d, sizes, nq):
    """Every S[i][c] within 2 (m + d + 4) 2^-53 relative of the fsum of the direct-form distances (so.dist_sum_bound; the
    bound is checked against a plain sequential sum in test_scores_cpu), an empty cluster exactly 0.0, two runs
    bit-equal.  Largest error seen on an MI355X: 0.098 of the bound (d = 5), 0.003 to 0.084 at the other d."""
    from deep_cartograph_amd import hip

    Q, P, start = so.dist_sum_case(d, sizes, nq)
    ref = so.cluster_dist_sums(Q, P, start)
    Qd, Pd, sd = dev(Q), dev(P), dev(start)
    S1 = hip.cluster_dist_sums(Qd, Pd, sd)
    S2 = hip.cluster_dist_sums(Qd, Pd, sd)
    assert torch.equal(S1, S2)
    got = S1.cpu().numpy()
    assert got.shape == (nq, len(sizes))
    worst = 0.0
    for c, m in enumerate(sizes):
        if m == 0:
            assert np.all(got[:, c] == 0.0)
            continue
        bound = so.dist_sum_bound(m, d) * ref[:, c]
        err = np.abs(got[:, c] - ref[:, c])
        worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
        assert np.all(err <= bound), (c, m, float(np.max(err / np.maximum(bound, 1e-300))))
    print(f"cluster_dist_sums d={d}: worst error {worst:.3f} of the bound")


# ------------------------------------------------------------------------------------------------ label_stats
LABEL_STATS_CASES = [(1, 1, 1), (300, 8, 2), (1025, 3, 5), (4097, 4, 64), (5000, 16, 64)]


def _label_stats_case(n, d, k):
    rng = np.random.Generator(np.random.PCG64(100 * n + d))
    P = so.rounded(rng, (n, d), 1.5)
    lab = rng.integers(0, k, n).astype(np.int32)
    if (n, d, k) == (1025, 3, 5):
        lab[rng.choice(n, 90, replace=False)] = -1
        lab[500] = k + 2          # a label >= k, passed on purpose: skipped like noise
    if (n, d, k) == (4097, 4, 64):
        lab[lab == 21] = 22       # one label id unused
    centers = rng.uniform(-1, 1, (k, d))
    return P, lab, centers


@pytest.mark.parametrize("with_centers", [False, True], ids=["sums", "centers"])
@pytest.mark.parametrize("n,d,k", LABEL_STATS_CASES)
def test_label_stats_match_oracle(n, d, k, with_centers):
    """Counts exact; sums within n max|x| 2^-52 absolute (zero-mean data cancels, so the bound is on the magnitudes
    added); the two dispersion groups within 2 (n + d + 4) 2^-53 relative, the argument of so.dist_sum_bound; a second
    call bit-equal.  Largest error seen on an MI355X: sums 0.025 of the bound (n = 300, d = 8), dispersions 0.0024."""
    from deep_cartograph_amd import hip

    P, lab, centers = _label_stats_case(n, d, k)
    if (n, d, k) == (1025, 3, 5):
        assert (lab == -1).sum() == 90 and (lab >= k).sum() == 1
    if (n, d, k) == (4097, 4, 64):
        assert (lab == 21).sum() == 0
    ref = so.label_stats(P, lab, k, centers if with_centers else None)
    Pd, ld, cd = dev(P), dev(lab), dev(centers) if with_centers else None
    a1 = hip.label_stats(Pd, ld, k, centers=cd)
    a2 = hip.label_stats(Pd, ld, k, centers=cd)
    got = a1.cpu().numpy()
    kd = k * d
    assert torch.equal(a1, a2)
    if not with_centers:
        assert np.all(got[kd + k:] == 0.0)   # include/dcv.h: the dispersion groups are zero without centres
    np.testing.assert_array_equal(got[kd: kd + k], ref[kd: kd + k])
    sum_bound = n * np.abs(P).max() * 2.0 ** -52
    sum_err = np.abs(got[:kd] - ref[:kd]).max()
    print(f"label_stats n={n} d={d} k={k}: sums worst error {sum_err / sum_bound:.4f} of the bound")
    assert sum_err <= sum_bound
    if with_centers:
        rtol = so.dist_sum_bound(n, d)
        disp_err = np.abs(got[kd + k:] - ref[kd + k:])
        assert np.all(disp_err <= rtol * ref[kd + k:])
        frac = np.max(disp_err[ref[kd + k:] > 0] / (rtol * ref[kd + k:][ref[kd + k:] > 0]), initial=0.0)
        print(f"label_stats n={n} d={d} k={k}: dispersions worst error {frac:.4f} of the bound")


# ------------------------------------------------------------------------------------------------ silhouette_sum
@functools.lru_cache(maxsize=None)
def _silhouette_case():
    """2500 points in 5 clusters of sizes 700, 1, 0, 900, 899 (a singleton and an empty one), d = 3; every point is a
    query, 200 of them relabelled as noise and one with a label >= k.  Returns (S of the oracle, qlabels, start)."""
    sizes = [700, 1, 0, 900, 899]
    rng = np.random.Generator(np.random.PCG64(41))
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    P = np.round(np.repeat(rng.uniform(-2, 2, (5, 3)), sizes, axis=0) + 0.5 * rng.standard_normal((2500, 3)), 4)
    ql = np.repeat(np.arange(5), sizes).astype(np.int32)
    S = so.cluster_dist_sums(P, P, start)
    noise = rng.choice(2500, 200, replace=False)
    ql[noise] = -1
    ql[noise[0]] = 5
    return S, ql, start


def _check_silhouette_sum(S, ql, start):
    from deep_cartograph_amd import hip

    samples = so.silhouette_samples(S, ql, start)
    got = float(hip.silhouette_sum(dev(S), dev(ql), dev(start)).item())
    tol = 2.0 * len(S) * so.U * float(np.abs(samples).sum())
    assert abs(got - math.fsum(samples)) <= tol, (got, math.fsum(samples), tol)
    return got, samples


def test_silhouette_sum_matches_oracle_samples():
    """The oracle's S uploaded as is, so that only this kernel is under test: nq = 2500 (three blocks, several trips of
    the grid-stride loop), a singleton cluster, an empty cluster, noise queries and a query label >= k.  The sum of the
    samples within 2 nq 2^-53 of sum |s| (the samples themselves are the same operations on both sides)."""
    S, ql, start = _silhouette_case()
    got, samples = _check_silhouette_sum(S, ql, start)
    assert samples[700] == 0.0 and np.all(samples[ql < 0] == 0.0) and np.count_nonzero(samples) > 2000
    assert abs(got) > 100.0   # a real sum, not the all-zero answer


def test_silhouette_sum_one_query_block_and_k1():
    S, ql, start = _silhouette_case()
    _check_silhouette_sum(S[:255], ql[:255], start)                       # less than one block
    # k = 1: no other cluster, every sample 0, the sum exactly 0
    got, _ = _check_silhouette_sum(S[:, :1].copy(), np.zeros(2500, dtype=np.int32), np.array([0, 2500], dtype=np.int64))
    assert got == 0.0


# ------------------------------------------------------------------------------------------------ clustering_scores
def _gap(lab):
    return np.where(lab >= 2, lab + 1, lab).astype(np.int32)      # label 2 unused


def _noisy(lab):
    out = lab.copy()
    out[np.random.Generator(np.random.PCG64(77)).choice(len(lab), len(lab) // 10, replace=False)] = -1
    return out


SCORE_SETS = {
    "d8_k5": lambda: so.mixture(81, 3001, 8, 5),
    "d16_k64": lambda: so.mixture(82, 3000, 16, 64, spread=0.25),
    "d8_gap": lambda: (lambda P, lab: (P, _gap(lab)))(*so.mixture(81, 3001, 8, 5)),
    "d8_noise": lambda: (lambda P, lab: (P, _noisy(lab)))(*so.mixture(81, 3001, 8, 5)),
}


@functools.lru_cache(maxsize=None)
def _score_set(name):
    """(P, labels, oracle's (ch, db, silhouette, samples)), computed once and shared."""
    P, lab = SCORE_SETS[name]()
    return P, lab, so.scores_and_samples(P, lab)


def _assert_scores(got, ref, rtol=1e-12):
    for g, r, what in zip(got, ref, ("Calinski-Harabasz", "Davies-Bouldin", "silhouette")):
        np.testing.assert_allclose(g, r, rtol=rtol, atol=0, err_msg=what)


@pytest.mark.parametrize("name", ["d8_k5", "d16_k64", "d8_gap"])
def test_clustering_scores_match_oracle(name):
    """Host code and kernels against scores_oracle.scores at rtol 1e-12: d = 8 / k = 5, d = 16 / k = 64 (the generic
    distance-sum kernel), labels with an unused id; the P_dev path bit-equal to the upload path."""
    from deep_cartograph_amd import statistics

    P, lab, ref = _score_set(name)
    if name == "d8_gap":
        assert (lab == 2).sum() == 0 and lab.max() == 5
    got = statistics.clustering_scores(P.copy(), lab)
    _assert_scores(got, ref[:3])
    assert statistics.clustering_scores(P, lab, P_dev=dev(P)) == got


def test_clustering_scores_leave_noise_out():
    """About 10 % of the labels set to -1: all three scores equal the oracle's and the scores of the filtered set.
    (Before the fix cluster 0 owned the noise rows, which sort first, and the mean divided by all the queries.)"""
    from deep_cartograph_amd import statistics

    P, lab, ref = _score_set("d8_noise")
    keep = lab >= 0
    assert keep.sum() == 3001 - 300
    got = statistics.clustering_scores(P.copy(), lab)
    print(f"noise: silhouette {got[2]!r}, oracle {ref[2]!r}")
    _assert_scores(got, ref[:3])
    _assert_scores(got, statistics.clustering_scores(P[keep].copy(), lab[keep]))


def test_clustering_scores_strided_silhouette():
    """silhouette_max_points = 1001 on 3001 points: stride 3.  The silhouette is the mean of the oracle's sample values
    at [::3]; CH and DB do not change."""
    from deep_cartograph_amd import statistics

    P, lab, ref = _score_set("d8_k5")
    assert math.ceil(len(P) / 1001) == 3
    got = statistics.clustering_scores(P.copy(), lab, silhouette_max_points=1001)
    sub = ref[3][::3]
    _assert_scores(got, (ref[0], ref[1], math.fsum(sub) / len(sub)))
    assert got[:2] == statistics.clustering_scores(P.copy(), lab)[:2]


def _scores_rank(rank, world, port, tmpdir):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deep_cartograph_amd import parallel, statistics

    torch.cuda.set_device(0)
    comm = parallel.Comm()
    data = np.load(os.path.join(tmpdir, "points.npz"))
    b, e = parallel.shard_bounds(data["P"].shape[0], world, rank)
    out = {tag: np.array(statistics.clustering_scores(data["P"][b:e].copy(), data[tag][b:e].copy(), comm=comm))
           for tag in ("plain", "noise")}
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), **out)
    dist.destroy_process_group()


def test_clustering_scores_two_ranks_match_single_process(tmp_path):
    """Frame-sharded scores with two processes on the one GPU (gloo): every rank returns the single-process CH, DB and
    silhouette to 1e-12 relative (the partial sums are grouped differently), with and without noise labels."""
    import socket

    import torch.multiprocessing as mp

    from deep_cartograph_amd import statistics

    P, plain, _ = _score_set("d8_k5")
    noise = _score_set("d8_noise")[1]
    np.savez(tmp_path / "points.npz", P=P, plain=plain, noise=noise)
    ref = {"plain": statistics.clustering_scores(P.copy(), plain), "noise": statistics.clustering_scores(P.copy(), noise)}
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_scores_rank, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=180)      # each rank under its own limit: a rank that is still there is ended
    alive = [p.is_alive() for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
            p.join()
    assert not any(alive) and [p.exitcode for p in procs] == [0, 0]
    for r in range(2):
        part = np.load(tmp_path / f"rank{r}.npz")
        for tag in ("plain", "noise"):
            _assert_scores(part[tag], ref[tag])


# ------------------------------------------------------------------------------------------------ linear_binning
def _check_grid(grid, n, outside):
    """What a wrapped fixed-point weight breaks: every weight in [0, n], and the weights add up to the points inside
    exactly (multiples of 2^-36 below 10^5: the float64 sum is exact)."""
    assert n <= 100_000
    assert grid.min() >= 0.0 and grid.max() <= n
    assert grid.sum() == n - outside


@functools.lru_cache(maxsize=None)
def _bin_matrix():
    """5000 x 4, every column on its own range, so that a swap of axes or bounds moves the weights."""
    rng = np.random.Generator(np.random.PCG64(51))
    X = np.empty((5000, 4))
    X[:, 0] = rng.uniform(0.0, 3.3, 5000)
    X[:, 1] = rng.uniform(-50.0, 50.0, 5000)
    X[:, 2] = rng.normal(-0.3, 0.45, 5000)
    X[:, 3] = rng.normal(1.0, 0.5, 5000) ** 2
    return np.round(X, 4)


def _binning(P, cols, lo, hi, bins):
    from deep_cartograph_amd import hip

    g, out = hip.linear_binning(P, cols, lo, hi, bins)
    return g.cpu().numpy(), out


@pytest.mark.parametrize("bins", [2, 37])
def test_linear_binning_column_selection(bins):
    """cols = [2, 0] of a 4-column matrix with different bounds per axis: a mix-up of axes, bounds or the leading
    dimension changes the grid."""
    X = _bin_matrix()
    lo, hi = [-1.0, 0.25], [0.5, 3.0]
    exp = ofes.linear_binning(X[:, [2, 0]], lo, hi, bins)
    n_out = int(np.sum((X[:, 2] < lo[0]) | (X[:, 2] > hi[0]) | (X[:, 0] < lo[1]) | (X[:, 0] > hi[1])))
    assert 100 < n_out < 2500
    got, out = _binning(dev(X), [2, 0], lo, hi, bins)
    assert out == n_out
    np.testing.assert_allclose(got, exp, rtol=0, atol=1e-9 * len(X))
    _check_grid(got, len(X), out)
    if bins > 2:
        assert np.abs(got - got.T).max() > 1.0     # the case can tell the axes apart


@pytest.mark.parametrize("bins", [2, 150, 4096, 4097])
def test_linear_binning_1d_row_slice_view(bins):
    """cols = [3] of the row-slice view P[100:], what compute_fes passes for a block; bins on both sides of the switch
    from the per-block LDS grid (<= 4096) to global atomics with the same data, and the smallest grid."""
    X = _bin_matrix()
    lo, hi = [0.2], [2.6]
    P = dev(X)[100:]
    assert P.stride(0) == 4 and P.storage_offset() == 400
    exp = ofes.linear_binning(X[100:, [3]], lo, hi, bins)
    n_out = int(np.sum((X[100:, 3] < lo[0]) | (X[100:, 3] > hi[0])))
    assert 100 < n_out < 2500
    got, out = _binning(P, [3], lo, hi, bins)
    assert out == n_out
    np.testing.assert_allclose(got, exp, rtol=0, atol=1e-9 * 4900)
    _check_grid(got, 4900, out)


BOUNDS = [(-1.0, 0.5), (0.25, 3.0)]


@pytest.mark.parametrize("lo,hi", BOUNDS)
@pytest.mark.parametrize("bins", [2, 150, 4096, 4097])
def test_linear_binning_1d_points_on_the_bounds(bins, lo, hi):
    """Points exactly at lo and hi are inside, a point at hi gives its full weight to the last node; one ulp outside,
    NaN and +-inf are counted as outside and leave the grid untouched."""
    col = np.array([lo, hi, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), np.nan, np.inf, -np.inf, hi, lo, lo])
    X = np.zeros((len(col), 2))
    X[:, 1] = col
    got, out = _binning(dev(X), [1], [lo], [hi], bins)
    exp = np.zeros(bins)
    exp[0], exp[-1] = 3.0, 3.0
    assert out == 5
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(ofes.linear_binning(X[:, [1]], [lo], [hi], bins), exp)


@pytest.mark.parametrize("bins", [2, 64])
def test_linear_binning_2d_points_on_the_bounds(bins):
    lo, hi = [-1.0, 0.25], [0.5, 3.0]
    mid = [-0.25, 1.0]
    above = [np.nextafter(hi[0], np.inf), np.nextafter(hi[1], np.inf)]
    below = [np.nextafter(lo[0], -np.inf), np.nextafter(lo[1], -np.inf)]
    inside = [(lo[0], lo[1]), (lo[0], hi[1]), (hi[0], lo[1]), (hi[0], hi[1]), (hi[0], hi[1])]
    outside = [(above[0], mid[1]), (mid[0], above[1]), (below[0], mid[1]), (mid[0], below[1]), (np.nan, mid[1]),
               (mid[0], np.nan), (np.inf, mid[1]), (mid[0], -np.inf), (hi[0], above[1]), (below[0], lo[1])]
    X = np.array(inside + outside)
    got, out = _binning(dev(X), [0, 1], lo, hi, bins)
    exp = np.zeros((bins, bins))
    exp[0, 0], exp[0, -1], exp[-1, 0], exp[-1, -1] = 1.0, 1.0, 1.0, 2.0
    assert out == len(outside)
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(ofes.linear_binning(X, lo, hi, bins), exp)


def test_linear_binning_2d_weights_do_not_wrap():
    """Points at hi on the first axis (f0 = 1) whose second fraction is an odd multiple of 2^-37: two of the rounded
    fixed-point weights come to 2^36 + 1 between them, and the fourth, taken as the remainder, must not go below zero.
    Nothing else lands on the first row of nodes: 64-bit atomics wrap back as soon as a cell receives a whole weight
    from elsewhere, so a wrapped remainder shows only where it stays alone (as 2^28 in a cell that holds nothing)."""
    X = np.array([[1.0, 0.5 + 2.0 ** -37], [1.0, 0.25 + 2.0 ** -37], [1.0, 1.0 - 2.0 ** -37]])
    lo, hi = [0.0, 0.0], [1.0, 1.0]
    got, out = _binning(dev(X), [0, 1], lo, hi, 2)
    assert out == 0
    _check_grid(got, len(X), out)
    np.testing.assert_array_equal(got[0], [0.0, 0.0])
    np.testing.assert_allclose(got, ofes.linear_binning(X, lo, hi, 2), rtol=0, atol=1e-9 * len(X))


# ------------------------------------------------------------------------------------------------ nearest_point
def _nearest_case(n_train, n_sup, d):
    """Training rows with a duplicated block (the first copy must win), every other query a training row, the rest
    independent; queries whose two smallest distinct squared distances are closer than 1e-9, or that tie between
    different rows, are drawn again, so that no index hangs on the last bit of a sum."""
    rng = np.random.Generator(np.random.PCG64(1000 * n_train + d))
    train = np.round(rng.uniform(-1, 1, (n_train, d)), 4)
    b = min(9, n_train // 3)
    train[n_train // 2: n_train // 2 + b] = train[:b]
    sup = np.round(rng.uniform(-1, 1, (n_sup, d)), 4)
    pick = rng.integers(0, n_train, n_sup)
    dup = np.arange(0, min(2 * b, n_sup), 2)
    pick[dup] = n_train // 2 + dup // 2                  # queries on the second copies of the duplicated rows
    sup[::2] = train[pick[::2]]
    for _ in range(20):
        nn, gap = so.nearest_point(train, sup)
        acc = ((sup[:, None, :] - train[None, :, :]) ** 2).sum(axis=2)
        tied = acc <= acc.min(axis=1, keepdims=True) + 1e-9
        bad = np.array([gap[i] <= 1e-9 or not np.all(train[tied[i]] == train[nn[i]]) for i in range(n_sup)])
        if not bad.any():
            break
        sup[bad] = np.round(rng.uniform(-1, 1, (int(bad.sum()), d)), 4)
    return train, sup, dup


@pytest.mark.parametrize("n_train,n_sup,d", [(1, 1, 1), (255, 257, 2), (256, 256, 3), (257, 1, 5), (700, 300, 8), (1000, 513, 16)])
def test_nearest_point_matches_oracle(n_train, n_sup, d):
    """Bit-exact indices at the 256-row tile of the training rows and the 256-query block, on both sides and with a
    tail, d up to 16, exact ties between duplicated rows (first index) and queries that are training rows."""
    from deep_cartograph_amd import hip

    train, sup, dup = _nearest_case(n_train, n_sup, d)
    nn, gap = so.nearest_point(train, sup)
    assert np.all(gap > 1e-9)
    np.testing.assert_array_equal(nn[dup], dup // 2)     # the first copy, not the one the query was taken from
    got = hip.nearest_point(dev(train), dev(sup)).cpu().numpy()
    np.testing.assert_array_equal(got, nn)
