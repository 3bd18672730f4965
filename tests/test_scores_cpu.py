"""The score oracle (tests/scores_oracle.py) pinned to scikit-learn, and the error bound of the cluster_dist_sums test
checked against the reference alone.  No GPU."""
import math

import numpy as np
import pytest

from tests import scores_oracle as so


def _mixture_with_edges(d):
    """~600 points in 6 labels: label 4 is unused (a gap) and label 5 holds one point."""
    P, lab = so.mixture(300 + d, 600, d, 4)
    lab[17] = 5
    return P, lab


@pytest.mark.parametrize("d", [1, 3, 8, 16])
def test_oracle_scores_match_sklearn(d):
    """CH, DB, the mean silhouette and every sample value against sklearn.metrics at rtol 1e-9 (float64 both sides;
    sklearn's distances use the dot-product expansion, the oracle the direct form); atol 1e-12 on the sample values,
    which are differences of two means of order 1."""
    from sklearn.metrics import calinski_harabasz_score, davies_bouldin_score, silhouette_samples, silhouette_score

    P, lab = _mixture_with_edges(d)
    assert np.sum(lab == 4) == 0 and np.sum(lab == 5) == 1
    ch, db, si, samples = so.scores_and_samples(P, lab)
    np.testing.assert_allclose(ch, calinski_harabasz_score(P, lab), rtol=1e-9)
    np.testing.assert_allclose(db, davies_bouldin_score(P, lab), rtol=1e-9)
    np.testing.assert_allclose(si, silhouette_score(P, lab), rtol=1e-9)
    np.testing.assert_allclose(samples, silhouette_samples(P, lab), rtol=1e-9, atol=1e-12)
    assert samples[17] == 0.0   # the singleton


@pytest.mark.parametrize("d", [3, 16])
def test_oracle_leaves_noise_out_of_all_three_scores(d):
    """With noise labels the oracle equals sklearn on the filtered set -- not sklearn's reading of -1 as a cluster."""
    from sklearn.metrics import calinski_harabasz_score, davies_bouldin_score, silhouette_samples, silhouette_score

    P, lab = _mixture_with_edges(d)
    rng = np.random.Generator(np.random.PCG64(5))
    lab[rng.choice(len(lab), 60, replace=False)] = -1
    lab[17] = 5
    keep = lab >= 0
    ch, db, si, samples = so.scores_and_samples(P, lab)
    np.testing.assert_allclose(ch, calinski_harabasz_score(P[keep], lab[keep]), rtol=1e-9)
    np.testing.assert_allclose(db, davies_bouldin_score(P[keep], lab[keep]), rtol=1e-9)
    np.testing.assert_allclose(si, silhouette_score(P[keep], lab[keep]), rtol=1e-9)
    ref = silhouette_samples(P[keep], lab[keep])
    assert len(samples) == keep.sum()
    np.testing.assert_allclose(si, ref.sum() / keep.sum(), rtol=1e-9)
    np.testing.assert_allclose(samples, ref, rtol=1e-9, atol=1e-12)
    assert so.scores(P, lab) == so.scores(P[keep], lab[keep])


def test_silhouette_sample_conventions():
    S = np.array([[3.0, 4.0, 0.0], [0.0, 2.0, 0.0], [5.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    start = np.array([0, 2, 3, 3])            # sizes 2, 1, 0
    got = so.silhouette_samples(S, [0, 0, 1, -1, 3], start)
    #      a = 3, b = 4         a = 0, b = 2   singleton  noise  label >= k
    np.testing.assert_array_equal(got, [0.25, 1.0, 0.0, 0.0, 0.0])
    assert so.silhouette_samples(np.array([[2.0]]), [0], np.array([0, 3]))[0] == 0.0          # no other cluster
    assert so.silhouette_samples(np.zeros((1, 2)), [0], np.array([0, 2, 4]))[0] == 0.0        # max(a, b) == 0


def test_nearest_point_oracle_first_index_and_gap():
    train = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 0.0], [0.0, 3.0]])
    nn, gap = so.nearest_point(train, np.array([[0.9, 0.0], [0.0, 0.0]]))
    np.testing.assert_array_equal(nn, [1, 0])
    np.testing.assert_allclose(gap, [0.81 - 0.01, 1.0], rtol=1e-12)
    assert so.nearest_point(train[:1], train[:1])[1][0] == np.inf


@pytest.mark.parametrize("d,sizes,nq", so.DIST_SUM_CASES, ids=[f"d{c[0]}" for c in so.DIST_SUM_CASES])
def test_dist_sum_bound_holds_for_a_plain_sequential_sum(d, sizes, nq):
    """The bound the GPU test allows, 2 (m + d + 4) 2^-53 relative, checked without the kernel: a float64 sum of the same
    terms taken one after the other (np.cumsum), with the squares added coordinate by coordinate, stays inside it."""
    Q, P, start = so.dist_sum_case(d, sizes, nq)
    worst = 0.0
    for q in Q[:: max(1, nq // 24)]:
        acc = np.zeros(len(P))
        for c in range(d):
            acc += (q[c] - P[:, c]) ** 2
        seq_terms, ref_terms = np.sqrt(acc), so.pair_distances(q, P)
        for c, m in enumerate(sizes):
            if m == 0:
                continue
            ref = math.fsum(ref_terms[start[c]:start[c + 1]])
            seq = np.cumsum(seq_terms[start[c]:start[c + 1]])[-1]
            bound = so.dist_sum_bound(m, d) * ref
            assert abs(seq - ref) <= bound
            if ref > 0:
                worst = max(worst, abs(seq - ref) / bound)
    assert worst < 1.0
