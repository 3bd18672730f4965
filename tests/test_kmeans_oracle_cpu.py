"""tests/kmeans_oracle.py checked on the CPU: every Lloyd case the GPU tests use decides every label by more than 1e-9,
the equal-root pairs behave under np.linalg.norm + np.argmin as the GPU test expects of the kernels, lloyd_reference
reproduces the golden sets and exact sums, and the planted duplicates lie where the streams have wrapped."""
import math

import numpy as np
import pytest

from tests import kmeans_oracle as ko


@pytest.mark.parametrize("d,k,n", ko.lloyd_cases())
def test_lloyd_case_decides_every_label(d, k, n):
    """The two smallest scores of EVERY point are more than 1e-9 apart, so the label does not depend on how a dot product
    is summed (differences below 1e-14 at these magnitudes): no point has to be left out of a comparison."""
    P, C, mean = ko.lloyd_case(d, k, n, ko.lloyd_seed(d, k, n))
    assert P.shape == (n, d) and C.shape == (k, d)
    ref = ko.lloyd_reference(P, C, mean)
    assert ref.counts.sum() == n
    if k > 1:
        assert ref.margin > 1e-9, ref.margin


def test_other_stream_cases_are_steady_state_cases():
    """The fresh-process test of tests/test_kernels_gpu.py reuses steady-state cases: their margins are asserted above."""
    assert set(ko.OTHER_STREAM_LLOYD_DK) <= set(ko.LLOYD_STEADY_DK)
    assert set(ko.OTHER_STREAM_NEAREST_DK) <= set(ko.NEAREST_STEADY_DK)


def test_lloyd_reference_sums_are_exact_on_a_small_case():
    """The longdouble sums against math.fsum (exact), with an empty cluster in the middle and one at the end."""
    P, C, mean = ko.lloyd_case(3, 5, 999, 11)
    C[2] = 50.0
    C[4] = -60.0
    ref = ko.lloyd_reference(P, C, mean)
    assert ref.counts[2] == 0 and ref.counts[4] == 0 and ref.counts.sum() == 999
    Xc = P - mean
    for j in range(5):
        rows = Xc[ref.labels == j]
        for c in range(3):
            assert float(ref.sums[j, c]) == math.fsum(rows[:, c])
            assert float(ref.abs_sums[j, c]) == math.fsum(np.abs(rows[:, c]))
    assert float(ref.inertia) == math.fsum(ref.dist)
    np.testing.assert_array_equal(ref.dist, ((Xc - (C - mean)[ref.labels]) ** 2).sum(1))


@pytest.mark.parametrize("tag", ["syn_a", "syn_b", "syn_c"])
def test_lloyd_reference_on_the_golden_sets(golden_cluster, tag):
    """The quantities tests/test_kernels_gpu.py::test_kmeans_step_and_nearest derives, from lloyd_reference."""
    P = golden_cluster[f"{tag}.points"]
    C = golden_cluster[f"{tag}.init"]
    mean = P.mean(0)
    ref = ko.lloyd_reference(P, C, mean)
    Xc, Cc = P - mean, C - mean
    lab = ((Cc * Cc).sum(1)[None, :] - 2.0 * (Xc @ Cc.T)).argmin(1)
    np.testing.assert_array_equal(ref.labels, lab)
    k, d = C.shape
    sums = np.zeros((k, d))
    np.add.at(sums, lab, Xc)
    np.testing.assert_allclose(ref.sums.astype(np.float64), sums, rtol=1e-12, atol=1e-9)
    np.testing.assert_array_equal(ref.counts, np.bincount(lab, minlength=k))
    np.testing.assert_allclose(float(ref.inertia), ((Xc - Cc[lab]) ** 2).sum(), rtol=1e-12)
    np.testing.assert_array_equal(ref.dist, ((Xc - Cc[lab]) ** 2).sum(1))
    assert np.all(ref.abs_sums >= np.abs(ref.sums))


@pytest.mark.parametrize("d", [2, 4, 8])
def test_equal_root_pair(d):
    pair = ko.equal_root_pair(d)
    for A, B, equal in ((pair.A, pair.B, True), (pair.A_diff, pair.B_diff, False)):
        resA, resB = ko.sum_squares(A, pair.c), ko.sum_squares(B, pair.c)
        assert resB == np.nextafter(resA, 0.0) and resB < resA
        assert (np.sqrt(resA) == np.sqrt(resB)) == equal
        # sum_squares is the sum NumPy's norm takes the root of
        for X, res in ((A, resA), (B, resB)):
            assert np.add.reduce((X - pair.c)[None, :] ** 2, axis=1)[0] == res
            assert np.linalg.norm((X - pair.c)[None, :], axis=1)[0] == np.sqrt(res)
    for first in "AB":
        for rows in ((10, 522), (10, 3000)):
            for equal in (True, False):
                P, C = ko.equal_root_scene(d, pair, first, rows, equal)
                row = int(np.argmin(np.linalg.norm(P - C[0], axis=1)))
                row_of_b = rows[0] if first == "B" else rows[1]
                assert row == (rows[0] if equal else row_of_b)
                assert ko.oc.find_centroid_rows(P, C)[0] == row


def test_planted_rows_lie_behind_the_wraps():
    """At the steady-state size the duplicates sit in workgroup 512 of 1024, behind its 4096th point; at the small sizes in
    the second workgroup, resp. later in the only one."""
    n = ko.NEAREST_STEADY_N
    src0, dst0, m = ko.planted_rows(n)
    per = -(-n // 1024)
    assert ko.point_blocks(n) == 1024 and per >= 4200 and m == 50
    assert src0 + m <= per
    assert dst0 // per == 512 and (dst0 + m - 1) // per == 512 and dst0 - 512 * per >= 4096
    assert ko.point_blocks(1_337) == 2
    src0, dst0, m = ko.planted_rows(1_337)
    assert m == 50 and src0 + m <= 669 <= dst0 and dst0 + m <= 1_337
    for n in ko.LADDER_N:
        src0, dst0, m = ko.planted_rows(n)
        assert dst0 + m <= n and (m == 0 or src0 + m <= dst0)
    assert ko.planted_rows(1) == (0, 0, 0) and ko.planted_rows(1024)[2] == 50


def test_nearest_case_first_row_wins():
    P, C, ref = ko.nearest_case(4, 6, 1_337, ko.nearest_seed(4, 6, 1_337))
    src0, dst0, m = ko.planted_rows(1_337)
    np.testing.assert_array_equal(P[dst0:dst0 + m], P[src0:src0 + m])
    np.testing.assert_array_equal(C[0], P[dst0 + m // 5])
    assert ref[0] == src0 + m // 5
