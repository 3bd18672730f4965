"""The point streams of kmeans.hip against tests/kmeans_oracle.py: every register-kernel instantiation, every trip count of
the LDS ring below its first wrap, and both streams in their steady state.

Which kernel a shape reaches (read from km_reg_pick / near_multi_pick / dcv_kmeans_step / dcv_nearest_rows):

  Lloyd pass, d <= 4:
    k <= 8        kmeans_step_reg_kernel<d, k, RING>: the cluster count is the instantiation.  RING (ring_stream, LDS-DMA)
                  when d is 2 or 4 and no per-point distances are asked for; otherwise reg_stream with U = 2 points per
                  thread and batch (d = 4: the lane-pair path pair_issue / pair_finish).
    9 <= k <= 16  kmeans_step_reg_kernel<d, 16, false>: always reg_stream, `j < k` tests in the point loop.
    k > 16, d > 4 kmeans_step_kernel (LDS atomics); not the subject of this file.
  nearest_rows, d <= 4, in chunks of 8 centroids on grid.y:
    d = 1, 3      nearest_rows_multi_kernel<d, false, 0>: reg_stream with U = 4.
    d = 2         nearest_rows_multi_kernel<2, true, 0>: ring.
    d = 4         nearest_rows_multi_kernel<4, true, k> for k <= 8 (one instantiation per count), <4, true, 0> above.
    d > 4         nearest_rows_kernel, one pass per centroid, always takes the root.
  DCV_KM_RING=0 (read once per process) sends every RING case to reg_stream: section D lives in
  tests/test_kernels_gpu.py::test_register_stream_matches_ring_and_numpy, which starts that process.

The grid: point_blocks(n) = min(ceil(n / 1024), 4 CUs, 1024) workgroups of ceil(n / grid) points; the Lloyd register
kernel caps it to CUs x resident blocks (one round of the chip).  On 256 CUs that is 1024 workgroups for nearest_rows
and 256 .. 1024 for Lloyd once n >= 1 M.

Sections and why their sizes are the smallest that reach what they are for:

  A  d in 1..4 x k in {1..8, 9, 16}: all 36 Lloyd instantiations without the ring, the 16 with it (plain run at even d,
     k <= 8) and k = 9 as the count that is not KMAX.  Every (D, KMAX) has its own WR = KMAX (D + 1) + 2, hence its own
     butterfly (halving steps while the count is even, all-reduce steps once it is odd), base / dup pattern and src mapping
     into `part`.  n = 40: less than one 64-point chunk, one workgroup.  n = 1 337: two workgroups of 669 / 668 points, an
     odd first row of the second, a ragged last chunk.  nearest_rows at n = 1 337 for d = 4, k in 1..8 (the KX
     instantiations) and d in 1..3, k in {1, 8, 9} (one full chunk of centroids, one more than a chunk).
  B  One workgroup, n in {1, 64, 65, 256, 257, 512, 769, 1024} = 1, 1, 2, 4, 5, 8, 13, 16 chunks: a wave of the ring runs
     0 .. 4 iterations, so every value of `ahead` (chunks requested behind the current one, 0 .. 3) and `since` (0 .. 3)
     below the wrap occurs, with and without a ragged last chunk.
  C  Steady state.  A workgroup refills a ring slot for the first time at its 17th chunk, i.e. with more than 1024 points,
     which the grid hands out only above 1024 x 1024 points.  Lloyd at n = 2 400 011: at least 2 344 points per workgroup
     = 37 chunks, 10 iterations per wave: every slot refilled twice (the lgkmcnt(0) wait before a refill and the
     since = kRingSlots - 1 term of the vmcnt count at work); reg_stream with U = 2 takes 512 points per batch: five
     batches ba, bb, ba, bb, ba, the `pos + 2 * step` re-issue twice.  nearest_rows at n = 4 300 003: 4 200 points per
     workgroup, U = 4 takes 1024 per batch: ba, bb, ba, bb, ba; the planted duplicates of rows 525 .. 574 sit from point 4100 of
     workgroup 512 on, in batch 5 and ring iteration 16, and must lose against the first workgroup's rows.
  E  Two sums of squares that are adjacent doubles with the same correctly rounded root (kmeans_oracle.equal_root_pair),
     once met by ONE thread (rows 10 and 522 of workgroup 0: same lane, same wave, the `res < best` / `bthr` branch of
     nearest_rows_multi_kernel decides) and once in different workgroups (take_min on the rounded roots decides).
  F  kmeanspp_potentials at 1 and 8 = kPpMaxTrials candidates.

The bound on a sum.  Labels and counts are exact.  A sum of the pass (a coordinate of a cluster, the inertia) is compared
as |got - ref| <= L 2^-53 S, S = the oracle's sum of the absolute values of the very terms added, L = the longest chain
of additions a term goes through: the first-order worst case of any summation tree of depth L.  From the code:
  * kmeans_step_reg_kernel adds a point into the thread's registers: one addition per point of the thread.  A thread of
    ring_stream and of reg_stream at d = 4 takes lane l of the chunks wave + 4 kk, any other d the rows begin + t + 256 m:
    ceil(points of the workgroup / 256) points either way, and the workgroup has ceil(n / grid) <= ceil(n / CUs) points
    once the grid is no smaller than the number of CUs: ceil(ceil(n / CUs) / 256).
  * butterfly_sum<WR, 32>: offsets 32, 16, 8, 4, 2, 1, one addition each: 6.
  * ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]: 3.
  * sum_blocks_kernel: a thread adds the blocks t, t + 256, ...: at most ceil(1024 / 256) = 4; block_sum's tree over 256
    threads: 8.
L = ceil(ceil(n / CUs) / 256) + 6 + 3 + 4 + 8 (kmeans_oracle.lloyd_chain).  Below 1024 CUs points the grid is smaller
than the CU count, a thread has up to 4 points and 3 rounded additions (the first one, to 0.0, is exact), and the grid is
at most 256 workgroups, whose single addition per thread in sum_blocks_kernel is exact as well: 3 + 6 + 3 + 0 + 8 = 20
roundings against L >= 22, so the same L holds there.  A lost or doubled point moves a sum by ~1e-7 of S; L 2^-53 is
~3e-15 at n = 2.4 M.  The inertia's terms are the kernel's own squared distances, which the per-point comparison ties to
the oracle's (rtol 1e-12, the project's bound for that quantity)."""
import numpy as np
import pytest
import torch

from tests import kmeans_oracle as ko

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.as_tensor(a).cuda()


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


# inputs and references, built once per case; of the steady-state cases (up to 138 MB of points) only the last one is kept
_small, _big = {}, {}


def _cached(kind, d, k, n, build):
    key = (kind, d, k, n)
    store = _big if n > 1_000_000 else _small
    if key not in store:
        if store is _big:
            store.clear()
        store[key] = build()
    return store[key]


def lloyd_inputs(d, k, n):
    def build():
        P, C, mean = ko.lloyd_case(d, k, n, ko.lloyd_seed(d, k, n))
        return P, C, mean, ko.lloyd_reference(P, C, mean)
    return _cached("lloyd", d, k, n, build)


def nearest_inputs(d, k, n):
    return _cached("nearest", d, k, n, lambda: ko.nearest_case(d, k, n, ko.nearest_seed(d, k, n)))


def check_lloyd(P, C, mean, ref, want_mindist):
    """One pass from labels of -1 against the oracle, a second one that changes nothing; returns labels and acc."""
    from deep_cartograph_amd import hip

    n, d = P.shape
    k = C.shape[0]
    Pd, Cd, off = dev(P), dev(C - mean), dev(mean)
    labels = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    acc_d, md = hip.kmeans_step(Pd, Cd, labels, offset=off, want_mindist=want_mindist)
    acc = acc_d.cpu().numpy()
    lab = labels.cpu().numpy()
    np.testing.assert_array_equal(lab, ref.labels)
    np.testing.assert_array_equal(acc[k * d:k * d + k], ref.counts)
    assert acc[k * d + k + 1] == n
    L = ko.lloyd_chain(n, _cus())
    ok, err = ko.within_sum_bound(acc[:k * d].reshape(k, d), ref.sums, ref.abs_sums, L)
    assert ok, (L, err, ref.abs_sums)
    ok, err = ko.within_sum_bound(acc[k * d + k], ref.inertia, ref.inertia, L)
    assert ok, (L, err, ref.inertia)
    if want_mindist:
        np.testing.assert_allclose(md.cpu().numpy(), ref.dist, rtol=1e-12, atol=1e-15)
    else:
        assert md is None
    again, _ = hip.kmeans_step(Pd, Cd, labels, offset=off, want_mindist=want_mindist)
    again = again.cpu().numpy()
    assert again[k * d + k + 1] == 0
    assert again[:k * d + k + 1].tobytes() == acc[:k * d + k + 1].tobytes()
    np.testing.assert_array_equal(labels.cpu().numpy(), ref.labels)
    return lab, acc


def check_nearest(P, C, ref, row_offset=None):
    from deep_cartograph_amd import hip

    Pd, Cd = dev(P), dev(C)
    dist, rows = hip.nearest_rows(Pd, Cd)
    np.testing.assert_array_equal(rows.cpu().numpy(), ref)
    np.testing.assert_array_equal(dist.cpu().numpy(), np.linalg.norm(P[ref] - C, axis=1))
    if row_offset is not None:
        dist_o, rows_o = hip.nearest_rows(Pd, Cd, row_offset=row_offset)
        np.testing.assert_array_equal(rows_o.cpu().numpy(), ref + row_offset)
        assert dist_o.cpu().numpy().tobytes() == dist.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("n", ko.LLOYD_SMALL_N)
@pytest.mark.parametrize("d,k", ko.LLOYD_SMALL_DK)
def test_every_lloyd_instantiation(d, k, n):
    """Section A: plain (the ring at even d and k <= 8, else the register stream) and with distances (always the register
    stream); both against the oracle and against each other."""
    P, C, mean, ref = lloyd_inputs(d, k, n)
    lab_p, acc_p = check_lloyd(P, C, mean, ref, False)
    lab_d, acc_d = check_lloyd(P, C, mean, ref, True)
    np.testing.assert_array_equal(lab_p, lab_d)
    np.testing.assert_array_equal(acc_p[k * d:k * d + k], acc_d[k * d:k * d + k])


@pytest.mark.parametrize("d,k", ko.NEAREST_SMALL_DK)
def test_every_nearest_rows_instantiation(d, k):
    """Section A: the KX instantiations of the ring kernel at d = 4 and one / two chunks of centroids at d = 1, 2, 3, on two
    workgroups."""
    check_nearest(*nearest_inputs(d, k, 1_337), row_offset=777)


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("n", ko.LADDER_N)
@pytest.mark.parametrize("d,k", ko.LADDER_DK)
def test_ring_trip_count_ladder(d, k, n):
    """Section B: 1 .. 16 chunks in one workgroup."""
    P, C, mean, ref = lloyd_inputs(d, k, n)
    lab_p, _ = check_lloyd(P, C, mean, ref, False)
    lab_d, _ = check_lloyd(P, C, mean, ref, True)
    np.testing.assert_array_equal(lab_p, lab_d)
    check_nearest(*nearest_inputs(d, k, n))


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("want_mindist", [False, True], ids=["plain", "dist"])
@pytest.mark.parametrize("d,k", ko.LLOYD_STEADY_DK)
def test_lloyd_steady_state(d, k, want_mindist):
    """Section C: the ring past its second wrap (plain, d = 2 / 4, k <= 8) and five batches of the register stream."""
    P, C, mean, ref = lloyd_inputs(d, k, ko.LLOYD_STEADY_N)
    check_lloyd(P, C, mean, ref, want_mindist)


@pytest.mark.parametrize("d,k", ko.NEAREST_STEADY_DK)
def test_nearest_rows_steady_state(d, k):
    """Section C: duplicates met in batch 5 / ring iteration 16 of workgroup 512 lose against the first workgroup's rows."""
    P, C, ref = nearest_inputs(d, k, ko.NEAREST_STEADY_N)
    src0, dst0, m = ko.planted_rows(ko.NEAREST_STEADY_N)
    assert ref[0] <= src0 + m // 5 and np.array_equal(P[ref[0]], C[0])
    check_nearest(P, C, ref, row_offset=1_000_000)


# ------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("d", [2, 4, 8])
def test_equal_rounded_roots_go_to_the_first_row(d):
    """Section E: the row is NumPy's: the earlier one when the roots are equal, B's when they differ."""
    from deep_cartograph_amd import hip

    pair = ko.equal_root_pair(d)
    for rows in ((10, 522), (10, 3000)):          # one thread's stream; two workgroups
        for first in "AB":
            for equal in (True, False):
                P, C = ko.equal_root_scene(d, pair, first, rows, equal)
                ref = ko.oc.find_centroid_rows(P, C)
                row_of_b = rows[0] if first == "B" else rows[1]
                assert ref[0] == (rows[0] if equal else row_of_b)
                dist, got = hip.nearest_rows(dev(P), dev(C))
                np.testing.assert_array_equal(got.cpu().numpy(), ref, err_msg=f"rows={rows} first={first} equal={equal}")
                np.testing.assert_array_equal(dist.cpu().numpy(), np.linalg.norm(P[ref] - C, axis=1))


# ------------------------------------------------------------------------------------------------ F
@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("d", [3, 16])
def test_kmeanspp_potentials_trial_counts(d, T):
    """Section F: one candidate and kPpMaxTrials of them; formula and tolerances of
    tests/test_kernels_gpu.py::test_kmeanspp_passes_even_and_odd_d."""
    from deep_cartograph_amd import hip

    n = 1_537
    rng = np.random.Generator(np.random.PCG64(3100 + 10 * d + T))
    P = np.round(rng.uniform(-1, 1, (n, d)), 4)
    mean = P.mean(0)
    X = P - mean

    def dist(c):
        return np.maximum(0.0, -2.0 * (X @ c) + (c * c).sum() + (X * X).sum(1))

    c0 = rng.uniform(-1, 1, d) - mean
    cand = rng.uniform(-1, 1, (T, d)) - mean
    Pd, off = dev(P), dev(mean)
    closest = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    hip.kmeanspp_update(Pd, dev(c0), closest, True, offset=off)
    ref = dist(c0)
    np.testing.assert_allclose(closest.cpu().numpy(), ref, rtol=1e-12, atol=1e-15)
    pots = hip.kmeanspp_potentials(Pd, dev(cand), closest, offset=off)
    assert pots.shape == (T,)
    np.testing.assert_allclose(pots.cpu().numpy(), [np.minimum(ref, dist(c)).sum() for c in cand], rtol=1e-12)
