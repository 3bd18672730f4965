"""NumPy restatement of what the point streams of kmeans.hip compute (test helper: NumPy only, no torch, no GPU), and
the seeded inputs the CPU and the GPU tests share.

* lloyd_case / lloyd_reference: one Lloyd pass.  Labels by the sklearn formula on float64 centred points; the sums of
  the centred points and the inertia are accumulated in np.longdouble (64-bit mantissa), so the reference carries the
  rounding of its terms only, and come with the sums of the absolute values of the same terms: the scale of the
  summation-tree bound the GPU tests use.
* nearest_case: points with a run of rows duplicated deep inside a later workgroup's range, expected rows from
  oracle.cluster.find_centroid_rows (np.linalg.norm + np.argmin).
* equal_root_pair: two points whose sums of squares against a centroid are adjacent doubles with the SAME correctly
  rounded root (and a counterpart pair whose roots differ): the case the square-root shortcut of the one-pass
  nearest-rows kernel exists for.
* the case lists of tests/test_kmeans_streams_gpu.py, each with the seed tests/test_kmeans_oracle_cpu.py checks."""
from collections import namedtuple

import numpy as np

from oracle import cluster as oc

assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 here: the reference would not be one"

U = 2.0 ** -53   # unit roundoff of float64

# the grid of a streaming pass (points.h: point_blocks): 1024 points per workgroup until CUs x 4, at most 1024
PT_BLOCK_POINTS = 1024
PT_MAX_BLOCKS = 1024


def point_blocks(n, cus=256):
    return max(1, min(-(-n // PT_BLOCK_POINTS), 4 * cus, PT_MAX_BLOCKS))


# ------------------------------------------------------------------------------------------------ Lloyd pass
def lloyd_case(d, k, n, seed):
    """Points around k cluster centres uniform in [-1, 1] with 0.15 sigma noise, rounded to 4 decimals; start centres =
    k distinct rows + 1e-3 (with fewer than k points: every row, then the rounded cluster centres); the mean of the points
    (the offset KMeans.fit subtracts)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cent = rng.uniform(-1, 1, (k, d))
    P = np.round(cent[rng.integers(0, k, n)] + 0.15 * rng.standard_normal((n, d)), 4)
    if n >= k:
        C = P[rng.choice(n, k, replace=False)] + 1e-3
    else:
        C = np.concatenate([P, np.round(cent[:k - n], 4)]) + 1e-3
    return P, C, P.mean(0)


LloydRef = namedtuple("LloydRef", "labels counts margin dist sums abs_sums inertia")


def _sums_by_label(values, order, starts, counts):
    """Per label the longdouble sum of the rows of `values` (n x d float64): sort by label, np.add.reduceat."""
    k, d = len(counts), values.shape[1]
    out = np.zeros((k, d), dtype=np.longdouble)
    full = np.flatnonzero(counts)
    if len(full):
        out[full] = np.add.reduceat(values[order].astype(np.longdouble), starts[full], axis=0)
    return out


def lloyd_reference(P, C, mean):
    """labels = argmin_j(|c_j|^2 - 2 x.c_j) on the float64 centred points x = P - mean against c = C - mean (first minimum
    wins), counts, margin = the smallest gap between the two smallest scores of a point (inf for one centre), dist = the
    squared distance of every point to its centre (float64), and in np.longdouble: sums / abs_sums[j][c] = the sum of
    x[c] / |x[c]| over the points of label j, inertia = the sum of dist."""
    P = np.asarray(P, dtype=np.float64)
    Xc, Cc = P - mean, np.asarray(C, dtype=np.float64) - mean
    k = Cc.shape[0]
    pw = (Cc * Cc).sum(1)[None, :] - 2.0 * (Xc @ Cc.T)
    labels = pw.argmin(1)
    if k > 1:
        two = np.partition(pw, 1, axis=1)[:, :2]
        margin = float((two[:, 1] - two[:, 0]).min())
    else:
        margin = float("inf")
    del pw
    counts = np.bincount(labels, minlength=k)
    dist = ((Xc - Cc[labels]) ** 2).sum(1)
    order = np.argsort(labels, kind="stable")
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    sums = _sums_by_label(Xc, order, starts, counts)
    abs_sums = _sums_by_label(np.abs(Xc), order, starts, counts)
    inertia = np.add.reduce(dist.astype(np.longdouble))
    return LloydRef(labels, counts, margin, dist, sums, abs_sums, inertia)


def lloyd_chain(n, cus):
    """L of the bound |got - ref| <= L * 2^-53 * S on a sum of the Lloyd pass: the longest chain of additions a term goes
    through in kmeans_step_reg_kernel + sum_blocks_kernel, for a grid no smaller than the number of CUs (derivation: module
    docstring of tests/test_kmeans_streams_gpu.py)."""
    per_thread = -(-(-(-n // cus)) // 256)
    blocks_chain = -(-PT_MAX_BLOCKS // 256)
    return per_thread + 6 + 3 + blocks_chain + 8


def within_sum_bound(got, ref, scale, L):
    """|got - ref| <= L * 2^-53 * scale, elementwise, evaluated in np.longdouble."""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(np.longdouble) - ref)
    return bool(np.all(err <= np.longdouble(L) * np.longdouble(U) * scale)), err


# ------------------------------------------------------------------------------------------------ nearest rows
def planted_rows(n, cus=256):
    """(src0, dst0, m): the rows [src0, src0 + m) of the first workgroup's range are copied to [dst0, dst0 + m), which lie in
    workgroup blocks // 2 and, where that workgroup has that many points, behind its 4096th point (offset 4100: chunk 64 of
    the workgroup -- iteration 16 of wave 0's ring, batch 5 of the register stream with four points per thread)."""
    nb = point_blocks(n, cus)
    per = -(-n // nb)
    b = nb // 2
    blk_len = min(per, n - b * per)
    m = min(50, per // 4)
    src0 = per // 8
    dst0 = b * per + min(4100, blk_len - m)
    if m == 0 or dst0 < src0 + m:
        return 0, 0, 0
    return src0, dst0, m


def nearest_case(d, k, n, seed):
    """Uniform points rounded to 4 decimals, centroids rounded to 3; planted_rows duplicated, centroid 0 IS one of the
    duplicated points (distance 0 at two rows: the first must win).  Returns P, C and the expected rows."""
    rng = np.random.Generator(np.random.PCG64(seed))
    P = np.round(rng.uniform(-1, 1, (n, d)), 4)
    C = np.round(rng.uniform(-1, 1, (k, d)), 3)
    src0, dst0, m = planted_rows(n)
    if m:
        P[dst0:dst0 + m] = P[src0:src0 + m]
        C[0] = P[dst0 + m // 5]
    return P, C, oc.find_centroid_rows(P, C)


# ------------------------------------------------------------------------------------------------ equal rounded roots
def sum_squares(x, c):
    """The sum of squares np.linalg.norm(x - c) takes the root of: separately rounded squares, added sequentially for
    d < 8 and as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) for d = 8 (NumPy's pairwise summation; kmeans.hip:
    np_norm)."""
    df = np.asarray(x, dtype=np.float64) - np.asarray(c, dtype=np.float64)
    sq = df * df
    d = len(sq)
    if d < 8:
        res = np.float64(0.0)
        for q in range(d):
            res = res + sq[q]
        return res
    assert d == 8
    return ((sq[0] + sq[1]) + (sq[2] + sq[3])) + ((sq[4] + sq[5]) + (sq[6] + sq[7]))


EqualRootPair = namedtuple("EqualRootPair", "c A B A_diff B_diff")


def _one_ulp_below(A, c, limit=200_000):
    """B = A with coordinate 0 stepped towards c until the rounded sum of squares drops: the step changes the sum by far
    less than its ulp, so the first drop is to the adjacent double (None when it is not)."""
    resA = sum_squares(A, c)
    B = A.copy()
    for _ in range(limit):
        B[0] = np.nextafter(B[0], c[0])
        resB = sum_squares(B, c)
        if resB != resA:
            return B if resB == np.nextafter(resA, 0.0) else None
    return None


def equal_root_pair(d):
    """Centroid c and points A, B with sum_squares(B, c) the double adjacent below sum_squares(A, c) and equal rounded
    roots: np.argmin over np.linalg.norm takes whichever comes first, a comparison of the sums of squares always B.  A_diff,
    B_diff: the same construction where the roots differ (B_diff is nearer in every arithmetic)."""
    rng = np.random.Generator(np.random.PCG64(7000 + d))
    c = np.round(rng.uniform(-1, 1, d), 3)
    same = diff = None
    for _ in range(64):
        # a small first coordinate (one ulp of it moves the sum by ~1e-4 of its ulp) beside ones that carry the sum
        A = c + np.concatenate([[0.01 * rng.uniform(0.5, 1.5)], rng.uniform(0.3, 0.6, d - 1)])
        B = _one_ulp_below(A, c)
        if B is None:
            continue
        resA, resB = sum_squares(A, c), sum_squares(B, c)
        assert resB == np.nextafter(resA, 0.0)
        if np.sqrt(resA) == np.sqrt(resB):
            same = same or (A, B)
        else:
            diff = diff or (A, B)
        if same and diff:
            break
    assert same and diff, "equal_root_pair: no pair found from 64 starting points"
    return EqualRootPair(c, same[0], same[1], diff[0], diff[1])


def equal_root_scene(d, pair, first, rows, equal=True, n_far=5000, n_cent=3):
    """The pair embedded in n_far far-away points: `first` ('A' or 'B') goes to rows[0], the other to rows[1].  Centroid 0
    is the pair's; the others are drawn among the far points."""
    rng = np.random.Generator(np.random.PCG64(7100 + d))
    n = n_far + 2
    P = np.round(pair.c + rng.uniform(5, 6, (n, d)), 4)
    A, B = (pair.A, pair.B) if equal else (pair.A_diff, pair.B_diff)
    P[rows[0]], P[rows[1]] = (A, B) if first == "A" else (B, A)
    C = np.concatenate([pair.c[None, :], np.round(pair.c + rng.uniform(5, 6, (n_cent - 1, d)), 3)])
    return P, C


# ------------------------------------------------------------------------------------------------ the GPU tests' cases
LLOYD_SMALL_N = (40, 1_337)
LLOYD_SMALL_DK = [(d, k) for d in (1, 2, 3, 4) for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16)]
LADDER_DK = [(2, 3), (4, 6)]
LADDER_N = (1, 64, 65, 256, 257, 512, 769, 1024)
LLOYD_STEADY_N = 2_400_011
LLOYD_STEADY_DK = [(1, 2), (2, 3), (2, 8), (3, 5), (4, 6), (4, 16)]
NEAREST_SMALL_DK = [(4, k) for k in range(1, 9)] + [(d, k) for d in (1, 2, 3) for k in (1, 8, 9)]
NEAREST_STEADY_N = 4_300_003
NEAREST_STEADY_DK = [(1, 3), (2, 6), (3, 11), (4, 6), (4, 17)]
# the other stream in a fresh process (tests/test_kernels_gpu.py)
OTHER_STREAM_NEAREST_DK = [(2, 6), (4, 6), (4, 17)]
OTHER_STREAM_LLOYD_DK = [(2, 3), (4, 6)]

# Seeds.  A Lloyd case is usable when the two smallest scores of EVERY point are more than 1e-9 apart (rounding differences
# between BLAS, sequential and fused dot products are below 1e-14 at these magnitudes), which a seed either gives or does
# not: 4-decimal points meet exact ties, most readily at d = 1.  The default is the formula below; the cases it fails for
# carry the first seed counted up from it that holds (tests/test_kmeans_oracle_cpu.py asserts every one).
_LLOYD_SEEDS = {
    (1, 5, 1_337): 342_106,
    (2, 3, 2_400_011): 16_204,
}


def lloyd_seed(d, k, n):
    return _LLOYD_SEEDS.get((d, k, n), 5000 + 100 * d + k + (n % 1000) * 1000)


def nearest_seed(d, k, n):
    return 6000 + 100 * d + k + (n % 1000) * 1000


def lloyd_cases():
    """Every (d, k, n) a Lloyd pass runs at in the GPU tests."""
    cases = [(d, k, n) for d, k in LLOYD_SMALL_DK for n in LLOYD_SMALL_N]
    cases += [(d, k, n) for d, k in LADDER_DK for n in LADDER_N]
    cases += [(d, k, LLOYD_STEADY_N) for d, k in LLOYD_STEADY_DK]
    return cases
