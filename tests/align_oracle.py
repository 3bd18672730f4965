"""Float64 / pure-Python oracles of align_trajectories, shared by tests/test_align_cpu.py and tests/test_align_gpu.py:

* `transform`      out = (x - c_mob) . R + c_ref of dcv_transform_frames, written out term by term (no matmul: a matrix
                   product may sum in another order or fuse), left to right in float64;
* `fit_transforms` the [n, 15] transform rows of a fit, from tests/geometry_oracle.py's Kabsch;
* `local_align`    a plain three-matrix (Gotoh) Smith-Waterman in Python loops, written independently of
                   deep_cartograph_amd/sequence.py.  It returns the score, the number of end cells that reach it and the
                   mapping under TWO OPPOSITE tie rules, so a test can tell whether the optimum of an input is unique."""
import numpy as np

from tests import geometry_oracle as go

IDENTITY_ROW = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0], dtype=np.float64)


def transform(xyz, rows):
    """float64 [n, A, 3]: every atom of frame f moved by rows[f] = R row-major (9), c_mob (3), c_ref (3)."""
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    rows = np.asarray(rows, dtype=np.float64)
    out = np.empty(x.shape, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        p0 = x[:, :, 0] - rows[:, None, 9]
        p1 = x[:, :, 1] - rows[:, None, 10]
        p2 = x[:, :, 2] - rows[:, None, 11]
        for c in range(3):
            out[:, :, c] = ((p0 * rows[:, None, c] + p1 * rows[:, None, 3 + c]) + p2 * rows[:, None, 6 + c]) + rows[:, None, 12 + c]
    return out


def fit_transforms(xyz, fit, fit_ref):
    """[n, 16] float64 rows (the last column 0) of the optimal fit of the atoms `fit` of every frame onto fit_ref."""
    xyz = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    rows = np.zeros((len(xyz), 16))
    for f in range(len(xyz)):
        R, c_mob, c_ref = go.kabsch(xyz[f, fit], fit_ref)
        rows[f, :15] = np.concatenate([R.ravel(), c_mob, c_ref])
    return rows


def random_transforms(n, seed, shift=300.0):
    """[n, 16]: seeded proper rotations and centroids of a few hundred Angstrom, different in every frame."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = np.zeros((n, 16))
    for f in range(n):
        rows[f, :9] = go.random_rotation(rng).ravel()
        rows[f, 9:15] = rng.uniform(-shift, shift, 6)
    return rows


# ------------------------------------------------------------------------------------------------ local alignment
NEG = float("-inf")


def local_align(a, b, match=1.0, mismatch=-1.0, gap_open=2.0, gap_extend=0.5):
    """(score, number of end cells, pairs_first, pairs_last) of the local alignment of two strings: a gap of length L
    costs gap_open + gap_extend (L - 1).  pairs_* are the aligned index pairs (i, j), mismatches included, under two
    opposite tie rules: `first` takes the end cell with the smallest (i, j) and prefers stop, diagonal, gap in a, gap in
    b in that order; `last` takes the end cell with the largest (i, j) and prefers them in the reverse order.  Where both
    give the same pairs and there is one end cell, the optimum is taken for unique."""
    n, m = len(a), len(b)
    M = [[NEG] * (m + 1) for _ in range(n + 1)]    # ends in a[i-1] : b[j-1]
    X = [[NEG] * (m + 1) for _ in range(n + 1)]    # ends in  -     : b[j-1]  (gap in a)
    Y = [[NEG] * (m + 1) for _ in range(n + 1)]    # ends in a[i-1] :  -      (gap in b)
    best = 0.0
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            s = match if a[i - 1] == b[j - 1] else mismatch
            M[i][j] = s + max(0.0, M[i - 1][j - 1], X[i - 1][j - 1], Y[i - 1][j - 1])
            X[i][j] = max(M[i][j - 1] - gap_open, X[i][j - 1] - gap_extend, Y[i][j - 1] - gap_open)
            Y[i][j] = max(M[i - 1][j] - gap_open, Y[i - 1][j] - gap_extend, X[i - 1][j] - gap_open)
            best = max(best, M[i][j])
    if best <= 0.0:
        return 0.0, 0, [], []
    ends = [(i, j) for i in range(1, n + 1) for j in range(1, m + 1) if M[i][j] == best]

    def walk(end, reverse):
        i, j = end
        state, pairs = "M", []
        while True:
            if state == "M":
                pairs.append((i - 1, j - 1))
                rest = M[i][j] - (match if a[i - 1] == b[j - 1] else mismatch)
                i, j = i - 1, j - 1
                options = [("stop", 0.0), ("M", M[i][j]), ("X", X[i][j]), ("Y", Y[i][j])]
            elif state == "X":
                rest = X[i][j]
                j -= 1
                options = [("M", M[i][j] - gap_open), ("X", X[i][j] - gap_extend), ("Y", Y[i][j] - gap_open)]
            else:
                rest = Y[i][j]
                i -= 1
                options = [("M", M[i][j] - gap_open), ("X", X[i][j] - gap_open), ("Y", Y[i][j] - gap_extend)]
            if reverse:
                options.reverse()
            state = next(name for name, value in options if value == rest)
            if state == "stop":
                return pairs[::-1]

    return best, len(ends), walk(ends[0], False), walk(ends[-1], True)


def pairs_of_blocks(blocks):
    """The (i, j) pairs of gap-free blocks ((a0, a1), (b0, b1))."""
    return [(i, j) for (a0, a1), (b0, b1) in blocks for i, j in zip(range(a0, a1), range(b0, b1))]
