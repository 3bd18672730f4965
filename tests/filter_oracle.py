"""Float64 CPU restatement of Hartigan's dip statistic and of the simulated-null p-value, used by the filter tests
only (the product never imports it).

Written from the published algorithm: Hartigan & Hartigan, "The dip test of unimodality", Ann. Statist. 13 (1985),
and Hartigan's AS 217 (Appl. Statist. 34, 1985), with the two known corrections (Maechler's termination test on
the modal interval and the symmetric formula for dx).  Indices are 1-based, as published."""
import numpy as np


def dip_full(x):
    """(dip, lo, hi) of a sorted 1-D array: the statistic, starting from 1/(2n) (0 for a constant sample or
    n < 2), and the 0-based ends of the modal interval.  The values are taken as float64."""
    n = len(x)
    if n < 2 or x[-1] == x[0]:
        return 0.0, 0, max(n - 1, 0)
    x = [0.0] + np.asarray(x, dtype=np.float64).tolist()
    mn = [0] * (n + 1)
    mj = [0] * (n + 1)
    # greatest convex minorant: mn[j] is the vertex before j on the hull of the points 1..j
    mn[1] = 1
    for j in range(2, n + 1):
        mn[j] = j - 1
        while True:
            mnj = mn[j]
            mnmnj = mn[mnj]
            if mnj == 1 or (x[j] - x[mnj]) * (mnj - mnmnj) < (x[mnj] - x[mnmnj]) * (j - mnj):
                break
            mn[j] = mnmnj
    # least concave majorant, from the right
    mj[n] = n
    for k in range(n - 1, 0, -1):
        mj[k] = k + 1
        while True:
            mjk = mj[k]
            mjmjk = mj[mjk]
            if mjk == n or (x[k] - x[mjk]) * (mjk - mjmjk) < (x[mjk] - x[mjmjk]) * (k - mjk):
                break
            mj[k] = mjmjk
    low, high = 1, n
    dipv = 1.0
    while True:
        gcm = [0, high]
        i = 1
        while gcm[i] > low:
            gcm.append(mn[gcm[i]])
            i += 1
        ig = l_gcm = i
        ix = ig - 1
        lcm = [0, low]
        i = 1
        while lcm[i] < high:
            lcm.append(mj[lcm[i]])
            i += 1
        ih = l_lcm = i
        iv = 2
        d = 0.0
        if l_gcm != 2 or l_lcm != 2:
            while True:
                gcmix = gcm[ix]
                lcmiv = lcm[iv]
                if gcmix > lcmiv:
                    gcmi1 = gcm[ix + 1]
                    dx = (lcmiv - gcmi1 + 1) - (x[lcmiv] - x[gcmi1]) * (gcmix - gcmi1) / (x[gcmix] - x[gcmi1])
                    iv += 1
                    if dx >= d:
                        d = dx
                        ig = ix + 1
                        ih = iv - 1
                else:
                    lcmiv1 = lcm[iv - 1]
                    dx = (x[gcmix] - x[lcmiv1]) * (lcmiv - lcmiv1) / (x[lcmiv] - x[lcmiv1]) - (gcmix - lcmiv1 - 1)
                    ix -= 1
                    if dx >= d:
                        d = dx
                        ig = ix + 1
                        ih = iv
                if ix < 1:
                    ix = 1
                if iv > l_lcm:
                    iv = l_lcm
                if gcm[ix] == lcm[iv]:
                    break
        else:
            d = 1.0
        if d < dipv:
            break
        dip_l = 0.0
        for j in range(ig, l_gcm):
            max_t = 1.0
            jb = gcm[j + 1]
            je = gcm[j]
            if je - jb > 1 and x[je] != x[jb]:
                c = (je - jb) / (x[je] - x[jb])
                for jj in range(jb, je + 1):
                    t = (jj - jb + 1) - (x[jj] - x[jb]) * c
                    if max_t < t:
                        max_t = t
            if dip_l < max_t:
                dip_l = max_t
        dip_u = 0.0
        for j in range(ih, l_lcm):
            max_t = 1.0
            jb = lcm[j]
            je = lcm[j + 1]
            if je - jb > 1 and x[je] != x[jb]:
                c = (je - jb) / (x[je] - x[jb])
                for jj in range(jb, je + 1):
                    t = (x[jj] - x[jb]) * c - (jj - jb - 1)
                    if max_t < t:
                        max_t = t
            if dip_u < max_t:
                dip_u = max_t
        dipnew = max(dip_u, dip_l)
        if dipv < dipnew:
            dipv = dipnew
        if low == gcm[ig] and high == lcm[ih]:
            break
        low = gcm[ig]
        high = lcm[ih]
    return dipv / (2 * n), low - 1, high - 1


def dip(x):
    return dip_full(x)[0]


def column_dips(X):
    """dip of every column of X (each column is sorted here, as float32 values taken to float64)."""
    X = np.asarray(X, dtype=np.float32)
    return np.array([dip(np.sort(X[:, c]).astype(np.float64)) for c in range(X.shape[1])])


_nulls = {}


def null_dips(m, samples=20000, seed=0):
    """Sorted dips of `samples` uniform samples of size m (NumPy RandomState(seed))."""
    key = (m, samples, seed)
    if key not in _nulls:
        rs = np.random.RandomState(seed)
        _nulls[key] = np.sort(np.array([dip(np.sort(rs.uniform(size=m))) for _ in range(samples)]))
    return _nulls[key]


def _null_block(args):
    m, count, seed = args
    rs = np.random.RandomState(seed)
    return [dip(np.sort(rs.uniform(size=m))) for _ in range(count)]


def _dip_of_sorted(col):
    return dip(col)


def _pool(workers):
    import multiprocessing as mp

    # spawn: the parent may hold a GPU context, which a forked child must not inherit
    return mp.get_context("spawn").Pool(workers)


def null_dips_parallel(m, samples, seed=0, workers=16, block=25):
    """As null_dips for large m, on several cores: block b of `block` samples is drawn from RandomState(seed + b)."""
    key = (m, samples, seed, "parallel", block)
    if key not in _nulls:
        jobs = [(m, min(block, samples - b), seed + b // block) for b in range(0, samples, block)]
        with _pool(workers) as pool:
            parts = pool.map(_null_block, jobs)
        _nulls[key] = np.sort(np.array([d for part in parts for d in part]))
    return _nulls[key]


def column_dips_parallel(X, workers=16):
    X = np.asarray(X, dtype=np.float32)
    cols = [np.sort(X[:, c]).astype(np.float64) for c in range(X.shape[1])]
    with _pool(workers) as pool:
        return np.array(pool.map(_dip_of_sorted, cols))


def pvalues(dips, null_sorted):
    """p = mean(null >= dip)."""
    below = np.searchsorted(null_sorted, np.asarray(dips, dtype=np.float64), side="left")
    return (null_sorted.size - below) / float(null_sorted.size)


def spearman(a, b):
    ra = np.argsort(np.argsort(a)).astype(np.float64)
    rb = np.argsort(np.argsort(b)).astype(np.float64)
    return float(np.corrcoef(ra, rb)[0, 1])
