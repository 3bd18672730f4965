"""The float32 streaming kernels -- dcv_col_stats, dcv_normalize (csrc/stats.hip), dcv_col_histogram (filter.hip),
dcv_project_linear (project.hip), dcv_lagged_cov (cov.hip) and the coordinate staging behind dcv_featurize / dcv_superpose
(stage.h) -- bit for bit against digests recorded on the MI355X (tests/golden/streaming_bits.json, written by
tests/golden/make_golden_streaming_bits.py from the commit named in that file).  The float64 oracles of
test_streaming_gpu.py, test_filter_gpu.py, test_compute_features_gpu.py and test_geometry_gpu.py allow rounding-level
drift; a change that only moves code must allow none.
Every result here is deterministic and independent of the CU count: the fixed-order float64 combine of col_stats depends
on n only, histogram counts are integers, the rows of project_linear do not depend on the grid and extrema are exact, the
chunks of lagged_cov follow from the row count, the frames of a staging tile from the atoms staged.  Each case is the
smallest shape that reaches the loop it is named for.  Run on the GPU box: python -m pytest tests -m gpu"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests import features_oracle as fo
from tests.test_compute_features_gpu import dense_buffer, planes_buffer
from tests.test_streaming_gpu import View, cov_inputs, dev, gpu_vectors, norm_inputs, project_inputs, quad_loads, rand_matrix

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streaming_bits.json")


def sha(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# (n, F, view, 16-byte loads, what the shape reaches)
COL_STATS = [
    (200, 2048, "contiguous", True, "VEC = 4, one row lane, 48 rows in the unrolled loop and 2 in the tail"),
    (1000, 100, "wide", True, "VEC = 4, 10 row lanes, idle threads"),
    (200, 257, "contiguous", False, "VEC = 1, second column pass of one column"),
    (131073, 8, "contiguous", True, "128 row lanes, tail loop only, blocks without rows"),
    (3, 12, "contiguous", True, "fewer rows than lanes"),
]
# 10 bins, edges from np.histogram_bin_edges per column
HISTOGRAM = [
    (1000, 72, "contiguous", True, "VEC = 4, second column block of 8, unrolled loop and tail"),
    (1000, 70, "contiguous", False, "VEC = 1, ragged second block"),
    (5000, 64, "offset", False, "scalar path because of the pointer, three row blocks"),
]
# (n, F, in place, 16-byte accesses)
NORMALIZE = [
    (513, 64, True, True, "rows form, in place: the switch test's shape"),
    (100, 36, False, True, "flat 16-byte form: ng = 9 does not divide 256"),
    (100, 7, False, False, "scalar form"),
]
PROJECT = [
    (129, 64, 3, "contiguous", True, "16-byte loads; one row into the third block iteration"),
    (65, 54, 3, "wide4", False, "scalar path"),
]
LAGGED_COV = [(2053, 130, 3, "wide4", "16-byte loaders"), (2053, 130, 3, "contiguous", "scalar loaders")]


def coordinate_defs(used):
    """distances, (sin, cos) torsions and torsions along the list of used atoms: [kind, a0, a1, a2, a3, column]"""
    defs, col = [], 0
    for i in range(len(used) - 1):
        defs.append([fo.DISTANCE, used[i], used[i + 1], 0, 0, col])
        col += 1
    for i in range(len(used) - 3):
        defs.append([fo.TORSION_SINCOS, used[i], used[i + 1], used[i + 2], used[i + 3], col])
        col += 2
    for i in range(0, len(used) - 3, 2):
        defs.append([fo.TORSION, used[i], used[i + 1], used[i + 2], used[i + 3], col])
        col += 1
    return np.asarray(defs, dtype=np.int32)


def coordinate_cases():
    """37 frames (two full staging tiles and five frames) of 50 atoms; atoms 3..40 fill their index range (ROWS form),
    every fifth atom does not (GATHER form); dense (n, A, 3) rows and the X / Y / Z planes of DCD records that start one
    word past a 16-byte boundary"""
    rng = np.random.Generator(np.random.PCG64(21))
    n, A = 37, 50
    ref = rng.standard_normal((A, 3)) * 4.0
    xyz = (ref + 0.3 * rng.standard_normal((n, A, 3))).astype(np.float32)
    for form, used in (("rows", list(range(3, 41))), ("gather", list(range(0, A, 5)))):
        for lay, (buf, layout) in (("dense", dense_buffer(xyz)), ("planes", planes_buffer(xyz, 3, cell=True))):
            yield f"{form}-{lay}", torch.from_numpy(buf).cuda(), layout, A, used, ref


def compute_digests():
    """{case: SHA-256 of the output's bytes}: what the library at hand computes"""
    from deep_cartograph_amd import hip

    out = {}
    for n, F, kind, vec, what in COL_STATS:
        v = View(rand_matrix(n, F, 31), kind)
        assert quad_loads(v.t) == vec, what
        out[f"col_stats-{n}x{F}-{kind}"] = sha(hip.col_stats_raw(v.t))
    for n, F, kind, vec, what in HISTOGRAM:
        X = rand_matrix(n, F, 32)
        v = View(X, kind)
        assert quad_loads(v.t) == vec, what
        edges = np.stack([np.histogram_bin_edges(X[:, c], bins=10) for c in range(F)]).astype(np.float32)
        counts = hip.col_histogram(v.t, dev(edges))
        assert int(counts.sum()) == n * F
        out[f"col_histogram-{n}x{F}-{kind}"] = sha(counts)
    for n, F, inplace, vec, what in NORMALIZE:
        X, m, r, _ = norm_inputs(n, F, seed=33)
        x = dev(X)
        assert quad_loads(x) == vec, what
        y = hip.normalize(x, dev(m), dev(r), out=x if inplace else None)
        assert (y is x) == inplace
        out[f"normalize-{n}x{F}"] = sha(y)
    for n, F, d, kind, vec, what in PROJECT:
        X, W, fm, fr, bias, cm, cr = project_inputs(n, F, d, seed=34)
        v = View(X, kind)
        assert quad_loads(v.t) == vec, what
        y, mm = hip.project_linear(v.t, dev(W), want_minmax=True, **gpu_vectors(fmean=fm, frange=fr, bias=bias, cvmean=cm, cvrange=cr))
        out[f"project_linear-{n}x{F}-{kind}-out"], out[f"project_linear-{n}x{F}-{kind}-minmax"] = sha(y), sha(mm)
    for P, F, lag, kind, what in LAGGED_COV:
        X, sh = cov_inputs(P, F, lag, True, seed=35)
        out[f"lagged_cov-{P}x{F}-lag{lag}-{kind}"] = sha(hip.lagged_cov_raw(View(X, kind).t, P, lag, dev(sh)))
    for tag, buf, layout, A, used, ref in coordinate_cases():
        out[f"featurize-{tag}"] = sha(hip.featurize(buf, coordinate_defs(used), A, strides=layout))
        got = hip.superpose(buf, A, used, ref[used], sel=used, sel_ref=ref[used], strides=layout, want=("transform", "aligned", "moments"))
        for k in ("transform", "aligned", "moments"):
            out[f"superpose-{tag}-{k}"] = sha(got[k])
    return out


def test_streaming_results_bit_equal_to_the_recorded_commit():
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = compute_digests()
    assert sorted(got) == sorted(golden["sha256"])
    differ = [k for k in sorted(got) if got[k] != golden["sha256"][k]]
    print(f"{len(got)} results against commit {golden['commit']}: {len(differ)} differ {differ}")
    assert not differ
