"""The float32 streaming kernels -- dcv_col_stats, dcv_normalize (csrc/stats.hip), dcv_col_histogram (filter.hip),
dcv_project_linear (project.hip), dcv_lagged_cov (cov.hip), the coordinate staging behind dcv_featurize / dcv_superpose
(stage.h) and the coordinate kernels that share coords.h (dcv_transform_frames, dcv_interpolate, dcv_xtc_decode,
dcv_xtc_encode / dcv_xtc_pack) -- bit for bit against digests recorded on the MI355X (tests/golden/streaming_bits.json, written by
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

from deep_cartograph_amd import _lib
from tests import features_oracle as fo
from tests import xtc_oracle as xo
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


def strided_buffer(xyz, pre=0):
    """A layout that is neither planes nor dense: atom stride 4 (a NaN behind every atom), component stride 1"""
    n, A = xyz.shape[:2]
    buf = np.full(pre + n * A * 4, np.nan, dtype=np.float32)
    buf[pre:].reshape(n, A, 4)[:, :, :3] = xyz
    return buf, (n, pre, 4 * A, 4, 1)


FORMS = {"dense": dense_buffer, "planes": lambda xyz: planes_buffer(xyz, 3, cell=True), "strided": strided_buffer}


def frames_of(n, A=50, seed=22):
    rng = np.random.Generator(np.random.PCG64(seed))
    ref = rng.standard_normal((A, 3)) * 4.0
    return ref, (ref + 0.3 * rng.standard_normal((n, A, 3))).astype(np.float32)


def source(xyz, form):
    buf, layout = FORMS[form](xyz)
    return torch.from_numpy(buf).cuda(), layout


def target(n, A, form):
    """a NaN-filled buffer of the form and its out_strides: the digest of the whole buffer also pins what stays untouched"""
    buf, layout = FORMS[form](np.zeros((n, A, 3), dtype=np.float32))
    buf[:] = np.nan
    return torch.from_numpy(buf).cuda(), layout[1:]


def xtc_stream(n, A, seed=23):
    """(file bytes, descriptors relative to them) of n frames from the structural encoder: eight groups with runs of up to
    three small atoms, then single atoms; raw frames for A <= 9"""
    rng = np.random.Generator(np.random.PCG64(seed))
    data = []
    for f in range(n):
        if A <= 9:
            data.append(xo.encode_raw_frame(rng.uniform(-5.0, 5.0, size=(A, 3)), step=f, time=float(f)))
            continue
        script = [(int(r), 0, False) for r in rng.integers(0, 4, size=8)]
        script += [(0, 0, False)] * (A - sum(1 + r for r, _, _ in script))
        smallidx = int(rng.integers(14, 30))
        centre, half = rng.integers(-2000, 8000, size=3), rng.integers(30, 6000, size=3)
        ints = xo.make_ints(rng, script, smallidx, centre - half, centre + half)
        data.append(xo.encode_frame(ints, script, smallidx, step=f, time=float(f)))
    data = b"".join(data)
    desc = np.zeros(n, dtype=_lib.XTC_FRAME_DTYPE)
    for d, fr in zip(desc, xo.frames(data)):
        d["offset"], d["raw"] = fr["offset"], int(fr["raw"])
        if not fr["raw"]:
            d["nbytes"], d["smallidx"], d["precision"], d["minint"], d["maxint"] = fr["nbytes"], fr["smallidx"], fr["precision"], fr["minint"], fr["maxint"]
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda(), desc


def coordinate_kernel_digests(hip, out):
    """dcv_transform_frames, dcv_interpolate, dcv_xtc_decode, dcv_xtc_encode / dcv_xtc_pack: the smallest shapes that reach
    each loop, through every layout form (dense rows, DCD planes, neither)"""
    n, A = 37, 50
    ref, xyz = frames_of(n)
    fit = list(range(3, 41))
    T = hip.superpose(source(xyz, "dense")[0], A, fit, ref[fit], strides=FORMS["dense"](xyz)[1], want=("transform",))["transform"]
    for fin in FORMS:       # 37 frames x 13 or 14 groups: two workgroups, frames that share a wave
        for fout in FORMS:
            (buf, lay), (o, ostr) = source(xyz, fin), target(n, A, fout)
            out[f"transform_frames-{fin}-{fout}"] = sha(hip.transform_frames(buf, A, T, strides=lay, out=o, out_strides=ostr))
    (buf, lay), (o, ostr) = source(xyz[:, :3], "planes"), target(n, 3, "dense")   # fewer than four atoms: no 16-byte form
    out["transform_frames-3atoms-planes-dense"] = sha(hip.transform_frames(buf, 3, T, strides=lay, out=o, out_strides=ostr))

    t = np.arange(2 * n - 1) / 2.0
    sel = list(range(0, A, 5))
    noise = torch.from_numpy(np.random.Generator(np.random.PCG64(24)).standard_normal((t.size, A, 3)) * 0.01).cuda()
    for kind in ("pchip", "makima"):
        buf, lay = source(xyz, "dense")
        out[f"interpolate-{kind}-dense-dense"] = sha(hip.interpolate(buf, A, t, kind=kind, strides=lay))
        (buf, lay), (o, ostr) = source(xyz, "planes"), target(t.size, len(sel), "planes")
        out[f"interpolate-{kind}-planes-sel-planes"] = sha(hip.interpolate(buf, A, t, kind=kind, sel=sel, strides=lay, out=o, out_strides=ostr))
        (buf, lay), (o, ostr) = source(xyz, "strided"), target(t.size, A, "planes")   # planes out, yet lanes along the noise
        out[f"interpolate-{kind}-strided-noise-planes"] = sha(hip.interpolate(buf, A, t, kind=kind, strides=lay, noise=noise, out=o, out_strides=ostr))

    n = 70   # a full wave and a partial one
    data, desc = xtc_stream(n, A)
    got, status = hip.xtc_decode(data, desc, A, return_status=True)
    assert not status.any()
    out["xtc_decode-50atoms-dense"] = sha(got)
    o, ostr = target(n, A, "planes")
    got, status = hip.xtc_decode(data, desc, A, out=o, out_strides=ostr, return_status=True)
    assert not status.any()
    out["xtc_decode-50atoms-planes"] = sha(got)
    data, desc = xtc_stream(n, 9)
    out["xtc_decode-9atoms-dense"] = sha(hip.xtc_decode(data, desc, 9))

    _, xyz = frames_of(n, seed=25)
    index = np.arange(n)[::-1].copy()
    index[5] = index[4]   # a repeat
    for tag, atoms, form, frames in (("50atoms-dense", A, "dense", None), ("50atoms-planes-indexed", A, "planes", index), ("9atoms-dense", 9, "dense", None)):
        buf, lay = source(xyz[:, :atoms], form)
        slots, desc, status = hip.xtc_encode_slots(buf, atoms, strides=lay, frames=frames)
        status = status.cpu().numpy()
        assert not status.any()
        slots_h, slot = slots.cpu().numpy(), slots.numel() // n
        assert np.array_equal(desc["offset"], slot * np.arange(n))
        length = np.full(n, 12 * atoms) if atoms <= 9 else desc["nbytes"]
        out[f"xtc_encode-{tag}-slots"] = sha(np.concatenate([slots_h[f * slot: f * slot + length[f]] for f in range(n)]))
        out[f"xtc_encode-{tag}-desc"], out[f"xtc_encode-{tag}-status"] = sha(desc), sha(status)
        offsets, image_bytes = hip.xtc_image_offsets(desc, status, atoms)
        step = np.arange(n, dtype=np.int32)
        out[f"xtc_encode-{tag}-image"] = sha(hip.xtc_pack(slots, desc, offsets, atoms, step, step.astype(np.float32), image_bytes=image_bytes))


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
    coordinate_kernel_digests(hip, out)
    return out


def test_streaming_results_bit_equal_to_the_recorded_commit():
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = compute_digests()
    assert sorted(got) == sorted(golden["sha256"])
    differ = [k for k in sorted(got) if got[k] != golden["sha256"][k]]
    print(f"{len(got)} results against commit {golden['commit']}: {len(differ)} differ {differ}")
    assert not differ
