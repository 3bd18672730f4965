"""dcv_featurize_project on the MI355X against the float64 oracle (tests/project_trajectory_oracle.py) within its derived
bound, on synthetic coordinates at the smallest shapes that reach each path: record counts around the lanes and the
pass length, every output width, every subset of the optional vectors, every record kind, the coordinate layouts and
staging forms of dcv_featurize, strided output, exact extrema, chunk independence and the error codes of the C-ABI."""
import itertools

import numpy as np
import pytest
import torch

from tests import project_trajectory_oracle as po

pytestmark = pytest.mark.gpu

D, SC, T = 0, 1, 2
N, A = 37, 23       # two full tiles of 16 frames and a ragged one
ratios = {}         # worst error / bound per test, printed by each


# ------------------------------------------------------------------------------------------------ helpers
def random_coordinates(n, A, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.standard_normal((n, A, 3)) * 12).astype(np.float32)


def random_records(A, n_rec, seed, kinds=("dist", "both", "sin", "tor", "cos")):
    """(records, F): the kinds in turn on random atoms (distinct inside a record); the feature indices are a random
    permutation, so feature order and record order differ."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rec, n_values = [], 0
    for r in range(n_rec):
        kind = kinds[r % len(kinds)]
        atoms = rng.choice(A, size=4, replace=False).tolist()
        if kind == "dist":
            rec.append([D, atoms[0], atoms[1], 0, 0, n_values, -1, 0])
        elif kind == "tor":
            rec.append([T, *atoms, n_values, -1, 0])
        elif kind == "sin":
            rec.append([SC, *atoms, n_values, -1, 0])
        elif kind == "cos":
            rec.append([SC, *atoms, -1, n_values, 0])
        else:
            rec.append([SC, *atoms, n_values, n_values + 1, 0])
            n_values += 1
        n_values += 1
    rec = np.asarray(rec, dtype=np.int32)
    perm = rng.permutation(n_values).astype(np.int32)
    for col in (5, 6):
        rec[:, col] = np.where(rec[:, col] >= 0, perm[np.maximum(rec[:, col], 0)], -1)
    return rec, n_values


def model(F, d, seed, use=("norm", "bias", "cvnorm")):
    """W with one zero row (two when there are enough features) and the optional vectors named in `use`."""
    rng = np.random.Generator(np.random.PCG64(seed))
    W = rng.standard_normal((F, d)).astype(np.float32)
    W[F // 2] = 0
    if F > 4:
        W[0] = 0
    v = {}
    if "norm" in use:
        v["fmean"] = (rng.standard_normal(F) * 0.4).astype(np.float32)
        v["frange"] = rng.uniform(0.5, 2.0, F).astype(np.float32)
    if "bias" in use:
        v["bias"] = rng.standard_normal(d).astype(np.float32)
    if "cvnorm" in use:
        v["cvmean"] = rng.standard_normal(d).astype(np.float32)
        v["cvrange"] = (rng.uniform(0.5, 3.0, d) * np.where(np.arange(d) == d - 1, -1, 1)).astype(np.float32)   # one negative range
    return W, v


def dense_buffer(xyz, pre=0):
    n, A = xyz.shape[:2]
    buf = np.full(pre + xyz.size, np.nan, dtype=np.float32)
    buf[pre:] = xyz.reshape(-1)
    return buf, (n, pre, 3 * A, 3, 1)


def planes_buffer(xyz, pre=0, cell=False):
    """DCD frame records in one flat buffer (markers, unit cell and padding are NaN), as tests/test_compute_features_gpu.py."""
    n, A = xyz.shape[:2]
    words = (14 if cell else 0) + 3 * (A + 2)
    buf = np.full(pre + n * words, np.nan, dtype=np.float32)
    for f in range(n):
        base = pre + f * words + (14 if cell else 0)
        for c in range(3):
            buf[base + c * (A + 2) + 1: base + c * (A + 2) + 1 + A] = xyz[f, :, c]
    return buf, (n, pre + (14 if cell else 0) + 1, words, 1, A + 2)


def run(buf, layout, rec, A, W, vectors, every=1, unit=0.1, out=None):
    from deep_cartograph_amd import hip

    n, off, fs, as_, cs = layout
    lay = ((n + every - 1) // every, off, fs * every, as_, cs)
    dev = {k: torch.from_numpy(v).cuda() for k, v in vectors.items()}
    got, mm = hip.featurize_project(torch.from_numpy(buf).cuda(), rec, A, W.shape[0], torch.from_numpy(W).cuda(), strides=lay, unit=unit,
                                    want_minmax=True, out=out, **dev)
    return got.cpu().numpy(), mm.cpu().numpy()


def check(got, mm, ref, bound, tag):
    assert got.shape == ref.shape and got.dtype == np.float32 and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(err / bound))
    ratios[tag] = ratio
    print(f"featurize_project {tag}: worst error / bound {ratio:.3f}, worst error {err.max():.2e}")
    assert np.all(err <= bound), tag
    assert np.array_equal(mm, np.stack([got.min(0), got.max(0)])), tag


@pytest.fixture(scope="module")
def xyz():
    return random_coordinates(N, A, 7)


# ------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 8, 9, 16])
@pytest.mark.parametrize("n_rec", [1, 3, 65, 300])
def test_record_counts_and_widths(xyz, n_rec, d):
    """One lane, a partial wave, across a wave boundary and the first pass (65 records hold 78 values, 300 hold 360:
    three passes of 128), at every compiled width D = 2, 4, 8, 16 and one below each; all optional vectors given."""
    rec, F = random_records(A, n_rec, 100 + n_rec)
    W, v = model(F, d, 10 * n_rec + d)
    ref, bound, _ = po.featurize_project(xyz, rec, W, **v)
    got, mm = run(*dense_buffer(xyz), rec, A, W, v)
    check(got, mm, ref, bound, f"n_rec={n_rec} F={F} d={d}")


@pytest.mark.parametrize("use", [c for k in range(4) for c in itertools.combinations(("norm", "bias", "cvnorm"), k)],
                         ids=lambda names: "+".join(names) or "none")
def test_every_subset_of_the_optional_vectors(xyz, use):
    rec, F = random_records(A, 65, 3)
    W, v = model(F, 3, 17, use)
    ref, bound, _ = po.featurize_project(xyz, rec, W, **v)
    got, mm = run(*planes_buffer(xyz, 1), rec, A, W, v)
    check(got, mm, ref, bound, "vectors: " + ("+".join(use) or "none"))


@pytest.mark.parametrize("kinds", [("sin",), ("cos",), ("both",), ("tor",), ("dist",), ("dist", "both", "sin", "tor", "cos")], ids="+".join)
def test_record_kinds(xyz, kinds):
    rec, F = random_records(A, 70, 5, kinds)     # 70 records of both: 140 values, two passes
    W, v = model(F, 2, 23)
    ref, bound, _ = po.featurize_project(xyz, rec, W, **v)
    got, mm = run(*dense_buffer(xyz), rec, A, W, v)
    check(got, mm, ref, bound, "kinds: " + "+".join(kinds))


def test_collinear_and_coincident_atoms_and_a_zero_row():
    """(sin, cos) = (0, 1) and a distance of exactly 0 go through the product unchanged: without normalisation the result
    is the float32 of the float64 sum of W's cosine rows, exactly; a feature whose row of W is zero does not count."""
    xyz = np.zeros((3, 8, 3), dtype=np.float32)
    xyz[:, 0:4] = [[0, 0, 0], [1, 1, 1], [2, 2, 2], [5, 5, 5]]            # collinear along a diagonal
    xyz[:, 4:8] = [[1.5, 0, 0], [0, 0, 0], [0, 0, 1.25], [0, 2.5, 1.25]]  # a right angle
    xyz[1] *= np.float32(3.7)
    xyz[2] += np.float32(11.3)
    rec = np.asarray([[SC, 0, 1, 2, 3, 0, 1, 0], [D, 2, 2, 0, 0, 2, -1, 0], [SC, 4, 4, 4, 4, -1, 3, 0], [SC, 5, 5, 6, 7, 4, -1, 0],
                      [T, 0, 1, 2, 3, 5, -1, 0], [SC, 4, 5, 6, 7, 6, 7, 0]], dtype=np.int32)
    W, _ = model(8, 3, 2, use=())
    W[6:8] = 0                                   # the only features that are not exactly 0 or 1
    f = po.features(xyz, rec, 8)
    assert np.array_equal(f[:, :6], np.tile([0.0, 1.0, 0.0, 1.0, 0.0, 0.0], (3, 1)))
    exact = (W[1].astype(np.float64) + W[3].astype(np.float64)).astype(np.float32)
    for buf, layout in (dense_buffer(xyz), planes_buffer(xyz, 1)):
        got, mm = run(buf, layout, rec, 8, W, {})
        assert np.array_equal(got, np.tile(exact, (3, 1)))
        assert np.array_equal(mm, np.stack([exact, exact]))
    W2, v = model(8, 3, 4)
    ref, bound, _ = po.featurize_project(xyz, rec, W2, **v)
    check(*run(*dense_buffer(xyz), rec, 8, W2, v), ref, bound, "degenerate geometry")


# ------------------------------------------------------------------------------------------------ 2. layouts and chunks
def test_layouts_strides_and_chunks_give_the_same_bits(xyz):
    """Dense rows and DCD planes with and without the unit-cell block at every alignment of the base pointer, every third
    frame through the frame stride, and frames [5:29) in a call of their own: a frame's result depends on nothing but its
    own coordinates."""
    rec, F = random_records(A, 65, 11)
    W, v = model(F, 4, 31)
    ref, bound, _ = po.featurize_project(xyz, rec, W, **v)
    first, mm = run(*dense_buffer(xyz), rec, A, W, v)
    check(first, mm, ref, bound, "layouts")
    for pre in range(4):
        for buf, layout in (dense_buffer(xyz, pre), planes_buffer(xyz, pre), planes_buffer(xyz, pre, cell=True)):
            got, _ = run(buf, layout, rec, A, W, v)
            assert np.array_equal(got, first), f"pre={pre} layout={layout}"
            got, mm = run(buf, layout, rec, A, W, v, every=3)
            assert got.shape[0] == 13 and np.array_equal(got, first[::3]), f"stride 3, pre={pre} layout={layout}"
            assert np.array_equal(mm, np.stack([first[::3].min(0), first[::3].max(0)]))
    for buf, layout in (dense_buffer(xyz[5:29], 1), planes_buffer(xyz[5:29], 2)):
        got, _ = run(buf, layout, rec, A, W, v)
        assert np.array_equal(got, first[5:29])
    view = torch.from_numpy(xyz).cuda()[::3]     # a strided (n, A, 3) tensor, no explicit layout
    from deep_cartograph_amd import hip
    dev = {k: torch.from_numpy(x).cuda() for k, x in v.items()}
    got, none = hip.featurize_project(view, rec, A, F, torch.from_numpy(W).cuda(), **dev)
    assert none is None and np.array_equal(got.cpu().numpy(), first[::3])


@pytest.mark.parametrize("form", ["gather", "rows"])
def test_many_atoms_gathered_or_staged_as_rows(form):
    """6 frames of 2000 atoms.  Twelve named atoms are gathered; a contiguous named range of 1900 atoms is staged as
    rows, 22.8 KB per frame, which leaves room for two frames per workgroup."""
    n, A = 6, 2000
    xyz = random_coordinates(n, A, 44)
    if form == "gather":
        atoms = np.asarray([3, 50, 200, 299, 700, 701, 999, 1200, 1500, 1777, 1998, 1999])
        rng = np.random.Generator(np.random.PCG64(1))
        rec = np.asarray([[SC, *rng.choice(atoms, 4, replace=False), 2 * r, 2 * r + 1, 0] for r in range(6)]
                         + [[D, atoms[r], atoms[11 - r], 0, 0, 12 + r, -1, 0] for r in range(6)], dtype=np.int32)
        F = 18
    else:
        lo = np.arange(50, 1000)
        rec = np.stack([np.full(950, D), lo, lo + 950, np.zeros(950), np.zeros(950), np.arange(950)[::-1], np.full(950, -1),
                        np.zeros(950)], axis=1).astype(np.int32)
        F = 950
    W, v = model(F, 2, 8)
    ref, bound, _ = po.featurize_project(xyz, rec, W, **v)
    first = None
    for buf, layout in (dense_buffer(xyz, 1), planes_buffer(xyz, 2)):
        got, mm = run(buf, layout, rec, A, W, v)
        check(got, mm, ref, bound, f"{form} {layout[3:]}")
        first = got if first is None else first
        assert np.array_equal(got, first)


def test_output_view_of_a_wider_buffer(xyz):
    rec, F = random_records(A, 20, 2)
    W, v = model(F, 5, 3)
    ref, bound, _ = po.featurize_project(xyz, rec, W, **v)
    big = torch.full((N + 2, 13), float("nan"), dtype=torch.float32, device="cuda")
    out = big[1:N + 1, 4:9]
    assert out.stride(0) == 13
    got, mm = run(*dense_buffer(xyz), rec, A, W, v, out=out)
    check(got, mm, ref, bound, "ldo 13")
    host = big.cpu().numpy()
    assert np.array_equal(host[1:N + 1, 4:9], got)
    host[1:N + 1, 4:9] = np.nan
    assert np.isnan(host).all()                  # nothing outside the view was written


def test_no_frames():
    from deep_cartograph_amd import hip

    rec = np.asarray([[SC, 0, 1, 2, 3, 0, 1, 0]], dtype=np.int32)
    out, mm = hip.featurize_project(torch.zeros(0, 6, 3, device="cuda"), rec, 6, 2, torch.ones(2, 3, device="cuda"), want_minmax=True)
    assert tuple(out.shape) == (0, 3) and out.dtype == torch.float32 and tuple(mm.shape) == (2, 3)


# ------------------------------------------------------------------------------------------------ 3. the C-ABI's refusals
def test_error_codes_launch_nothing():
    """Every DCV_EINVAL / DCV_ENOMEM case of include/dcv.h returns its code with the output still NaN; n_frames = 0 is OK."""
    from deep_cartograph_amd import _lib

    lib = _lib.load()
    n, A, F, d = 10, 6, 4, 3
    xyz = torch.from_numpy(random_coordinates(n, A, 1)).cuda()
    out = torch.full((n, d), float("nan"), dtype=torch.float32, device="cuda")
    W = torch.ones(F, d, device="cuda")
    vec = torch.ones(16, device="cuda")
    good = [[D, 0, 1, 0, 0, 0, -1, 0], [SC, 0, 1, 2, 3, 2, 1, 0], [T, 1, 2, 3, 4, 3, -1, 0]]
    need = lib.dcv_featurize_project_workspace(n, A, 3, F, d)
    assert need > 0
    ws = torch.zeros(need + 4096, dtype=torch.uint8, device="cuda")

    def call(rec=good, n=n, A=A, F=F, d=d, ldo=d, strides=(3 * A, 3, 1), fmean=vec, frange=vec, ws_bytes=None, coords=xyz):
        r = np.ascontiguousarray(rec, dtype=np.int32)
        need_now = lib.dcv_featurize_project_workspace(n, A, len(r), F, d)
        big = torch.zeros(max(need_now, 16), dtype=torch.uint8, device="cuda") if need_now > ws.numel() else ws
        rc = lib.dcv_featurize_project(coords.data_ptr(), n, *strides, A, r.ctypes.data, len(r), F, 0.1,
                                       None if fmean is None else fmean.data_ptr(), None if frange is None else frange.data_ptr(),
                                       W.data_ptr(), d, None, None, None, out.data_ptr(), ldo, None, big.data_ptr(),
                                       need_now if ws_bytes is None else ws_bytes, None)
        torch.cuda.synchronize()
        return rc

    rest = good[1:]
    cases = {
        "kind": (dict(rec=[[3, 0, 1, 0, 0, 0, -1, 0]] + rest), -1, "kind"),
        "atom index": (dict(rec=[[D, 0, A, 0, 0, 0, -1, 0]] + rest), -1, "atom"),
        "negative atom": (dict(rec=good[:2] + [[T, 1, -1, 3, 4, 3, -1, 0]]), -1, "atom"),
        "feature index": (dict(rec=[[D, 0, 1, 0, 0, F, -1, 0]] + rest), -1, "features"),
        "feature below -1": (dict(rec=[good[0], [SC, 0, 1, 2, 3, 2, -2, 0], good[2]]), -1, "features"),
        "no feature": (dict(rec=good + [[SC, 0, 1, 2, 4, -1, -1, 0]]), -1, "features"),
        "second feature of a distance": (dict(rec=[[D, 0, 1, 0, 0, 0, 1, 0], [SC, 0, 1, 2, 3, 2, -1, 0], good[2]]), -1, "one value"),
        "feature written twice": (dict(rec=good + [[D, 2, 3, 0, 0, 1, -1, 0]]), -1, "feature 1 is written by 2"),
        "feature never written": (dict(rec=good[:2], F=4), -1, "feature 3 is written by 0"),
        "d = 0": (dict(d=0), -1, "d=0"),
        "d = 17": (dict(d=17), -1, "d=17"),
        "ldo": (dict(ldo=d - 1), -1, "ldo"),
        "fmean alone": (dict(frange=None), -1, "fmean/frange"),
        "frange alone": (dict(fmean=None), -1, "fmean/frange"),
        "atom stride": (dict(strides=(3 * A, 0, 1)), -1, "strides"),
        "negative frame stride": (dict(strides=(-1, 3, 1)), -1, "strides"),
        "workspace": (dict(ws_bytes=need - 1), -3, "workspace"),
    }
    for what, (kw, code, message) in cases.items():
        assert call(**kw) == code, what
        error = lib.dcv_last_error().decode()
        assert error.startswith("dcv_featurize_project") and message in error, (what, error)
        assert bool(torch.isnan(out).all()), f"{what}: the output was written"
    # one frame of 5462 staged atoms exceeds the LDS of a workgroup
    big_A = 5462
    pairs = np.stack([np.full(big_A // 2, D), np.arange(0, big_A, 2), np.arange(1, big_A, 2), np.zeros(big_A // 2), np.zeros(big_A // 2),
                      np.arange(big_A // 2), np.full(big_A // 2, -1), np.zeros(big_A // 2)], axis=1).astype(np.int32)
    wide_W = torch.ones(big_A // 2, d, device="cuda")
    coords = torch.zeros(2, big_A, 3, device="cuda")
    r = np.ascontiguousarray(pairs)
    big_ws = torch.zeros(lib.dcv_featurize_project_workspace(2, big_A, len(r), len(r), d), dtype=torch.uint8, device="cuda")
    rc = lib.dcv_featurize_project(coords.data_ptr(), 2, 3 * big_A, 3, 1, big_A, r.ctypes.data, len(r), len(r), 0.1, None, None,
                                   wide_W.data_ptr(), d, None, None, None, out.data_ptr(), d, None, big_ws.data_ptr(), big_ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == -1 and "LDS" in lib.dcv_last_error().decode() and bool(torch.isnan(out).all())
    assert call(n=0) == 0 and bool(torch.isnan(out).all())
    assert call() == 0 and bool(torch.isfinite(out).all())
    assert lib.dcv_featurize_project_workspace(n, 0, 3, F, d) == 0 and lib.dcv_featurize_project_workspace(n, A, 3, F, 17) == 0
