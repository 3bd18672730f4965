"""traj_augmentation on the device: hip.interpolate (csrc/interp.hip) against scipy's PchipInterpolator and
Akima1DInterpolator(method="makima") -- the classes the reference calls -- and the tool and workflow on top of it.

Tolerance (tests/augmentation_oracle.tolerance): both sides evaluate the same cubic in float64 from slopes that are
exact and round once to float32, so |out - ref| <= spacing(float32(|ref|)) + 2^-43 Ymax per element, Ymax the largest
|y| of the column.  Every finite element is compared; NaN positions must match exactly."""
import json
import os

import numpy as np
import pytest
import torch

from tests import augmentation_oracle as ao

pytestmark = pytest.mark.gpu

N_SEL = (1, 5, 67, 700)
SEL_MODES = ("contiguous", "sparse", "shuffled", "none")
IN_LAYOUTS = ("dense", "dcd_odd_offset", "dcd_two_records")
OUT_LAYOUTS = ("dense", "dcd")


def _selection(mode, n_sel, rng):
    """(n_atoms, sel or None)"""
    if mode == "none":
        return n_sel, None
    if mode == "contiguous":
        return n_sel + 7, np.arange(3, 3 + n_sel)
    n_atoms = 2 * n_sel + 3
    sel = np.sort(rng.choice(n_atoms, n_sel, replace=False))
    return n_atoms, (rng.permutation(sel) if mode == "shuffled" else sel)


def _upload(y, layout):
    """(device tensor, strides argument of hip.interpolate) holding y (n, A, 3) in one of the input layouts."""
    n, A = y.shape[:2]
    if layout == "dense":
        return torch.from_numpy(y).cuda(), None
    words = 3 * (A + 2)
    step = 2 if layout == "dcd_two_records" else 1      # every second record holds a frame, the others NaN
    offset = 7 if layout == "dcd_odd_offset" else 4     # 7: an odd float offset, the X plane starts 4 bytes past a 16-byte boundary at best
    buf = np.full(offset + n * step * words + 3, np.nan, dtype=np.float32)
    rec = buf[offset:offset + n * step * words].reshape(n, step, 3, A + 2)
    rec[:, 0, :, 1:A + 1] = y.transpose(0, 2, 1)
    return torch.from_numpy(buf).cuda(), (n, offset + 1, step * words, 1, A + 2)


def _run(y, t, kind, sel, in_layout, out_layout, extrapolate=True, noise=None):
    """hip.interpolate through the given layouts -> (n_out, n_sel, 3) float32 on the host.  The output buffer is poisoned
    with NaN; everything the call must not touch (a guard band on both sides, the record markers between the planes) is
    checked to be NaN still."""
    from deep_cartograph_amd import hip

    n_atoms = y.shape[1]
    n_sel = n_atoms if sel is None else len(sel)
    n_out = len(t)
    buf, strides = _upload(y, in_layout)
    noise_d = None if noise is None else torch.from_numpy(noise).cuda()
    guard = 37
    if out_layout == "dense":
        off, fs, as_, cs = guard, 3 * n_sel, 3, 1
        total = guard + 3 * n_sel * n_out + guard
    else:
        off, fs, as_, cs = guard + 1, 3 * (n_sel + 2), 1, n_sel + 2
        total = guard + 3 * (n_sel + 2) * n_out + guard
    out = torch.full((total,), float("nan"), dtype=torch.float32, device="cuda")
    got = hip.interpolate(buf, n_atoms, t, kind=kind, sel=sel, strides=strides, extrapolate=extrapolate, noise=noise_d, out=out,
                          out_strides=(off, fs, as_, cs))
    assert got is out
    flat = out.cpu().numpy()
    idx = off + fs * np.arange(n_out)[:, None, None] + as_ * np.arange(n_sel)[None, :, None] + cs * np.arange(3)[None, None, :]
    written = np.zeros(total, dtype=bool)
    written[idx] = True
    assert np.isnan(flat[~written]).all(), "the call wrote outside its output elements (guard band / record markers)"
    return flat[idx]


CASES = []
for _kind in ("pchip", "makima"):
    for _n in (2, 3, 4, 5, 7, 40):
        if (_kind, _n) == ("makima", 2):
            continue
        for _ratio in (0.3, 1, 60):
            _i = len(CASES)
            CASES.append((_kind, _n, _ratio, N_SEL[_i % 4], SEL_MODES[(_i // 4 + _i) % 4], IN_LAYOUTS[_i % 3], OUT_LAYOUTS[(_i // 3 + _i) % 2]))
# every value of every axis is reached, and the large selection meets both output layouts
assert {c[3] for c in CASES} == set(N_SEL) and {c[4] for c in CASES} == set(SEL_MODES) and {c[5] for c in CASES} == set(IN_LAYOUTS)
assert {(c[3], c[6]) for c in CASES} >= {(700, "dense"), (700, "dcd"), (1, "dense"), (1, "dcd")}


def _times(n, ratio):
    """About ratio * n times: a regular grid from half a frame below 0 to half a frame above n - 1, plus exact knots,
    duplicates and the two ends."""
    grid = np.linspace(-0.5, n - 0.5, max(1, int(round(ratio * n))))
    extra = [0.0, 0.0, float(n - 1), float(n - 1), 1.0, -0.25, n - 0.75, float(n // 2)]
    return np.sort(np.concatenate([grid, extra]))


@pytest.mark.parametrize("kind,n,ratio,n_sel,sel_mode,in_layout,out_layout", CASES)
def test_interpolate_against_scipy(kind, n, ratio, n_sel, sel_mode, in_layout, out_layout):
    rng = np.random.default_rng(1000 * n + n_sel)
    n_atoms, sel = _selection(sel_mode, n_sel, rng)
    chosen = np.arange(n_atoms) if sel is None else sel
    y = ao.crafted(n, n_atoms, 17 * n + n_sel, special_atoms=(chosen[0], chosen[-1]) if n_sel > 1 else (chosen[0],))
    y_sel = y[:, chosen]
    if kind == "makima":
        ao.makima_margin(y_sel)
    t = _times(n, ratio)
    ref = ao.scipy_interpolate(y_sel, t, kind, True)
    got = _run(y, t, kind, sel, in_layout, out_layout)
    ao.assert_close(got, ref, y_sel, f"{kind} n={n} n_out={len(t)} n_sel={n_sel} {sel_mode} {in_layout}->{out_layout}")
    assert np.isfinite(got).all()


@pytest.mark.parametrize("kind", ["pchip", "makima"])
def test_long_trajectory_and_times_that_skip_knots(kind):
    """Paths the small shapes do not reach: 300 knots are more than one run of the pass that finds makima's G, and times
    that jump over six knots or more reload the window instead of walking it."""
    n, n_atoms = 300, 5
    y = ao.crafted(n, n_atoms, 77, special_atoms=(0, 4))
    if kind == "makima":
        ao.makima_margin(y)
    t = np.sort(np.concatenate([[0.2, 0.4, 9.7, 9.9, 15.9, 30.1, 38.5, 250.0, 298.2, 299.0, 299.4], np.linspace(40.0, 44.0, 90)]))
    got = _run(y, t, kind, None, "dcd_odd_offset", "dense")
    ao.assert_close(got, ao.scipy_interpolate(y, t, kind, True), y, f"{kind}: 300 knots, times that skip knots")


@pytest.mark.parametrize("kind", ["pchip", "makima"])
def test_without_extrapolation_nan_exactly_where_scipy(kind):
    n, n_atoms = 7, 67
    y = ao.crafted(n, n_atoms, 3, special_atoms=(0, 66))
    t = _times(n, 5)
    ref = ao.scipy_interpolate(y, t, "makima", False)   # scipy's default Akima: NaN outside [0, n - 1]
    assert np.array_equal(np.isnan(ref).all(axis=(1, 2)), (t < 0) | (t > n - 1)) and np.isnan(ref).any() and not np.isnan(ref).all()
    if kind == "pchip":
        ref = ao.scipy_interpolate(y, t, "pchip", False)
    got = _run(y, t, kind, None, "dense", "dcd", extrapolate=False)
    ao.assert_close(got, ref, y, f"{kind} without extrapolation")
    assert np.array_equal(np.isnan(got).all(axis=(1, 2)), (t < 0) | (t > n - 1))


def test_makima_threshold_is_one_maximum_over_all_columns():
    """One atom scaled by 1e12: every other column falls under 1e-9 G and takes the plain average, as in scipy.  A G per
    column, per block of 64 columns or per run would leave quiet columns on the weighted branch."""
    n, n_atoms = 9, 67
    y = ao.crafted(n, n_atoms, 11, special_atoms=(0, 66))
    y[:, 40] *= np.float32(1e12)
    thr, above, below = ao.makima_margin(y)
    assert below < 0.5 * thr and above > 2.0 * thr
    t = _times(n, 8)
    ref = ao.scipy_interpolate(y, t, "makima", True)
    quiet = [a for a in range(n_atoms) if a != 40]
    per_column = np.stack([ao.restated(y[:, a:a + 1], t, "makima")[:, 0] for a in quiet], axis=1)
    assert (np.abs(per_column - ref[:, quiet]) > 4 * ao.tolerance(ref[:, quiet], y[:, quiet])).mean() > 0.2   # the branches differ visibly
    for sel, in_layout in ((None, "dense"), (np.arange(n_atoms)[::-1].copy(), "dcd_odd_offset")):
        got = _run(y, t, "makima", sel, in_layout, "dense")
        chosen = np.arange(n_atoms) if sel is None else sel
        ao.assert_close(got, ref[:, chosen], y[:, chosen], "makima with one atom of 1e12")
    # ... and a selection without the loud atom is a different array: its own G, the weighted branch
    got = _run(y, t, "makima", np.asarray(quiet), "dense", "dense")
    ao.assert_close(got, ao.scipy_interpolate(y[:, quiet], t, "makima", True), y[:, quiet], "makima without the loud atom")


@pytest.mark.parametrize("kind", ["pchip", "makima"])
def test_noise_is_added_in_float64(kind):
    n, n_atoms = 7, 67
    rng = np.random.default_rng(9)
    sel = np.sort(rng.choice(n_atoms, 20, replace=False))
    y = ao.crafted(n, n_atoms, 5, special_atoms=(sel[0], sel[-1]))
    t = _times(n, 6)
    noise = np.random.RandomState(42).normal(0, 0.3, (len(t), len(sel), 3))
    ref = ao.scipy_interpolate(y[:, sel], t, kind, True) + noise
    for out_layout in OUT_LAYOUTS:
        got = _run(y, t, kind, sel, "dcd_odd_offset", out_layout, noise=noise)
        ao.assert_close(got, ref, y[:, sel], f"{kind} with noise -> {out_layout}")


@pytest.mark.parametrize("kind,n", [("pchip", 2), ("pchip", 40), ("makima", 3), ("makima", 40)])
def test_knots_come_back_bit_for_bit_and_runs_repeat(kind, n):
    n_atoms = 67
    y = ao.crafted(n, n_atoms, 21, special_atoms=(0, 66))
    y[:, 30] *= np.float32(1e6)   # a column whose slopes dwarf its neighbours' values
    got = _run(y, np.arange(n), kind, None, "dcd_odd_offset", "dcd")
    assert np.array_equal(got, y)
    t = _times(n, 60)
    first = _run(y, t, kind, None, "dense", "dense")
    assert np.array_equal(first, _run(y, t, kind, None, "dense", "dense"))
    assert np.array_equal(first, _run(y, t, kind, None, "dcd_two_records", "dcd"))   # the layouts change addresses, not values


@pytest.mark.parametrize("kind", ["pchip", "makima"])
def test_a_non_finite_coordinate_spoils_its_own_atom_only(kind):
    n, n_atoms = 9, 67
    y = ao.crafted(n, n_atoms, 31, special_atoms=(0, 66))
    t = _times(n, 7)
    clean = _run(y, t, kind, None, "dense", "dense")
    bad = y.copy()
    bad[4, 13, 1] = np.nan
    bad[2, 13, 2] = np.inf
    got = _run(bad, t, kind, None, "dense", "dense")
    others = [a for a in range(n_atoms) if a != 13]
    assert np.array_equal(got[:, others], clean[:, others]) and np.array_equal(got[:, 13, 0], clean[:, 13, 0])
    assert np.isnan(got[:, 13, 1]).any() and not np.isfinite(got[:, 13, 2]).all()


def test_invalid_arguments_are_refused_with_nothing_written():
    from deep_cartograph_amd import _lib, hip
    from deep_cartograph_amd._lib import DcvError

    lib = _lib.load()
    n, A, n_out = 5, 8, 6
    xyz = torch.from_numpy(ao.crafted(n, A, 1)).cuda()
    out = torch.full((n_out * A * 3,), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.dcv_interpolate_workspace(n, A, A, n_out)), dtype=torch.uint8, device="cuda")
    good_t = np.linspace(0.0, 4.0, n_out)
    good_sel = np.arange(A, dtype=np.int32)

    def call(n_knots=n, strides=(3 * A, 3, 1), sel=good_sel, n_sel=A, kind=0, t=good_t, ostrides=(3 * A, 3, 1), ws_bytes=ws.numel(), nt=n_out):
        t = np.ascontiguousarray(t, dtype=np.float64)
        sel = None if sel is None else np.ascontiguousarray(sel, dtype=np.int32)   # kept alive over the call
        sel_p = None if sel is None else sel.ctypes.data
        rc = lib.dcv_interpolate(xyz.data_ptr(), n_knots, *strides, A, sel_p, n_sel, kind, 1, t.ctypes.data, nt, None, out.data_ptr(), *ostrides,
                                 ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    EINVAL, ENOMEM = -1, -3
    assert call(kind=2) == EINVAL and call(kind=-1) == EINVAL
    assert call(n_knots=1) == EINVAL and call(n_knots=2, kind=1) == EINVAL
    assert call(sel=[0, 1, A], n_sel=3) == EINVAL and call(sel=[-1], n_sel=1) == EINVAL
    assert call(n_sel=0) == EINVAL and call(n_sel=-4) == EINVAL
    assert call(strides=(3 * A, 0, 1)) == EINVAL and call(strides=(-1, 3, 1)) == EINVAL and call(strides=(3 * A, 3, 0)) == EINVAL
    assert call(ostrides=(0, 3, 1)) == EINVAL and call(ostrides=(3 * A, 3, 0)) == EINVAL
    assert call(t=[0, 1, 2, 1.5, 3, 4]) == EINVAL and call(t=[0, 1, np.nan, 3, 4, 4]) == EINVAL and call(t=[0, 1, 2, 3, 4, np.inf]) == EINVAL
    assert call(ws_bytes=ws.numel() - 1) == ENOMEM
    assert call(nt=0) == 0
    assert torch.isnan(out).all(), "a refused call wrote to the output"
    assert call(n_knots=2) == 0 and call(sel=None, n_sel=0) == 0 and not torch.isnan(out).any()   # the same calls, valid: they do write
    # the front end: its own checks, in the error style of featurize / superpose
    with pytest.raises(DcvError, match="kind"):
        hip.interpolate(xyz, A, good_t, kind="linear")
    with pytest.raises(DcvError, match="makima needs at least 3"):
        hip.interpolate(xyz[:2], A, good_t[:2], kind="makima")
    with pytest.raises(DcvError, match="must not decrease"):
        hip.interpolate(xyz, A, good_t[::-1])
    with pytest.raises(DcvError, match="outside"):
        hip.interpolate(xyz, A, good_t, sel=[0, A])
    with pytest.raises(DcvError, match="empty"):
        hip.interpolate(xyz, A, good_t, sel=[])
    with pytest.raises(DcvError, match="CPU tensor"):
        hip.interpolate(xyz.cpu(), A, good_t)
    with pytest.raises(DcvError, match="noise"):
        hip.interpolate(xyz, A, good_t, noise=torch.zeros(n_out, A, 3, device="cuda"))
    with pytest.raises(DcvError, match="reaches element"):
        hip.interpolate(xyz, A, good_t, out=out[:-1], out_strides=(0, 3 * A, 3, 1))
    assert tuple(hip.interpolate(xyz, A, []).shape) == (0, A, 3)
    assert tuple(hip.interpolate(xyz, A, good_t, sel=[2, 1]).shape) == (n_out, 2, 3)


# ------------------------------------------------------------------------------------------------ tool and workflow
def _topology(n_res=10):
    from deep_cartograph_amd import trajectory as tr

    names, resids, pos = [], [], []
    rng = np.random.default_rng(5)
    for r in range(n_res):
        for name in ("N", "CA", "C"):
            names.append(name)
            resids.append(r + 1)
            pos.append(np.round(rng.normal(0.0, 1.0, 3) + [3.8 * r, 0.0, 0.0], 3))
    A = len(names)
    return tr.Topology(names, ["ALA"] * A, ["A"] * A, ["A"] * A, np.asarray(resids, dtype=np.int64), np.asarray(pos, dtype=np.float32),
                       {(i, i + 1) for i in range(A - 1)})


def _write_traj(folder, stem, n, seed):
    """A synthetic trajectory of 30 atoms (10 residues) as <stem>.dcd + <stem>.pdb -> (dcd, pdb, xyz, topology)."""
    from deep_cartograph_amd import trajectory as tr

    top = _topology()
    rng = np.random.default_rng(seed)
    xyz = (top.positions[None] + np.cumsum(rng.normal(0.0, 0.4, (n, top.n_atoms, 3)), axis=0)).astype(np.float32)
    pdb, dcd = os.path.join(folder, stem + ".pdb"), os.path.join(folder, stem + ".dcd")
    tr.write_topology(pdb, top)
    with tr.write_dcd(dcd, top.n_atoms) as w:
        img = w.image(n)
        off, fs, as_, cs = w.layout()
        img[off + fs * np.arange(n)[:, None, None] + as_ * np.arange(top.n_atoms)[None, :, None] + cs * np.arange(3)[None, None, :]] = xyz
        w.append(img)
    return dcd, pdb, xyz, top


@pytest.fixture(scope="module")
def seed(tmp_path_factory):
    return _write_traj(str(tmp_path_factory.mktemp("seed")), "morph", 12, 3)


@pytest.mark.parametrize("method", ["pchip", "akima"])
@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("traj_format", ["dcd", "npy"])
def test_tool_against_the_oracle(seed, tmp_path, method, keep, traj_format):
    """tools.traj_augmentation on 12 frames of 30 atoms, `name CA`, two replicas with noise, in chunks of a few frames: the
    files read back equal the oracle on the same grid plus each seed's noise stream; names, restart and the topology."""
    from deep_cartograph_amd import augmentation, tools
    from deep_cartograph_amd import trajectory as tr

    dcd, pdb, xyz, top = seed
    ca = tr.select_atoms(top, "name CA")
    cfg = {"num_frames": 57, "keep_original_frames": keep, "interpolation_method": method, "noise_std": 0.3, "random_seed": 7,
           "atom_selection": "name CA", "traj_format": traj_format}
    out = str(tmp_path / "aug")
    budget = 10 * (12 * 12 + 24 * 10)   # ten frames of ten atoms per chunk: 57 frames take six chunks
    trajs, tops = tools.traj_augmentation(dict(cfg), [dcd], [pdb], num_replicas=2, output_folder=out, memory_budget=budget)
    assert trajs == [os.path.join(out, f"morph_augmented_{method}_rep{r}.{traj_format}") for r in range(2)]
    assert tops == [os.path.join(out, f"morph_augmented_{method}_rep{r}.pdb") for r in range(2)]
    assert not [f for f in os.listdir(out) if f.endswith(".partial")]
    t = augmentation.new_frame_times(12, 57, keep)
    clean = ao.scipy_interpolate(xyz[:, ca], t, ao.KIND_OF_METHOD[method], True)
    frames = []
    for r in range(2):
        back_top = tr.read_topology(tops[r])
        assert back_top.names == ["CA"] * 10 and np.array_equal(back_top.resids, top.resids[ca]) and np.array_equal(back_top.positions, top.positions[ca])
        traj = tr.open_trajectory(trajs[r], back_top.n_atoms)
        assert traj.n_frames == 57
        noise = np.random.RandomState(7 + r).normal(0, 0.3, (57, 10, 3))
        frames.append(traj.frames())
        ao.assert_close(frames[-1], clean + noise, xyz[:, ca], f"{method} keep={keep} {traj_format} replica {r}")
    assert not np.array_equal(frames[0], frames[1])
    stamps = [os.stat(p).st_mtime_ns for p in trajs + tops]
    assert tools.traj_augmentation(dict(cfg), [dcd], [pdb], num_replicas=2, output_folder=out) == (trajs, tops)
    assert stamps == [os.stat(p).st_mtime_ns for p in trajs + tops]   # the second call skips
    # one replica, no noise: no suffix; with keep_original_frames the original frames appear bit for bit
    cfg["noise_std"] = None
    (one,), (one_top,) = tools.traj_augmentation(dict(cfg), dcd, pdb, output_folder=out, memory_budget=budget)
    assert one == os.path.join(out, f"morph_augmented_{method}.{traj_format}")
    got = tr.open_trajectory(one, 10).frames()
    ao.assert_close(got, clean, xyz[:, ca], f"{method} keep={keep} {traj_format} without noise")
    if keep:
        at = np.searchsorted(t, np.arange(12.0))
        assert np.array_equal(t[at], np.arange(12.0)) and np.array_equal(got[at], xyz[:, ca])


def test_tool_without_interpolation_emits_the_original_frames(seed, tmp_path):
    from deep_cartograph_amd import tools
    from deep_cartograph_amd import trajectory as tr

    dcd, pdb, xyz, top = seed
    (traj,), (new_top,) = tools.traj_augmentation({"interpolation_method": None, "num_frames": 5, "atom_selection": "resid 2:6"}, [dcd], [pdb],
                                                  output_folder=str(tmp_path))
    assert traj == str(tmp_path / "morph_augmented_None.dcd")
    atoms = tr.select_atoms(top, "resid 2:6")
    assert np.array_equal(tr.open_trajectory(traj, len(atoms)).frames(), xyz[:, atoms])
    assert tr.read_topology(new_top).bonds == {(i, i + 1) for i in range(len(atoms) - 1)}


def test_deep_carto_augments_the_seed_trajectories(seed, tmp_path):
    from deep_cartograph_amd import deep_carto

    seed_dcd, seed_pdb, _, _ = seed
    main_dcd, main_pdb, _, _ = _write_traj(str(tmp_path), "md", 90, 8)
    features = {"dihedral_groups": {"tor": {"selection": "name CA", "periodic_encoding": True, "search_mode": "virtual"}}}
    cfg = {"traj_augmentation": {"num_frames": 41, "interpolation_method": "akima", "atom_selection": "name CA"},
           "compute_features": {"plumed_settings": {"traj_stride": 1, "features": features}},
           "train_colvars": {"cvs": ["pca"], "common": {"dimension": 2, "features_normalization": "mean_std"}}, "traj_cluster": {"run": False}}
    out = tmp_path / "run"
    res = deep_carto.deep_cartograph(json.loads(json.dumps(cfg)), [], trajectory_data=[main_dcd], topology_data=[main_pdb],
                                     seed_trajectory_data=[seed_dcd], seed_topology_data=[seed_pdb], output_folder=str(out))
    assert os.path.exists(out / "traj_augmentation" / "morph_augmented_akima.dcd") and os.path.exists(out / "traj_augmentation" / "morph_augmented_akima.pdb")
    matrices = sorted(d for d in os.listdir(out / "compute_features") if os.path.isdir(out / "compute_features" / d))
    assert matrices == ["md", "morph_augmented_akima"]   # len(traj) + len(seed) feature matrices
    assert np.load(out / "compute_features" / "md" / "colvars.npy").shape == (90, 14)
    aug = np.load(out / "compute_features" / "morph_augmented_akima" / "colvars.npy")
    assert aug.shape == (41, 14) and np.isfinite(aug).all()   # num_frames rows; akima extrapolates, so the last frames are finite
    assert len(res["train_colvars"]["pca"]) == 2
    # seeds alone
    alone = tmp_path / "alone"
    deep_carto.deep_cartograph(json.loads(json.dumps(cfg)), [], seed_trajectory_data=seed_dcd, seed_topology_data=seed_pdb, output_folder=str(alone))
    assert os.path.exists(alone / "compute_features" / "morph_augmented_akima" / "colvars.npy") and not os.path.exists(alone / "analyze_geometry") and os.path.exists(alone / "train_colvars" / "pca" / "model.zip")
