"""analyze_geometry on the MI355X: the superposition kernel (dcv_superpose) against the float64 SVD oracle
(tests/geometry_oracle.py) over its shapes, layouts and arithmetic edges, the moments' determinism, the error codes of
the C-ABI, and the tool and the deep_carto pre-step on the reference's own trajectory.

Tolerance: both sides are float64 on identical float32 input; SVD-Kabsch and the quaternion form differ by <= 6e-14
Angstrom in RMSD and <= 7e-14 in rotation entries for n_fit >= 4 (1e-11 at n_fit = 3) on the host.  TOL = 1e-9
(Angstrom for RMSD, RMSF and moments / n; absolute for rotation entries) leaves four orders for summation order and the
Jacobi stopping rule and is 60 times below half a float32 ulp at 1 Angstrom."""
import json
import os

import numpy as np
import pytest
import torch

from tests import features_oracle as fo
from tests import geometry_oracle as go
from tests.conftest import load_golden
from tests.test_compute_features_gpu import dense_buffer, planes_buffer

pytestmark = pytest.mark.gpu

TOL = 1e-9
TILE = 16
ALL = ("transform", "rmsd", "aligned", "moments")


def run(buf, layout, A, fit, fit_ref, sel=None, sel_ref=None, w=None, want=ALL, every=1):
    from deep_cartograph_amd import hip

    n, off, fs, as_, cs = layout
    lay = ((n + every - 1) // every, off, fs * every, as_, cs)
    out = hip.superpose(torch.from_numpy(buf).cuda(), A, fit, fit_ref, sel=sel, sel_ref=sel_ref, fit_weights=w, strides=lay, want=want)
    return {k: v.cpu().numpy() for k, v in out.items()}


def rotations(transform):
    return transform[:, :9].reshape(-1, 3, 3)


def assert_proper_rotations(transform):
    R = rotations(transform)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < TOL
    assert np.abs(np.linalg.det(R) - 1.0).max() < TOL


def assert_matches_oracle(got, ref, n, rotation=True, selection=True):
    """`rotation`: R is unique (the fit atoms are in general position); `selection`: what depends on R outside the fit
    atoms (aligned coordinates, the selection's RMSD, moments) is compared too.  Every figure is printed before it is
    asserted."""
    err = {"fit rmsd": np.abs(got["rmsd"][:, 0] - ref["rmsd"][:, 0]).max(), "centroids": np.abs(got["transform"][:, 9:15] - ref["transform"][:, 9:15]).max()}
    if rotation:
        err["rotation"] = np.abs(got["transform"][:, :9] - ref["transform"][:, :9]).max()
    if selection:
        err["selection rmsd"] = np.abs(got["rmsd"][:, 1] - ref["rmsd"][:, 1]).max()
        if "moments" in got:
            err["moments / n"] = np.abs(got["moments"] - ref["moments"]).max() / n
    print("max |got - oracle|: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert max(err.values()) < TOL, err
    assert np.array_equal(got["transform"][:, 15], got["rmsd"][:, 0])
    assert_proper_rotations(got["transform"])
    if selection and "aligned" in got:
        assert got["aligned"].dtype == np.float32
        ulps = int(fo.ulp_distance_f32(got["aligned"], ref["aligned"].astype(np.float32)).max())
        print(f"aligned: at most {ulps} float32 ulp from float32(oracle)")
        assert ulps <= 1


# ------------------------------------------------------------------------------------------------ 1. kernel shapes
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("n_fit", [1, 2, 3, 4, 63, 64, 65, 257])
def test_fit_sizes_frames_and_layouts(n_fit, n):
    """Fit sets around the lanes of a frame's group (16) and the wave, frame counts around the tile of 16; dense rows,
    DCD planes and planes behind a unit-cell block, each with the base shifted by 0 to 3 words and NaN in every marker
    and padding word: the same bits in every layout.  The selection is every atom, the fit set a subset of them."""
    A = n_fit + 3
    xyz, ref = go.synthetic(n, A, 1000 * n_fit + n)
    fit = np.arange(A)[np.random.Generator(np.random.PCG64(n_fit)).permutation(A)[:n_fit]]
    sel = np.arange(A)
    oracle = go.superpose(xyz, fit, ref[fit], sel, ref)
    first = None
    for pre in range(4):
        for buf, layout in (dense_buffer(xyz, pre), planes_buffer(xyz, pre), planes_buffer(xyz, pre, cell=True)):
            got = run(buf, layout, A, fit, ref[fit], sel, ref)
            if first is None:
                first = got
                assert got["transform"].shape == (n, 16) and got["rmsd"].shape == (n, 2) and got["aligned"].shape == (n, A, 3)
                assert got["moments"].shape == (A, 3, 2)
                # one or two fit atoms leave R free and three are always coplanar: there the RMSD of the fit, which is unique,
                # is compared and R must be a proper rotation
                assert_matches_oracle(got, oracle, n, rotation=n_fit >= 4, selection=n_fit >= 4)
            for k in ALL:
                assert np.array_equal(got[k], first[k]), f"{k}: pre={pre} layout={layout}"
    if n_fit == 1:
        assert np.array_equal(first["rmsd"][:, 0], np.zeros(n)) and np.abs(rotations(first["transform"]) - np.eye(3)).max() < TOL


def test_frame_stride_keeps_every_third_frame():
    n, A = 50, 11
    xyz, ref = go.synthetic(n, A, 9)
    fit = np.arange(A)
    full = run(*dense_buffer(xyz), A, fit, ref, fit, ref)
    assert_matches_oracle(full, go.superpose(xyz, fit, ref, fit, ref), n)
    oracle3 = go.superpose(xyz[::3], fit, ref, fit, ref)
    for buf, layout in (dense_buffer(xyz, 2), planes_buffer(xyz, 3, cell=True)):
        got = run(buf, layout, A, fit, ref, fit, ref, every=3)
        assert got["rmsd"].shape[0] == 17
        for k in ("transform", "rmsd", "aligned"):
            assert np.array_equal(got[k], full[k][::3]), k
        assert np.abs(got["moments"] - oracle3["moments"]).max() / 17 < TOL


def test_sparse_subset_is_gathered():
    """Every 8th of 600 atoms: the used atoms fill an eighth of their range, so they are gathered, not copied as rows."""
    n, A = 2 * TILE + 3, 600
    xyz, ref = go.synthetic(n, A, 21)
    fit = np.arange(0, A, 8)
    sel = fit[::3]
    oracle = go.superpose(xyz, fit, ref[fit], sel, ref[sel])
    first = run(*dense_buffer(xyz), A, fit, ref[fit], sel, ref[sel])
    assert_matches_oracle(first, oracle, n)
    got = run(*planes_buffer(xyz, 1), A, fit, ref[fit], sel, ref[sel])
    for k in ALL:
        assert np.array_equal(got[k], first[k]), k


@pytest.mark.parametrize("relation", ["equal", "disjoint", "overlapping", "containing"])
def test_selection_and_fit_set(relation):
    n, A = 19, 40
    xyz, ref = go.synthetic(n, A, 77)
    fit = np.arange(10, 25)
    sel = {"equal": fit, "disjoint": np.arange(27, 38), "overlapping": np.arange(20, 33), "containing": np.arange(5, 31)}[relation]
    got = run(*planes_buffer(xyz, 2), A, fit, ref[fit], sel, ref[sel])
    assert_matches_oracle(got, go.superpose(xyz, fit, ref[fit], sel, ref[sel]), n)
    if relation == "equal":
        assert np.abs(got["rmsd"][:, 0] - got["rmsd"][:, 1]).max() < TOL
    # without a reference for the selection there is no second RMSD to hand out; the aligned coordinates are the same
    bare = run(*planes_buffer(xyz, 2), A, fit, ref[fit], sel, None, want=("rmsd", "aligned"))
    assert bare["rmsd"].shape == (n, 1) and np.array_equal(bare["rmsd"][:, 0], got["rmsd"][:, 0])
    assert np.array_equal(bare["aligned"], got["aligned"])


def test_many_atoms_shrink_the_tile():
    """2000 staged atoms: 24 KB of LDS per frame, two frames per workgroup and 64 lanes per frame."""
    n, A = 5, 2000
    xyz, ref = go.synthetic(n, A, 33)
    fit = np.arange(A)
    sel = np.arange(0, A, 4)     # 500 atoms: with moments one frame per workgroup
    oracle = go.superpose(xyz, fit, ref, sel, ref[sel])
    for buf, layout in (dense_buffer(xyz, 1), planes_buffer(xyz, 2)):
        assert_matches_oracle(run(buf, layout, A, fit, ref, sel, ref[sel], want=("transform", "rmsd", "aligned")), oracle, n)
        assert_matches_oracle(run(buf, layout, A, fit, ref, sel, ref[sel]), oracle, n)


# ------------------------------------------------------------------------------------------------ 2. arithmetic
def test_mirror_images_get_the_proper_rotation():
    """Every 7th frame mirrored: a reflection would fit it as well as its neighbours; the proper rotation cannot, and its
    larger RMSD is what comes back.  This is where a Newton iteration on the characteristic polynomial stalls."""
    n, A = 29, 30
    xyz, ref = go.synthetic(n, A, 5)
    xyz[::7, :, 2] *= -1
    fit = np.arange(A)
    got = run(*dense_buffer(xyz), A, fit, ref, fit, ref)
    assert_matches_oracle(got, go.superpose(xyz, fit, ref, fit, ref), n)
    mirrored = np.zeros(n, dtype=bool)
    mirrored[::7] = True
    assert got["rmsd"][mirrored, 0].min() > 5.0 > 2.5 > got["rmsd"][~mirrored, 0].max()


@pytest.mark.parametrize("shape", ["coplanar", "collinear", "mirrored coplanar"])
def test_degenerate_fit_sets_of_many_atoms(shape):
    """40 fit atoms in a plane or on a line, and planar frames that are mirror images of the reference inside their plane:
    the two largest eigenvalues of the 4 x 4 matrix meet.  The minimal RMSD is unique and is compared; R is not unique
    (collinear) or only just (coplanar), so it must be a proper rotation and is not compared."""
    n, A = 23, 40
    xyz, ref = go.synthetic(n, A, 17, noise=0.0)
    rng = np.random.Generator(np.random.PCG64(18))
    flat = ref.copy()
    flat[:, 2] = 0.0
    if shape == "collinear":
        flat[:, 1] = 0.0
    for f in range(n):
        mobile = flat + rng.standard_normal((A, 3)) * [1.0, 0.0 if shape == "collinear" else 1.0, 0.0]   # noise inside the set's own space
        if shape == "mirrored coplanar" and f % 2:
            mobile[:, 0] *= -1
        xyz[f] = (mobile @ go.random_rotation(rng) + rng.uniform(-300, 300, 3)).astype(np.float32)
    fit = np.arange(A)
    got = run(*dense_buffer(xyz), A, fit, flat, want=("transform", "rmsd"))
    assert_matches_oracle(got, go.superpose(xyz, fit, flat), n, rotation=False, selection=False)


def test_identical_frame_gives_zero_and_identity():
    A = 50
    _, ref = go.synthetic(1, A, 8)
    ref32 = ref.astype(np.float32)
    xyz = np.stack([ref32, ref32 + np.float32(0.5)])      # the reference itself, and (inexactly) translated
    fit = np.arange(A)
    got = run(*dense_buffer(xyz), A, fit, ref32.astype(np.float64), fit, ref32.astype(np.float64), want=("transform", "rmsd"))
    assert got["rmsd"][0].max() < TOL and np.abs(rotations(got["transform"])[0] - np.eye(3)).max() < TOL
    assert got["rmsd"][1].max() < 1e-5      # float32 rounding of the shifted coordinates, 4e-6 at 60 Angstrom


def test_exact_translation_changes_nothing():
    """Coordinates on a 1/64 Angstrom grid moved by exactly 1024 Angstrom are the same structure to the last bit; RMSD
    and R must not notice (centring before the correlation is formed)."""
    n, A = 21, 64
    xyz, ref = go.synthetic(n, A, 13, shift=50.0)
    near = (np.round(xyz * 64) / 64).astype(np.float32)
    far = near + np.float32(1024.0)
    assert np.array_equal((far - np.float32(1024.0)), near)
    fit = np.arange(0, A, 2)
    a = run(*dense_buffer(near), A, fit, ref[fit], want=("transform", "rmsd"))
    b = run(*dense_buffer(far), A, fit, ref[fit], want=("transform", "rmsd"))
    assert np.abs(a["rmsd"][:, 0] - b["rmsd"][:, 0]).max() < TOL
    assert np.abs(a["transform"][:, :9] - b["transform"][:, :9]).max() < TOL
    assert np.abs(b["transform"][:, 9:12] - a["transform"][:, 9:12] - 1024.0).max() < TOL
    assert_matches_oracle(b, go.superpose(far, fit, ref[fit]), n, selection=False)


def test_weights():
    n, A = 18, 37
    xyz, ref = go.synthetic(n, A, 61)
    fit, sel = np.arange(A), np.arange(5, 20)
    rng = np.random.Generator(np.random.PCG64(4))
    w = rng.uniform(0.05, 4.0, A)
    got = run(*planes_buffer(xyz, 1), A, fit, ref, sel, ref[sel], w=w)
    assert_matches_oracle(got, go.superpose(xyz, fit, ref, sel, ref[sel], w=w), n)
    # weights 0 / 1 are the fit on the subset
    mask = rng.uniform(size=A) < 0.5
    masked = run(*planes_buffer(xyz, 1), A, fit, ref, sel, ref[sel], w=mask.astype(np.float64))
    subset = run(*planes_buffer(xyz, 1), A, fit[mask], ref[mask], sel, ref[sel])
    for k in ("transform", "rmsd", "moments"):
        assert np.abs(masked[k] - subset[k]).max() < TOL, k
    assert fo.ulp_distance_f32(masked["aligned"], subset["aligned"]).max() <= 1


# ------------------------------------------------------------------------------------------------ 3. moments
def test_moments_are_deterministic_over_many_tiles():
    """16 * DCV_SUPERPOSE_MAX_GROUPS + 17 frames of 4 atoms: every workgroup takes a second tile, two a third one."""
    from deep_cartograph_amd import _lib

    n, A = TILE * _lib.SUPERPOSE_MAX_GROUPS + 17, 4
    xyz, ref = go.synthetic(n, A, 99)
    fit = np.arange(A)
    buf, layout = dense_buffer(xyz)
    one = run(buf, layout, A, fit, ref, fit, ref, want=("rmsd", "moments"))
    two = run(buf, layout, A, fit, ref, fit, ref, want=("rmsd", "moments"))
    assert np.array_equal(one["moments"], two["moments"]) and np.array_equal(one["rmsd"], two["rmsd"])
    oracle = go.superpose(xyz, fit, ref, fit, ref)
    assert np.abs(one["moments"] - oracle["moments"]).max() / n < TOL
    assert np.abs(one["rmsd"] - oracle["rmsd"]).max() < TOL


# ------------------------------------------------------------------------------------------------ 4. errors
def test_error_codes_leave_the_outputs_untouched():
    from deep_cartograph_amd import _lib, hip

    lib = _lib.load()
    n, A = 10, 6
    xyz_h, ref = go.synthetic(n, A, 1)
    xyz = torch.from_numpy(xyz_h).cuda()
    outs = {"transform": torch.full((n, 16), 123.0, dtype=torch.float64, device="cuda"), "rmsd": torch.full((n, 2), 123.0, dtype=torch.float64, device="cuda"),
            "aligned": torch.full((n, 3 * A), 123.0, dtype=torch.float32, device="cuda"), "moments": torch.full((A, 3, 2), 123.0, dtype=torch.float64, device="cuda")}
    need = lib.dcv_superpose_workspace(n, A, A, A)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    fit_ok = np.arange(A, dtype=np.int32)
    dptr = lambda x: None if x is None else x.ctypes.data

    def call(fit=fit_ok, w=None, sel=fit_ok, sel_ref=ref, ws_bytes=need, lda=3 * A, n_atoms=A, coords=xyz, fit_ref=ref):
        fit, fit_ref = np.ascontiguousarray(fit, dtype=np.int32), np.ascontiguousarray(fit_ref, dtype=np.float64)   # alive across the call
        rc = lib.dcv_superpose(coords.data_ptr(), n, 3 * n_atoms, 3, 1, n_atoms, dptr(fit), dptr(w), dptr(fit_ref), len(fit),
                               dptr(sel), dptr(sel_ref), 0 if sel is None else len(sel), outs["transform"].data_ptr(), outs["rmsd"].data_ptr(),
                               outs["aligned"].data_ptr(), lda, outs["moments"].data_ptr(), ws.data_ptr(), ws_bytes, None)
        torch.cuda.synchronize()
        return rc

    big = 5462    # one frame is 65 544 bytes of LDS
    big_xyz, big_ref = torch.zeros(n, big, 3, device="cuda"), np.zeros((big, 3))
    big_ws = torch.zeros(lib.dcv_superpose_workspace(n, big, big, A), dtype=torch.uint8, device="cuda")
    cases = {"atom index": (dict(fit=[0, 1, 2, 3, 4, A]), -1), "negative atom": (dict(sel=np.asarray([0, -1, 2, 3, 4, 5], dtype=np.int32)), -1),
             "zero weight sum": (dict(w=np.zeros(A)), -1), "negative weight": (dict(w=np.asarray([1, 1, -1, 1, 1, 1], dtype=np.float64)), -1),
             "nan weight": (dict(w=np.asarray([1, 1, np.nan, 1, 1, 1], dtype=np.float64)), -1),
             "moments without sel_ref": (dict(sel_ref=None), -1), "lda": (dict(lda=3 * A - 1), -1), "workspace": (dict(ws_bytes=need - 1), -3)}
    for what, (kw, code) in cases.items():
        assert call(**kw) == code, what
        assert lib.dcv_last_error().decode().startswith("dcv_superpose"), what
        for k, o in outs.items():
            assert bool((o == 123.0).all()), f"{what}: {k} was written"
    ws, need_small = big_ws, need
    assert call(fit=np.arange(big), sel=fit_ok, sel_ref=ref, n_atoms=big, coords=big_xyz, fit_ref=big_ref, ws_bytes=big_ws.numel()) == -1
    assert "LDS" in lib.dcv_last_error().decode()
    for k, o in outs.items():
        assert bool((o == 123.0).all()), f"5462 staged atoms: {k} was written"
    ws = torch.zeros(need_small, dtype=torch.uint8, device="cuda")
    assert call() == 0
    for k, o in outs.items():
        assert bool((o != 123.0).all()), k
    assert lib.dcv_superpose_workspace(n, 0, A, A) == 0 and lib.dcv_superpose_workspace(n, A, 0, A) == 0
    # the front end: no frames is an empty result, a CPU tensor and an unknown output are refused
    empty = hip.superpose(torch.zeros(0, A, 3, device="cuda"), A, fit_ok, ref, want=("rmsd", "transform"))
    assert tuple(empty["rmsd"].shape) == (0, 1) and tuple(empty["transform"].shape) == (0, 16)
    with pytest.raises(hip.DcvError, match="LDS"):
        hip.superpose(big_xyz, big, np.arange(big), big_ref)
    with pytest.raises(hip.DcvError, match="want"):
        hip.superpose(xyz, A, fit_ok, ref, want=("rmsf",))
    with pytest.raises(hip.DcvError, match="sel_ref"):
        hip.superpose(xyz, A, fit_ok, ref, sel=fit_ok, want=("moments",))


# ------------------------------------------------------------------------------------------------ 5. the tool
@pytest.fixture(scope="module")
def fixture_files(tmp_path_factory):
    g = load_golden("compute_features_golden.npz")
    d = tmp_path_factory.mktemp("ca_example")
    dcd, pdb = str(d / "CA_example.dcd"), str(d / "CA_example.pdb")
    with open(dcd, "wb") as f:
        f.write(g["dcd"].tobytes())
    with open(pdb, "w") as f:
        f.write(str(g["pdb"]))
    return dcd, pdb


CONFIG = {"dt_per_frame": 10.0,
          "analysis": {"RMSD": {"ca": {}, "part": {"selection": "resid {a}:{b} and name CA"}}, "RMSF": {"ca": {}},
                       "dRMSD": {"ca": {"selection_stride": 5}}}}


@pytest.fixture(scope="module")
def fixture_case(fixture_files, tmp_path_factory):
    """Topology, coordinates, a second PDB written from frame 10, the configuration and -- computed once -- the oracle's
    series under the keys of the files the tool writes."""
    from deep_cartograph_amd import trajectory as tr

    dcd, pdb = fixture_files
    top = tr.read_topology(pdb)
    xyz = tr.open_trajectory(dcd, top.n_atoms).frames()
    assert xyz.shape == (164, 104, 3)
    frame10 = str(tmp_path_factory.mktemp("refs") / "frame10.pdb")
    with open(pdb) as src, open(frame10, "w") as dst:
        i = 0
        for line in src:
            if line.startswith(("ATOM", "HETATM")):
                line = line[:30] + "%8.3f%8.3f%8.3f" % tuple(xyz[10, i]) + line[54:]
                i += 1
            dst.write(line)
    ref10 = tr.read_topology(frame10)
    a, b = int(top.resids[10]), int(top.resids[40])
    cfg = json.loads(json.dumps(CONFIG).replace("{a}", str(a)).replace("{b}", str(b)))
    ca = tr.select_atoms(top, "name CA")
    part = tr.select_atoms(top, f"resid {a}:{b} and name CA")
    assert len(ca) == 104 and 3 < len(part) < 104
    t = np.arange(164) * 10.0 * 1e-3
    group = {"first_selection": "name CA", "second_selection": "name CA", "first_stride": 5, "second_stride": 5,
             "skip_neigh_residues": True, "skip_bonded_atoms": True}
    _, defs = tr.feature_definitions({"distance_groups": {"distances": group}}, top)
    _, defs10 = tr.feature_definitions({"distance_groups": {"distances": group}}, ref10)
    assert np.array_equal(defs, defs10)
    rmsf, residues = go.rmsf(xyz, ca, ca, top.resids)
    series = {}
    for ref_name, ref_top in (("first_frame", top), ("_to_frame10", ref10)):
        pos = ref_top.positions.astype(np.float64)
        series[f"ca_RMSD_CA_example{ref_name}"] = (t, go.rmsd(xyz, ca, pos[ca], ca, pos[ca]))
        series[f"part_RMSD_CA_example{ref_name}"] = (t, go.rmsd(xyz, ca, pos[ca], part, pos[part]))
    series["ca_RMSF_CA_example"] = (residues.astype(np.float64), rmsf)
    series["ca_dRMSD_CA_example_to_CA_example"] = (t, go.drmsd(xyz, top.positions, defs))
    series["ca_dRMSD_CA_example_to_frame10"] = (t, go.drmsd(xyz, ref10.positions, defs))
    d_max = float(fo.featurize(xyz, defs).max())
    return {"cfg": cfg, "frame10": frame10, "series": series, "drmsd_tol": float(np.spacing(np.float32(d_max))), "top": top}


def assert_csv(path, key, case):
    x, y = case["series"][key]
    category = key.split("_")[1]
    with open(path) as f:
        assert f.readline() == ("Residue" if category == "RMSF" else "Time (ns)") + f",{category} (A)\n"
    got = np.loadtxt(path, delimiter=",", skiprows=1)
    assert got.shape == (len(x), 2) and np.array_equal(got[:, 0], x)
    err = np.abs(got[:, 1] - y).max()
    print(f"{key}: max |got - oracle| = {err:.3e}")
    # dRMSD: float32 distances from the device, one float32 ulp of the largest distance (nm); everything else float64
    assert err <= (case["drmsd_tol"] if category == "dRMSD" else TOL)


def test_tool_on_the_reference_trajectory(fixture_files, fixture_case, tmp_path):
    from deep_cartograph_amd import tools

    dcd, pdb = fixture_files
    out = tools.analyze_geometry(fixture_case["cfg"], [dcd], [pdb], output_folder=str(tmp_path / "own"))
    assert sorted(out) == ["ca_RMSD_CA_examplefirst_frame", "ca_RMSF_CA_example", "ca_dRMSD_CA_example_to_CA_example", "part_RMSD_CA_examplefirst_frame"]
    for key, path in out.items():
        assert_csv(path, key, fixture_case)
    out = tools.analyze_geometry(fixture_case["cfg"], [dcd], [pdb], ref_topologies=[fixture_case["frame10"]], output_folder=str(tmp_path / "ref"))
    assert sorted(out) == ["ca_RMSD_CA_example_to_frame10", "ca_RMSF_CA_example", "ca_dRMSD_CA_example_to_frame10", "part_RMSD_CA_example_to_frame10"]
    for key, path in out.items():
        assert_csv(path, key, fixture_case)
    # frame 10 against the structure written from it: the PDB's three decimals are all that is left
    assert np.loadtxt(out["ca_RMSD_CA_example_to_frame10"], delimiter=",", skiprows=1)[10, 1] < 1e-3
    assert np.loadtxt(out["ca_dRMSD_CA_example_to_frame10"], delimiter=",", skiprows=1)[10, 1] < 1e-4


def test_chunks_give_the_same_bits(fixture_files, fixture_case, tmp_path, caplog):
    """A budget of 60 frame records: chunks of 60, 60 and 44 frames.  The per-frame series (RMSD, dRMSD) have the bits
    of the single chunk.  The RMSF adds the chunks' float64 moments on the host, which associates the sum over frames
    differently from one launch over all of them: it is held to the oracle's tolerance and, between the two runs, to
    1e-12 Angstrom (sums of 164 terms of order 1 carry rounding of order 1e-14)."""
    import logging

    from deep_cartograph_amd import geometry

    caplog.set_level(logging.INFO, logger="deep_cartograph_amd.geometry")
    from deep_cartograph_amd import trajectory as tr

    dcd, pdb = fixture_files
    record = 4 * tr.open_trajectory(dcd, 104).frame_stride      # bytes of a frame as it is uploaded
    budget = 60 * (record + 16) + 100
    whole = geometry.rmsd(dcd, pdb, "name CA", "name CA")
    parts = geometry.rmsd(dcd, pdb, "name CA", "name CA", memory_budget=budget)
    assert "164 frames in chunks of 60 frames" in caplog.text
    assert whole.dtype == np.float64 and np.array_equal(whole, parts)
    assert np.array_equal(geometry.drmsd(dcd, pdb, "name CA", 5, pdb), geometry.drmsd(dcd, pdb, "name CA", 5, pdb, memory_budget=40 * record))
    one, residues = geometry.rmsf(dcd, pdb, "name CA", "name CA")
    many, residues_many = geometry.rmsf(dcd, pdb, "name CA", "name CA", memory_budget=budget)
    x, y = fixture_case["series"]["ca_RMSF_CA_example"]
    assert np.array_equal(residues, x) and np.array_equal(residues_many, x)
    print(f"RMSF: chunks vs one {np.abs(one - many).max():.3e}, one vs oracle {np.abs(one - y).max():.3e}")
    assert np.abs(one - y).max() < TOL and np.abs(many - y).max() < TOL and np.abs(one - many).max() < 1e-12
    avg = geometry.average_structure(dcd, pdb, "name CA", memory_budget=budget)
    xyz = tr.open_trajectory(dcd, 104).frames()
    assert np.abs(avg - go.average_structure(xyz, np.arange(104))).max() < TOL


def test_rmsf_of_a_selection_larger_than_one_call_of_moments(tmp_path):
    """1 600 selected atoms fitted on 300: the moment partials of one call hold 808 atoms beside the staged frame, so the
    selection is served in two batches; average structure and RMSF against the oracle."""
    from deep_cartograph_amd import geometry
    from deep_cartograph_amd import trajectory as tr

    n, A = 6, 1600
    xyz, ref = go.synthetic(n, A, 44)
    top = tr.Topology(["CA"] * A, ["ALA"] * A, ["A"] * A, ["A"] * A, np.arange(1, A + 1, dtype=np.int64), ref.astype(np.float32), None)
    traj = tr.Trajectory(xyz.reshape(-1), n, A, 0, 3 * A, 3, 1)
    fit = np.arange(300)
    assert (geometry.MOMENT_LDS_BYTES - 24 * 300) // 72 == 808
    got, residues = geometry.rmsf(traj, top, "name CA", "resid 1:300")
    want, want_residues = go.rmsf(xyz, fit, np.arange(A), top.resids)
    err = np.abs(got - want).max()
    print(f"RMSF in two batches of atoms: max |got - oracle| = {err:.3e}")
    assert np.array_equal(residues, want_residues) and err < TOL
    assert np.abs(geometry.average_structure(traj, top, "resid 1:300") - go.average_structure(xyz, fit)).max() < TOL


def test_deep_carto_runs_the_tool_first(fixture_files, fixture_case, tmp_path):
    from deep_cartograph_amd import deep_carto

    dcd, pdb = fixture_files
    features = {"dihedral_groups": {"tor": {"selection": "all", "periodic_encoding": True, "search_mode": "virtual"}}}
    cfg = {"compute_features": {"plumed_settings": {"traj_stride": 1, "features": features}},
           "train_colvars": {"cvs": ["pca"], "common": {"dimension": 2, "features_normalization": "mean_std"}}, "traj_cluster": {"run": False}}
    deep_carto.deep_cartograph(json.loads(json.dumps(cfg)), [], trajectory_data=[dcd], topology_data=[pdb], output_folder=str(tmp_path / "without"))
    assert os.path.exists(tmp_path / "without" / "compute_features") and not os.path.exists(tmp_path / "without" / "analyze_geometry")
    cfg["analyze_geometry"] = fixture_case["cfg"]
    deep_carto.deep_cartograph(json.loads(json.dumps(cfg)), [], trajectory_data=[dcd], topology_data=[pdb], output_folder=str(tmp_path / "with"))
    folder = tmp_path / "with" / "analyze_geometry"
    files = sorted(f for f in os.listdir(folder) if f.endswith(".csv"))
    assert files == ["ca_RMSD_CA_examplefirst_frame.csv", "ca_RMSF_CA_example.csv", "ca_dRMSD_CA_example_to_CA_example.csv",
                     "part_RMSD_CA_examplefirst_frame.csv"]
    for f in files:
        assert_csv(str(folder / f), f[:-4], fixture_case)
    assert os.path.exists(tmp_path / "with" / "train_colvars" / "pca" / "model.zip")
