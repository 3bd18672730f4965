"""compute_features on the MI355X: the featurisation kernel against PLUMED's own output and the float64 oracle
(tests/features_oracle.py), its layouts, tiles and edges on small synthetic coordinates, the error codes of the
C-ABI, the streaming tool and the deep_carto pre-step."""
import json
import os
import zipfile

import numpy as np
import pandas as pd
import pytest
import torch

from tests import features_oracle as fo
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

VIRTUAL_DIHEDRALS = {"dihedral_groups": {"tor": {"selection": "all", "periodic_encoding": True, "search_mode": "virtual"}}}
DISTANCES = {"distance_groups": {"dist": {"first_selection": "all", "second_selection": "all", "first_stride": 1, "second_stride": 10,
                                          "skip_neigh_residues": False, "skip_bonded_atoms": True}}}
TILE = 16   # frames per workgroup (include/dcv.h)
D, SC, T = fo.DISTANCE, fo.TORSION_SINCOS, fo.TORSION


@pytest.fixture(scope="module")
def golden():
    g, f = load_golden("compute_features_golden.npz"), load_golden("filter_golden.npz")
    return {"dcd": g["dcd"].tobytes(), "pdb": str(g["pdb"]), "distances": np.ascontiguousarray(g["distances"]),
            "distance_names": [str(s) for s in g["distance_names"]],
            "dihedrals": np.ascontiguousarray(f["X"]), "dihedral_names": [str(s) for s in f["names"]]}


@pytest.fixture(scope="module")
def fixture_files(golden, tmp_path_factory):
    d = tmp_path_factory.mktemp("ca_example")
    dcd, pdb = str(d / "CA_example.dcd"), str(d / "CA_example.pdb")
    with open(dcd, "wb") as f:
        f.write(golden["dcd"])
    with open(pdb, "w") as f:
        f.write(golden["pdb"])
    return dcd, pdb


@pytest.fixture(scope="module")
def fixture_case(fixture_files):
    """Topology, trajectory, coordinates and -- computed once -- the oracle's matrices of the reference's fixture."""
    from deep_cartograph_amd import trajectory as tr

    top = tr.read_topology(fixture_files[1])
    traj = tr.open_trajectory(fixture_files[0], top.n_atoms)
    xyz = traj.frames()
    case = {"top": top, "traj": traj, "xyz": xyz}
    for key, features in (("dihedrals", VIRTUAL_DIHEDRALS), ("distances", DISTANCES)):
        names, defs = tr.feature_definitions(features, top)
        case[key] = {"names": names, "defs": defs, "oracle": fo.featurize(xyz, defs)}
    return case


# ------------------------------------------------------------------------------------------------ helpers
def planes_buffer(xyz, pre=0, cell=False):
    """The frames as DCD records in one flat float32 buffer: per frame [14 words of unit cell] and three planes
    marker X[A] marker, marker Y[A] marker, marker Z[A] marker; `pre` words in front shift the alignment.  Markers and
    padding are NaN, so a kernel that read one would show it.  Returns (buffer, layout for hip.featurize)."""
    n, A = xyz.shape[:2]
    words = (14 if cell else 0) + 3 * (A + 2)
    buf = np.full(pre + n * words, np.nan, dtype=np.float32)
    for f in range(n):
        base = pre + f * words + (14 if cell else 0)
        for c in range(3):
            buf[base + c * (A + 2) + 1: base + c * (A + 2) + 1 + A] = xyz[f, :, c]
    return buf, (n, pre + (14 if cell else 0) + 1, words, 1, A + 2)


def dense_buffer(xyz, pre=0):
    n, A = xyz.shape[:2]
    buf = np.full(pre + xyz.size, np.nan, dtype=np.float32)
    buf[pre:] = xyz.reshape(-1)
    return buf, (n, pre, 3 * A, 3, 1)


def run(buf, layout, defs, A, unit=0.1, every=1):
    from deep_cartograph_amd import hip

    n, off, fs, as_, cs = layout
    lay = ((n + every - 1) // every, off, fs * every, as_, cs)
    return hip.featurize(torch.from_numpy(buf).cuda(), np.asarray(defs, dtype=np.int32), A, strides=lay, unit=unit).cpu().numpy()


def assert_matches_oracle(got, xyz, defs, unit=0.1):
    """Every written entry equals float32(oracle) up to 1 float32 ulp (the oracle's float64 value and the kernel's may
    fall on either side of a rounding boundary)."""
    ref = fo.featurize(xyz, defs, unit=unit, n_cols=got.shape[1])
    written = ~np.isnan(ref)
    assert np.isfinite(got[written]).all()
    ulps = fo.ulp_distance_f32(got[written], ref[written].astype(np.float32))
    assert ulps.max() <= 1, f"{int((ulps > 1).sum())} entries off by up to {int(ulps.max())} float32 ulp"
    return ref


def random_coordinates(n, A, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.standard_normal((n, A, 3)) * 12).astype(np.float32)


def mixed_definitions(A, n_defs, seed):
    """All three kinds, random atoms (repeats allowed between records, distinct inside one), packed columns."""
    rng = np.random.Generator(np.random.PCG64(seed))
    defs, col = [], 0
    for d in range(n_defs):
        kind = (D, SC, T)[d % 3]
        atoms = rng.choice(A, size=4, replace=False)
        defs.append([kind, *atoms.tolist(), col])
        col += fo.COLUMNS[kind]
    return np.asarray(defs, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ 1. parity with PLUMED
@pytest.mark.parametrize("key", ["dihedrals", "distances"])
def test_fixture_parity_with_plumed_and_oracle(golden, fixture_case, key):
    """|got - printed| <= 5e-5 + 2.5e-7 on every entry: PLUMED's %.4f rounding plus half a float32 ulp at the largest
    distance (6.47 nm, ulp 4.8e-7); the float64 compute error is below 1e-12.  `printed` is the golden rounded back to
    the 4 decimals PLUMED printed (the .npz keeps them as float32, up to 2.4e-7 away, which the bound has no term for).
    The DCD file is read in place: the memory-mapped float32 view goes to the device as it is."""
    from deep_cartograph_amd import hip

    traj, case = fixture_case["traj"], fixture_case[key]
    flat = torch.from_numpy(np.array(traj.data)).cuda()
    got = hip.featurize(flat, case["defs"], traj.n_atoms, strides=traj.layout()).cpu().numpy()
    printed = np.round(golden[key].astype(np.float64), 4)
    assert got.shape == printed.shape and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - printed).max()
    print(f"{key}: max |got - PLUMED| = {err:.6e}")
    assert err <= 5e-5 + 2.5e-7
    ulps = fo.ulp_distance_f32(got, case["oracle"].astype(np.float32))
    print(f"{key}: {int((ulps > 0).sum())} of {ulps.size} entries differ from float32(oracle), max {int(ulps.max())} ulp")
    assert ulps.max() <= 1
    # the dense (n, A, 3) layout of the same frames: the same bits
    dense = hip.featurize(torch.from_numpy(fixture_case["xyz"]).cuda(), case["defs"], traj.n_atoms).cpu().numpy()
    assert np.array_equal(dense, got)


# ------------------------------------------------------------------------------------------------ 2. kernel edges
@pytest.mark.parametrize("n", [1, 63, 65, TILE + 1])
@pytest.mark.parametrize("A,n_defs", [(4, 1), (4, 7), (37, 50), (104, 300)])
def test_layouts_agree_bit_for_bit(n, A, n_defs):
    """Dense rows and DCD planes of the same frames, every alignment of the base pointer; frame counts around the wave
    and one past the frame tile; one record, fewer records than lanes, more than one pass over the records; column counts
    (1, 9, 67, 400): odd, and not multiples of 64."""
    xyz = random_coordinates(n, A, 1000 * A + n)
    defs = mixed_definitions(A, n_defs, A + n_defs)
    ref = None
    for pre in range(4):
        for buf, layout in (dense_buffer(xyz, pre), planes_buffer(xyz, pre), planes_buffer(xyz, pre, cell=True)):
            got = run(buf, layout, defs, A)
            if ref is None:
                ref = got
                assert got.shape == (n, fo.n_columns(defs))
                assert_matches_oracle(got, xyz, defs)
            assert np.array_equal(got, ref), f"pre={pre} layout={layout}"


def test_repeated_atoms_collinear_and_coincident():
    xyz = np.zeros((3, 8, 3), dtype=np.float32)
    xyz[:, 0:4] = [[0, 0, 0], [1, 1, 1], [2, 2, 2], [5, 5, 5]]            # collinear along a diagonal: products cancel exactly
    xyz[:, 4:8] = [[1.5, 0, 0], [0, 0, 0], [0, 0, 1.25], [0, 2.5, 1.25]]  # a right angle
    xyz[1] *= np.float32(3.7)
    xyz[2] += np.float32(11.3)
    defs = [[SC, 0, 1, 2, 3, 0], [T, 0, 1, 2, 3, 2], [D, 0, 3, 0, 0, 3], [D, 2, 2, 0, 0, 4],      # collinear, coincident
            [SC, 4, 5, 5, 6, 5], [SC, 4, 4, 4, 4, 7], [SC, 5, 5, 6, 7, 9],                        # repeated atoms inside a torsion
            [SC, 4, 5, 6, 7, 11], [T, 4, 5, 6, 7, 13], [SC, 7, 6, 5, 4, 14], [D, 4, 7, 0, 0, 16]]
    for buf, layout in (dense_buffer(xyz), planes_buffer(xyz, 1)):
        got = run(buf, layout, defs, 8)
        assert_matches_oracle(got, xyz, defs)
        assert np.array_equal(got[:, 0:3], np.tile(np.float32([0, 1, 0]), (3, 1)))      # (sin, cos) = (0, 1), angle 0
        assert np.array_equal(got[:, 4], np.zeros(3, dtype=np.float32))                 # distance of an atom to itself
        assert np.array_equal(got[:, 5:11], np.tile(np.float32([0, 1, 0, 1, 0, 1]), (3, 1)))
        # PLUMED's sign convention (exact in frame 0; the scaled and shifted frames carry float32 coordinate rounding)
        assert np.array_equal(got[0, 11:14], np.float32([1, 0, np.pi / 2]))
        assert np.allclose(got[:, 11:14], np.float32([1, 0, np.pi / 2]), atol=1e-5)
        assert np.allclose(got[:, 14:16], np.float32([1, 0]), atol=1e-5)                # a torsion read backwards is the same


def test_plain_angles_near_pi():
    """Trans torsions a hair on either side of +-pi: the angle may legitimately come out as +pi or -pi, so it is compared
    through its sine and cosine."""
    eps = np.float32([0.0, 1e-6, -1e-6, 1e-3, -1e-3, 3e-8, -3e-8])
    xyz = np.zeros((eps.size, 4, 3), dtype=np.float32)
    xyz[:, 0] = [1, 0, 0]
    xyz[:, 2] = [0, 0, 1]
    xyz[:, 3, 0], xyz[:, 3, 1], xyz[:, 3, 2] = -1, eps, 1
    defs = [[T, 0, 1, 2, 3, 0], [SC, 0, 1, 2, 3, 1]]
    got = run(*dense_buffer(xyz), defs, 4, unit=1.0)
    ref = fo.featurize(xyz, defs, unit=1.0)
    assert np.all(np.abs(np.abs(got[:, 0]) - np.pi) < 2e-3)
    assert np.abs(np.sin(got[:, 0].astype(np.float64)) - np.sin(ref[:, 0])).max() < 2e-7    # float32 spacing at pi: 2.4e-7
    assert np.abs(np.cos(got[:, 0].astype(np.float64)) - np.cos(ref[:, 0])).max() < 1e-12 + 1e-7
    assert fo.ulp_distance_f32(got[:, 1:], ref[:, 1:].astype(np.float32)).max() <= 1


def test_wide_output_keeps_sentinels_and_gaps():
    from deep_cartograph_amd import hip

    n, A = 37, 9
    xyz = random_coordinates(n, A, 5)
    defs = np.asarray([[D, 0, 1, 0, 0, 0], [SC, 1, 2, 3, 4, 2], [T, 5, 6, 7, 8, 6]], dtype=np.int32)   # columns 1, 4, 5 unwritten
    big = torch.full((n, 13), -7.5, dtype=torch.float32, device="cuda")
    out = big[:, :8]
    assert out.stride(0) == 13
    ret = hip.featurize(torch.from_numpy(xyz).cuda(), defs, A, out=out)
    assert ret.data_ptr() == big.data_ptr()
    got = big.cpu().numpy()
    ref = fo.featurize(xyz, defs, n_cols=13, fill=-7.5)
    untouched = ref == -7.5
    assert untouched[:, [1, 4, 5, 7, 8, 12]].all() and np.array_equal(got[untouched], ref[untouched].astype(np.float32))
    assert fo.ulp_distance_f32(got[~untouched], ref[~untouched].astype(np.float32)).max() <= 1
    with pytest.raises(hip.DcvError, match="columns"):
        hip.featurize(torch.from_numpy(xyz).cuda(), defs, A, out=big[:, :6])


@pytest.mark.parametrize("every", [3])
def test_frame_stride(every):
    """traj_stride as a frame stride: rows [::3] without a copy, in both layouts and through a strided tensor view."""
    from deep_cartograph_amd import hip

    n, A = 50, 11
    xyz = random_coordinates(n, A, 9)
    defs = mixed_definitions(A, 20, 3)
    full = run(*dense_buffer(xyz), defs, A)
    for buf, layout in (dense_buffer(xyz, 2), planes_buffer(xyz, 3, cell=True)):
        got = run(buf, layout, defs, A, every=every)
        assert got.shape[0] == 17 and np.array_equal(got, full[::every])
    view = torch.from_numpy(xyz).cuda()[::every]
    assert view.stride(0) == every * 3 * A
    assert np.array_equal(hip.featurize(view, defs, A).cpu().numpy(), full[::every])


def test_sparse_subset_and_general_strides():
    """Four atoms of 300 (gathered, not copied as a range), a transposed (3, A) frame, and padded atoms (stride 7, 2)."""
    from deep_cartograph_amd import hip

    n, A = 2 * TILE + 3, 300
    xyz = random_coordinates(n, A, 21)
    defs = np.asarray([[D, 3, 299, 0, 0, 0], [SC, 3, 50, 200, 299, 1], [T, 299, 200, 50, 3, 3], [D, 50, 200, 0, 0, 4]], dtype=np.int32)
    ref = run(*dense_buffer(xyz), defs, A)
    assert_matches_oracle(ref, xyz, defs)
    assert np.array_equal(run(*planes_buffer(xyz, 1), defs, A), ref)
    # (n, 3, A) storage viewed as (n, A, 3): atom stride 1, component stride A -- planes without markers
    t = torch.from_numpy(np.ascontiguousarray(xyz.transpose(0, 2, 1))).cuda().transpose(1, 2)
    assert t.stride() == (3 * A, 1, A)
    assert np.array_equal(hip.featurize(t, defs, A).cpu().numpy(), ref)
    # every atom padded to 7 floats, components 2 apart
    padded = np.full((n, A, 7), np.nan, dtype=np.float32)
    padded[:, :, 0:6:2] = xyz
    assert np.array_equal(run(padded.reshape(-1), (n, 0, 7 * A, 7, 2), defs, A), ref)
    dense_defs = mixed_definitions(A, 90, 4)      # the same strides with most atoms used: still gathered (stride != 1)
    assert np.array_equal(run(padded.reshape(-1), (n, 0, 7 * A, 7, 2), dense_defs, A), run(*dense_buffer(xyz), dense_defs, A))


def test_many_atoms_shrink_the_tile_and_too_many_are_refused():
    """2000 atoms: 24 KB of LDS per frame, two frames per workgroup.  5462 atoms do not fit one frame: DCV_EINVAL."""
    from deep_cartograph_amd import hip

    n, A = 5, 2000
    xyz = random_coordinates(n, A, 33)
    defs = np.stack([np.zeros(A // 2, dtype=np.int32), np.arange(0, A, 2), np.arange(A - 1, 0, -2), np.zeros(A // 2), np.zeros(A // 2),
                     np.arange(A // 2)], axis=1).astype(np.int32)
    for buf, layout in (dense_buffer(xyz, 1), planes_buffer(xyz, 2)):
        assert_matches_oracle(run(buf, layout, defs, A), xyz, defs)
    # 5000 atoms: one frame is 60 000 bytes, above the 48 KB budget and inside the 64 KB a launch may ask for; tile of 1
    A = 5000
    xyz = random_coordinates(3, A, 34)
    defs = np.stack([np.zeros(A // 2, dtype=np.int32), np.arange(0, A, 2), np.arange(A - 1, 0, -2), np.zeros(A // 2), np.zeros(A // 2),
                     np.arange(A // 2)], axis=1).astype(np.int32)
    for buf, layout in (dense_buffer(xyz, 3), planes_buffer(xyz, 1)):
        assert_matches_oracle(run(buf, layout, defs, A), xyz, defs)
    A = 5462
    defs = np.stack([np.zeros(A // 2, dtype=np.int32), np.arange(0, A, 2), np.arange(1, A, 2), np.zeros(A // 2), np.zeros(A // 2),
                     np.arange(A // 2)], axis=1).astype(np.int32)
    with pytest.raises(hip.DcvError, match="LDS"):
        hip.featurize(torch.zeros(2, A, 3, device="cuda"), defs, A)


def test_no_frames_give_an_empty_result():
    from deep_cartograph_amd import hip

    out = hip.featurize(torch.zeros(0, 6, 3, device="cuda"), [[SC, 0, 1, 2, 3, 0]], 6)
    assert tuple(out.shape) == (0, 2) and out.dtype == torch.float32


def test_non_finite_coordinates_propagate():
    xyz = random_coordinates(20, 6, 2)
    xyz[7, 2, 1] = np.nan
    xyz[9, 5, 0] = np.inf
    defs = [[D, 0, 1, 0, 0, 0], [D, 2, 3, 0, 0, 1], [SC, 0, 1, 2, 3, 2], [T, 1, 2, 3, 4, 4], [D, 4, 5, 0, 0, 5], [SC, 0, 1, 3, 4, 6]]
    got = run(*planes_buffer(xyz), defs, 6)
    bad = np.zeros_like(got, dtype=bool)
    bad[7, 1:5] = True
    assert np.isnan(got[bad]).all() and np.isinf(got[9, 5]) and np.isfinite(got[~bad & ~np.isinf(got)]).all()
    assert np.isfinite(got[:, [0, 6, 7]]).all()


def test_error_codes_leave_the_output_untouched():
    """DCV_EINVAL for a bad atom index, a bad column and a bad kind, DCV_ENOMEM for a short workspace: each before
    anything is launched."""
    from deep_cartograph_amd import _lib

    lib = _lib.load()
    n, A = 10, 5
    xyz = torch.from_numpy(random_coordinates(n, A, 1)).cuda()
    out = torch.full((n, 4), 123.0, dtype=torch.float32, device="cuda")
    good = [[D, 0, 1, 0, 0, 0], [SC, 0, 1, 2, 3, 1], [T, 1, 2, 3, 4, 3]]
    need = lib.dcv_featurize_workspace(n, A, 3)
    assert need >= 3 * 24 + 4 * A
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def call(defs, ws_bytes=need, ldo=4):
        d = np.ascontiguousarray(defs, dtype=np.int32)
        rc = lib.dcv_featurize(xyz.data_ptr(), n, 3 * A, 3, 1, A, d.ctypes.data, len(d), 0.1, out.data_ptr(), ldo, ws.data_ptr(), ws_bytes, None)
        torch.cuda.synchronize()
        return rc

    cases = {"atom index": ([[D, 0, A, 0, 0, 0]], need, -1), "negative atom": ([[T, 0, 1, -1, 2, 0]], need, -1),
             "column": ([[D, 0, 1, 0, 0, 4]], need, -1), "second column of a pair": ([[SC, 0, 1, 2, 3, 3]], need, -1),
             "negative column": ([[D, 0, 1, 0, 0, -1]], need, -1), "kind": ([[3, 0, 1, 2, 3, 0]], need, -1),
             "bad record after good ones": (good + [[D, 0, 9, 0, 0, 0]], lib.dcv_featurize_workspace(n, A, 4), -1),
             "workspace": (good, need - 1, -3)}
    for what, (defs, ws_bytes, code) in cases.items():
        assert call(defs, ws_bytes) == code, what
        assert lib.dcv_last_error().decode().startswith("dcv_featurize"), what
        assert bool((out == 123.0).all()), f"{what}: the output was written"
    assert call(good) == 0 and bool((out != 123.0).all())
    assert lib.dcv_featurize_workspace(n, 0, 3) == 0 and lib.dcv_featurize_workspace(n, A, 0) == 0


# ------------------------------------------------------------------------------------------------ 3. the tool
def tool_configuration(features, **extra):
    return json.loads(json.dumps({"plumed_settings": {"traj_stride": 1, "features": features}, **extra}))


def test_tool_chunks_stride_restart_and_formats(fixture_files, fixture_case, tmp_path, caplog):
    import logging

    from deep_cartograph_amd import colvars, tools

    caplog.set_level(logging.INFO, logger="deep_cartograph_amd.tools")

    dcd, pdb = fixture_files
    case = fixture_case["dihedrals"]
    one = tools.compute_features(tool_configuration(VIRTUAL_DIHEDRALS), [dcd], [pdb], output_folder=str(tmp_path / "one"))
    assert one == [str(tmp_path / "one" / "CA_example" / "colvars.npy")]
    X, names, labels = colvars.load_feature_matrix(one)
    assert X.shape == (164, 202) and names == case["names"] and not labels.any()
    assert fo.ulp_distance_f32(X, case["oracle"].astype(np.float32)).max() <= 1
    assert not os.path.exists(tmp_path / "one" / "CA_example" / "colvars.partial.npy")
    # a budget of 60 frames (input record + output row each): chunks of 60, 60, 44 -- the same bits
    per_frame = 4 * (3 * (104 + 2) + 202)
    many = tools.compute_features(tool_configuration(VIRTUAL_DIHEDRALS), dcd, pdb, output_folder=str(tmp_path / "many"),
                                  memory_budget=60 * per_frame + 100)
    assert "164 frames of CA_example.dcd in chunks of 60 frames" in caplog.text     # three chunks did run
    assert np.array_equal(np.load(many[0]), X)
    # traj_stride: the argument wins over the configuration; rows [::5]
    cfg = tool_configuration(VIRTUAL_DIHEDRALS)
    cfg["plumed_settings"]["traj_stride"] = 2
    strided = tools.compute_features(cfg, [dcd], [pdb], traj_stride=5, output_folder=str(tmp_path / "s5"), memory_budget=10 * 5 * per_frame)
    assert "33 frames of CA_example.dcd in chunks of 14 frames" in caplog.text
    assert np.array_equal(np.load(strided[0]), X[::5])
    assert np.array_equal(np.load(tools.compute_features(cfg, [dcd], [pdb], output_folder=str(tmp_path / "s2"))[0]), X[::2])
    # restart: an existing output is returned as it is
    np.save(strided[0], np.zeros((2, 202), dtype=np.float32))
    again = tools.compute_features(cfg, [dcd], [pdb], traj_stride=5, output_folder=str(tmp_path / "s5"))
    assert again == strided and np.load(again[0]).shape == (2, 202)
    # the text format, and a .npy trajectory as input
    np.save(tmp_path / "frames.npy", fixture_case["xyz"])
    dat = tools.compute_features(tool_configuration(VIRTUAL_DIHEDRALS, colvars_format="dat"), [str(tmp_path / "frames.npy")], [pdb],
                                 output_folder=str(tmp_path / "dat"))
    assert dat == [str(tmp_path / "dat" / "frames" / "colvars.dat")] and os.listdir(tmp_path / "dat" / "frames") == ["colvars.dat"]
    Xt, names_t, _ = colvars.load_feature_matrix(dat)
    assert names_t == names and np.abs(Xt.astype(np.float64) - X).max() <= 5e-9 + 6e-8   # %.8f, then float32 again
    # distances and dihedrals in one run, distance columns first
    both = tools.compute_features(tool_configuration({**VIRTUAL_DIHEDRALS, **DISTANCES}), [dcd], [pdb], output_folder=str(tmp_path / "both"))
    Xb, names_b, _ = colvars.load_feature_matrix(both)
    assert names_b == fixture_case["distances"]["names"] + names and np.array_equal(Xb[:, 1078:], X)
    assert fo.ulp_distance_f32(Xb[:, :1078], fixture_case["distances"]["oracle"].astype(np.float32)).max() <= 1


def test_tool_refuses_mismatched_inputs(fixture_files, tmp_path):
    from deep_cartograph_amd import tools

    dcd, pdb = fixture_files
    with open(pdb) as f:
        lines = f.readlines()
    short = str(tmp_path / "short.pdb")
    with open(short, "w") as f:
        f.writelines(lines[:-5])
    with pytest.raises(ValueError, match="104 atoms in the trajectory, 10[0-3] in the topology"):
        tools.compute_features(tool_configuration(VIRTUAL_DIHEDRALS), [dcd], [short], output_folder=str(tmp_path / "x"))
    with pytest.raises(FileNotFoundError):
        tools.compute_features(tool_configuration(VIRTUAL_DIHEDRALS), [str(tmp_path / "none.dcd")], [pdb], output_folder=str(tmp_path / "y"))
    with pytest.raises(ValueError, match="search_mode"):
        tools.compute_features({"plumed_settings": {"features": {"dihedral_groups": {"t": {"selection": "all"}}}}}, [dcd], [pdb],
                               output_folder=str(tmp_path / "z"))


# ------------------------------------------------------------------------------------------------ 4. the pipeline
def _members(model_zip):
    with zipfile.ZipFile(model_zip) as z:
        return {name: z.read(name) for name in z.namelist() if name.endswith((".npy", ".txt"))}


def test_deep_carto_from_trajectories(fixture_files, tmp_path):
    from deep_cartograph_amd import deep_carto, tools

    dcd, pdb = fixture_files
    filt = {"filter_settings": {"diptest_significance_level": 0.05}, "sampling_settings": {"relaxation_time": 1}}
    train = {"cvs": ["pca"], "common": {"dimension": 2, "features_normalization": "mean_std"}}
    cfg = {"compute_features": tool_configuration(VIRTUAL_DIHEDRALS), "filter_features": filt, "train_colvars": train,
           "traj_cluster": {"run": False}}
    out = deep_carto.deep_cartograph(json.loads(json.dumps(cfg)), [], trajectory_data=[dcd], topology_data=[pdb],
                                     output_folder=str(tmp_path / "from_traj"))
    run_dir = tmp_path / "from_traj"
    assert os.path.exists(run_dir / "compute_features" / "CA_example" / "colvars.npy")
    assert os.path.exists(run_dir / "filter_features" / "filtered_features.txt")
    csv = out["train_colvars"]["pca"][0]
    assert os.path.basename(os.path.dirname(csv)) == "CA_example"
    # the same as computing the features with the tool and feeding the matrix
    colvars_path = tools.compute_features(tool_configuration(VIRTUAL_DIHEDRALS), [dcd], [pdb], output_folder=str(tmp_path / "cf"))
    cfg.pop("compute_features")
    out2 = deep_carto.deep_cartograph(json.loads(json.dumps(cfg)), colvars_path, output_folder=str(tmp_path / "from_colvars"))
    a, b = pd.read_csv(csv), pd.read_csv(out2["train_colvars"]["pca"][0])
    assert len(a) == 164 and a.equals(b)
    m1 = _members(str(run_dir / "train_colvars" / "pca" / "model.zip"))
    m2 = _members(str(tmp_path / "from_colvars" / "train_colvars" / "pca" / "model.zip"))
    assert m1 and m1 == m2
    # supplementary trajectories are featurised and projected too
    sup = str(tmp_path / "sup.npy")
    from deep_cartograph_amd import trajectory as tr
    np.save(sup, tr.open_trajectory(dcd, 104).frames(0, 40))
    cfg["compute_features"] = tool_configuration(VIRTUAL_DIHEDRALS)
    out3 = deep_carto.deep_cartograph(json.loads(json.dumps(cfg)), [], trajectory_data=[dcd], topology_data=[pdb], sup_trajectory_data=[sup],
                                      output_folder=str(tmp_path / "with_sup"))
    sup_csv = pd.read_csv(out3["traj_projection"]["pca"][0])
    assert len(sup_csv) == 40 and np.allclose(sup_csv.to_numpy()[:, :2], a.to_numpy()[:40, :2], atol=2e-4)
    with pytest.raises(ValueError, match="topology_data"):
        deep_carto.deep_cartograph(json.loads(json.dumps(cfg)), [], trajectory_data=[dcd], output_folder=str(tmp_path / "no_top"))
