"""align_trajectories on the device: dcv_transform_frames / hip.transform_frames against the float64 oracle
(tests/align_oracle.py) over every pairing of input and output layouts and alignments, its guard bands and refusals,
its agreement with hip.superpose, and tools.align_trajectories on the reference's own trajectory.

Bounds.  An identity transform is exact: (double)x - 0 is x, x * 1 + y * 0 + z * 0 + 0 is x, and float32(x) is x again,
so the output equals the input bit for bit.  A general transform is one float64 expression evaluated in the oracle's
order and rounded once: 0 ulp is expected, and 1 float32 ulp is allowed as in tests/test_geometry_gpu.py (where the
transform itself comes from two different fit algorithms, a value may fall on either side of a rounding boundary)."""
import os

import numpy as np
import pytest
import torch

from deep_cartograph_amd import _lib
from tests import align_oracle as ao
from tests import features_oracle as fo
from tests import geometry_oracle as go
from tests.conftest import load_golden
from tests.test_compute_features_gpu import dense_buffer, planes_buffer

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x7FC0BEEF)   # a NaN with a payload: no coordinate the kernel writes has these bits
GUARD = 8                          # untouched words on both ends of every output buffer (a multiple of 4: keeps the alignment)


def coordinates(n, A, seed, scale=300.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(-scale, scale, (n, A, 3)).astype(np.float32)


def identity_rows(n):
    return np.tile(ao.IDENTITY_ROW, (n, 1))


def inputs(xyz):
    """{name: (flat buffer, layout)}: dense rows, DCD planes, DCD planes behind a unit-cell block, each 0-3 floats off
    the 16-byte grid."""
    out = {}
    for pre in range(4):
        out[f"dense+{pre}"] = dense_buffer(xyz, pre)
        out[f"planes+{pre}"] = planes_buffer(xyz, pre)
        out[f"cell+{pre}"] = planes_buffer(xyz, pre, cell=True)
    return out


def target(kind, n, A, shift, gap=0):
    """(sentinel-filled buffer, out_strides, index [n, A, 3] of the coordinate slots): a dense array or a DCD record
    image, `shift` floats off the 16-byte grid, GUARD words on both ends, `gap` untouched words between frames."""
    words = 3 * A if kind == "dense" else 3 * (A + 2)
    fs = words + gap
    buf = np.full(GUARD + shift + n * fs + GUARD, SENTINEL, dtype=np.uint32)
    off, as_, cs = (GUARD + shift, 3, 1) if kind == "dense" else (GUARD + shift + 1, 1, A + 2)
    idx = (off + fs * np.arange(n)[:, None, None] + as_ * np.arange(A)[None, :, None] + cs * np.arange(3)[None, None, :])
    return buf, (off, fs, as_, cs), idx


def launch(xyz_d, layout, A, rows_d, kind, shift, gap=0):
    """Run into a sentinel-filled target; returns the coordinates [n, A, 3] after checking that nothing else changed."""
    from deep_cartograph_amd import hip

    n = layout[0]
    buf, strides, idx = target(kind, n, A, shift, gap)
    out = torch.from_numpy(buf.view(np.float32)).cuda()
    ret = hip.transform_frames(xyz_d, A, rows_d, strides=layout, out=out, out_strides=strides)
    assert ret is out
    got = out.cpu().numpy().view(np.uint32)
    rest = np.ones(got.size, dtype=bool)
    rest[idx.reshape(-1)] = False
    assert (got[rest] == SENTINEL).all(), f"{int((got[rest] != SENTINEL).sum())} words outside the coordinate slots were written"
    return got[idx].view(np.float32)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


@pytest.mark.parametrize("A", [1, 3, 4, 5, 63, 64, 65, 257, 5462, 70001])
def test_identity_copies_every_layout_and_alignment_bit_for_bit(A):
    """12 input forms x 8 output forms: every input base mod 4 with every output base mod 4, dense and planes on both
    sides, and a frame stride of two records.  5 462 atoms are past the LDS limit of the staged kernels, 70 001 past 65 535."""
    from deep_cartograph_amd import hip

    n = 17 if A <= 5 else (5 if A <= 257 else 3)
    xyz = coordinates(n, A, seed=A)
    rows = torch.from_numpy(identity_rows(n)).cuda()
    for name, (buf, layout) in inputs(xyz).items():
        xyz_d = torch.from_numpy(buf).cuda()
        for kind in ("dense", "image"):
            for shift in range(4):
                got = launch(xyz_d, layout, A, rows, kind, shift)
                assert same_bits(got, xyz), f"{name} -> {kind}+{shift}"
        m, off, fs, as_, cs = layout
        every = ((m + 1) // 2, off, 2 * fs, as_, cs)
        for kind in ("dense", "image"):
            got = launch(xyz_d, every, A, rows[: every[0]], kind, 1)
            assert same_bits(got, xyz[::2]), f"{name}, every second frame -> {kind}"
        if name in ("dense+0", "planes+1"):   # the default output: a new (n, A, 3) tensor
            new = hip.transform_frames(xyz_d, A, rows, strides=layout)
            assert new.shape == (n, A, 3) and new.dtype == torch.float32 and same_bits(new.cpu().numpy(), xyz)
    dense = torch.from_numpy(xyz).cuda()
    assert same_bits(hip.transform_frames(dense, A, rows).cpu().numpy(), xyz)   # a (n, A, 3) tensor through its own strides


@pytest.mark.parametrize("A", [5, 104, 257])
def test_guard_bands_markers_and_gaps_keep_their_contents(A):
    """General transforms into buffers that are longer than needed on both ends and have 5 unused words between frames:
    every word that is not a coordinate slot -- record markers, gaps, both ends -- still holds the sentinel (checked in
    `launch`), for planes and dense targets and a strided (neither dense nor planes) target."""
    from deep_cartograph_amd import hip

    n = 9
    xyz = coordinates(n, A, seed=100 + A)
    rows = ao.random_transforms(n, seed=A)
    want = ao.transform(xyz, rows).astype(np.float32)
    rows_d = torch.from_numpy(rows).cuda()
    for name, (buf, layout) in (("dense", dense_buffer(xyz, 3)), ("planes", planes_buffer(xyz, 2))):
        xyz_d = torch.from_numpy(buf).cuda()
        for kind in ("dense", "image"):
            for shift in (0, 3):
                got = launch(xyz_d, layout, A, rows_d, kind, shift, gap=5)
                assert fo.ulp_distance_f32(got, want).max() <= 1, (name, kind, shift)
        # atoms 4 floats apart, components 1 apart: a slot of 4 words per atom of which the last stays untouched
        fs = 4 * A + 3
        out = torch.from_numpy(np.full(GUARD + n * fs + GUARD, SENTINEL, dtype=np.uint32).view(np.float32)).cuda()
        hip.transform_frames(xyz_d, A, rows_d, strides=layout, out=out, out_strides=(GUARD, fs, 4, 1))
        got = out.cpu().numpy().view(np.uint32)
        idx = GUARD + fs * np.arange(n)[:, None, None] + 4 * np.arange(A)[None, :, None] + np.arange(3)[None, None, :]
        rest = np.ones(got.size, dtype=bool)
        rest[idx.reshape(-1)] = False
        assert (got[rest] == SENTINEL).all()
        assert fo.ulp_distance_f32(got[idx].view(np.float32), want).max() <= 1


@pytest.mark.parametrize("A", [3, 104, 257, 5462])
def test_general_transforms_match_the_oracle(A):
    """Seeded proper rotations and centroids of a few hundred Angstrom, another transform in every frame: within 1
    float32 ulp of float32(oracle), 0 expected; dense and planes layouts give the same bits.  With 104 atoms a workgroup
    holds several frames and waves straddle them; with 257 and more most waves sit inside one frame."""
    n = 33 if A <= 257 else 5
    xyz = coordinates(n, A, seed=200 + A)
    rows = ao.random_transforms(n, seed=300 + A)
    want = ao.transform(xyz, rows).astype(np.float32)
    rows_d = torch.from_numpy(rows).cuda()
    results = {}
    for name, (buf, layout) in (("dense", dense_buffer(xyz, 0)), ("dense+1", dense_buffer(xyz, 1)), ("planes", planes_buffer(xyz, 0)),
                                ("cell+3", planes_buffer(xyz, 3, cell=True))):
        xyz_d = torch.from_numpy(buf).cuda()
        for kind, shift in (("dense", 0), ("image", 0), ("image", 2)):
            results[f"{name} -> {kind}+{shift}"] = launch(xyz_d, layout, A, rows_d, kind, shift)
    worst = max(int(fo.ulp_distance_f32(got, want).max()) for got in results.values())
    print(f"transform_frames, {A} atoms: at most {worst} float32 ulp from float32(oracle)")
    assert worst <= 1
    first = next(iter(results.values()))
    for name, got in results.items():
        assert np.isfinite(got).all() and same_bits(got, first), name
    # a row stride of the transforms above 16
    wide = torch.zeros(n, 24, dtype=torch.float64, device="cuda")
    wide[:, :16] = rows_d
    buf, layout = planes_buffer(xyz, 1)
    assert same_bits(launch(torch.from_numpy(buf).cuda(), layout, A, wide, "image", 0), first)
    assert same_bits(launch(torch.from_numpy(buf).cuda(), layout, A, wide[:, :15], "image", 0), first)


def test_a_nan_row_poisons_its_frame_only_and_no_frames_launch_nothing():
    from deep_cartograph_amd import hip

    n, A = 7, 104
    xyz = coordinates(n, A, seed=5)
    rows = ao.random_transforms(n, seed=6)
    rows[2, 9] = np.nan     # c_mob x: every component of the frame
    rows[5, 13] = np.inf    # c_ref y: that component of the frame
    want = ao.transform(xyz, rows).astype(np.float32)
    buf, layout = planes_buffer(xyz, 1)
    got = launch(torch.from_numpy(buf).cuda(), layout, A, torch.from_numpy(rows).cuda(), "image", 0)
    assert np.isnan(got[2]).all() and np.isinf(got[5][:, 1]).all() and np.isfinite(got[5][:, [0, 2]]).all()
    keep = [0, 1, 3, 4, 6]
    assert np.isfinite(got[keep]).all() and fo.ulp_distance_f32(got[keep], want[keep]).max() <= 1
    # no frames: an empty result, and a given buffer stays as it is
    empty = hip.transform_frames(torch.empty(0, A, 3, dtype=torch.float32, device="cuda"), A, torch.empty(0, 16, dtype=torch.float64, device="cuda"))
    assert empty.shape == (0, A, 3)
    sentinel = torch.from_numpy(np.full(64, SENTINEL, dtype=np.uint32).view(np.float32)).cuda()
    hip.transform_frames(torch.from_numpy(buf).cuda(), A, torch.empty(0, 16, dtype=torch.float64, device="cuda"), strides=(0,) + layout[1:],
                         out=sentinel, out_strides=(0, 3 * A, 3, 1))
    assert (sentinel.cpu().numpy().view(np.uint32) == SENTINEL).all()
    lib = _lib.load()
    x = torch.from_numpy(buf).cuda()
    assert lib.dcv_transform_frames(x.data_ptr(), 0, 3 * A, 3, 1, A, sentinel.data_ptr(), 16, sentinel.data_ptr(), 3 * A, 3, 1, None) == 0


def test_refusals_leave_the_output_untouched():
    from deep_cartograph_amd import hip

    n, A = 4, 10
    xyz = coordinates(n, A, seed=9)
    rows = torch.from_numpy(ao.random_transforms(n, seed=10)).cuda()
    x = torch.from_numpy(xyz.reshape(-1)).cuda()
    out = torch.from_numpy(np.full(n * A * 3 + 16, SENTINEL, dtype=np.uint32).view(np.float32)).cuda()
    lib = _lib.load()
    EINVAL = -1

    def call(xyz_ptr=None, n_frames=n, strides=(3 * A, 3, 1), n_atoms=A, t_ptr=None, ldt=16, out_ptr=None, out_strides=(3 * A, 3, 1)):
        return lib.dcv_transform_frames(x.data_ptr() if xyz_ptr is None else xyz_ptr, n_frames, *strides, n_atoms,
                                        rows.data_ptr() if t_ptr is None else t_ptr, ldt, out.data_ptr() if out_ptr is None else out_ptr,
                                        *out_strides, None)

    assert call(ldt=14) == EINVAL and b"ldt" in lib.dcv_last_error()
    assert call(out_strides=(3 * A, 0, 1)) == EINVAL
    assert call(out_strides=(0, 3, 1)) == EINVAL
    assert call(strides=(-1, 3, 1)) == EINVAL
    assert call(strides=(3 * A, 3, 0)) == EINVAL
    assert call(n_atoms=0) == EINVAL and call(n_frames=-1) == EINVAL
    assert call(xyz_ptr=0) == EINVAL and call(t_ptr=0) == EINVAL and call(out_ptr=0) == EINVAL
    # overlapping element ranges: the same buffer, and an output that begins on the input's last element
    assert call(out_ptr=x.data_ptr()) == EINVAL and b"overlap" in lib.dcv_last_error()
    assert call(out_ptr=x.data_ptr() + 4 * (n * A * 3 - 1)) == EINVAL
    assert call(xyz_ptr=out.data_ptr() + 4 * 8) == EINVAL
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all()
    assert same_bits(x.cpu().numpy(), xyz.reshape(-1))
    # the same through the wrapper
    lay = (n, 0, 3 * A, 3, 1)
    with pytest.raises(_lib.DcvError, match="overlap"):
        hip.transform_frames(x, A, rows, strides=lay, out=x, out_strides=(0, 3 * A, 3, 1))
    with pytest.raises(_lib.DcvError):
        hip.transform_frames(x, A, rows[:, :14], strides=lay)
    with pytest.raises(_lib.DcvError):
        hip.transform_frames(x, A, rows, strides=lay, out=out, out_strides=(0, 3 * A, 0, 1))
    with pytest.raises(_lib.DcvError, match="reaches element"):
        hip.transform_frames(x, A, rows, strides=lay, out=out[: n * A * 3 - 1], out_strides=(0, 3 * A, 3, 1))
    with pytest.raises(_lib.DcvError):
        hip.transform_frames(x, A, rows, strides=lay, out=out)
    with pytest.raises(_lib.DcvError):
        hip.transform_frames(x, A, rows.float(), strides=lay)
    with pytest.raises(_lib.DcvError):
        hip.transform_frames(x, A, rows[:3], strides=lay)
    with pytest.raises(_lib.DcvError):
        hip.transform_frames(x.cpu(), A, rows, strides=lay)
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all()
    # a call that is fine, in the same buffers
    hip.transform_frames(x, A, rows, strides=lay, out=out, out_strides=(8, 3 * A, 3, 1))
    assert fo.ulp_distance_f32(out.cpu().numpy()[8:8 + n * A * 3].reshape(n, A, 3), ao.transform(xyz, rows.cpu().numpy()).astype(np.float32)).max() <= 1


def test_fit_on_a_subset_then_transform_all_atoms():
    """hip.superpose fits on every 7th atom; hip.transform_frames moves all atoms with its transform rows as they are.
    The subset agrees with superpose's own `aligned` output and everything with the Kabsch oracle within 1 ulp."""
    from deep_cartograph_amd import hip

    n, A = 9, 700
    xyz, ref = go.synthetic(n, A, seed=11)
    fit = np.arange(0, A, 7)
    buf, layout = planes_buffer(xyz, 1)
    xyz_d = torch.from_numpy(buf).cuda()
    fitted = hip.superpose(xyz_d, A, fit, ref[fit], sel=fit, strides=layout, want=("transform", "aligned"))
    assert fitted["transform"].shape == (n, 16)
    moved = hip.transform_frames(xyz_d, A, fitted["transform"], strides=layout).cpu().numpy()
    subset = int(fo.ulp_distance_f32(moved[:, fit], fitted["aligned"].cpu().numpy()).max())
    want = ao.transform(xyz, ao.fit_transforms(xyz, fit, ref[fit])).astype(np.float32)
    everything = int(fo.ulp_distance_f32(moved, want).max())
    print(f"fit + transform: subset at most {subset} ulp from superpose's aligned, all atoms at most {everything} ulp from the oracle")
    assert subset <= 1 and everything <= 1


# ------------------------------------------------------------------------------------------------ the tool
@pytest.fixture(scope="module")
def systems(tmp_path_factory):
    """Two systems from the reference's trajectory (164 frames x 104 C-alpha): the original, and a copy without its
    first 5 residues, resids shifted by +500, every frame moved by its own seeded rigid motion; each as .dcd and .npy."""
    from deep_cartograph_amd import trajectory

    g = load_golden("compute_features_golden.npz")
    d = tmp_path_factory.mktemp("align_gpu")
    dcd, pdb = str(d / "CA_example.dcd"), str(d / "CA_example.pdb")
    with open(dcd, "wb") as f:
        f.write(g["dcd"].tobytes())
    with open(pdb, "w") as f:
        f.write(str(g["pdb"]))
    top = trajectory.read_topology(pdb)
    xyz = trajectory.open_trajectory(dcd, top.n_atoms).frames()
    rng = np.random.Generator(np.random.PCG64(21))
    moved = np.stack([(xyz[f, 5:].astype(np.float64) @ go.random_rotation(rng) + rng.uniform(-200, 200, 3)).astype(np.float32)
                      for f in range(len(xyz))])
    keep = np.arange(5, top.n_atoms)
    top2 = trajectory.Topology([top.names[i] for i in keep], [top.resnames[i] for i in keep], [top.chains[i] for i in keep],
                               [top.segids[i] for i in keep], top.resids[keep] + 500, moved[0].copy(), None)
    pdb2 = str(d / "moved.pdb")
    trajectory.write_topology(pdb2, top2)
    dcd2 = str(d / "moved.dcd")
    with trajectory.write_dcd(dcd2, top2.n_atoms) as w:
        image = w.image(len(moved))
        image.reshape(len(moved), 3, top2.n_atoms + 2)[:, :, 1:-1] = moved.transpose(0, 2, 1)
        w.append(image)
    np.save(str(d / "CA_example.npy"), xyz)
    np.save(str(d / "moved.npy"), moved)
    fit_ref = top.positions[5:].astype(np.float64)
    want = [ao.transform(xyz, ao.fit_transforms(xyz, np.arange(5, 104), fit_ref)).astype(np.float32),
            ao.transform(moved, ao.fit_transforms(moved, np.arange(99), fit_ref)).astype(np.float32)]
    return {"dir": d, "pdbs": [pdb, pdb2], "stems": ["CA_example", "moved"], "fit": [np.arange(5, 104), np.arange(99)],
            "fit_ref": fit_ref, "want": want}


@pytest.mark.parametrize("ext", [".dcd", ".npy"])
def test_tool_on_the_reference_trajectory(systems, ext, tmp_path):
    from deep_cartograph_amd import geometry, tools, trajectory

    trajs = [str(systems["dir"] / (stem + ext)) for stem in systems["stems"]]
    out = str(tmp_path / "aligned")
    got_trajs, got_tops = tools.align_trajectories(trajs, systems["pdbs"], ref_topology=systems["pdbs"][0], output_folder=out)
    assert got_trajs == [os.path.join(out, stem + ext) for stem in systems["stems"]]
    assert got_tops == [os.path.join(out, stem + ".pdb") for stem in systems["stems"]]
    assert sorted(os.listdir(out)) == sorted(os.path.basename(p) for p in got_trajs + got_tops)   # no .partial left
    for path, top_path, fit, want in zip(got_trajs, got_tops, systems["fit"], systems["want"]):
        traj = trajectory.open_trajectory(path, want.shape[1])
        assert traj.n_frames == 164
        got = traj.frames()
        ulps = int(fo.ulp_distance_f32(got, want).max())
        print(f"{os.path.basename(path)}: at most {ulps} float32 ulp from float32(oracle)")
        assert ulps <= 1
        worst = max(np.abs(go.kabsch(got[f, fit], systems["fit_ref"])[0] - np.eye(3)).max() for f in range(len(got)))
        print(f"{os.path.basename(path)}: re-fitted rotations within {worst:.2e} of the identity")
        assert worst < 1e-6
        written = trajectory.read_topology(top_path)
        assert written.n_atoms == want.shape[1]
        assert np.abs(written.positions.astype(np.float64) - got[0].astype(np.float64)).max() <= 0.0005 + 1e-5   # %8.3f, and float32 of it
    # chunks of 7 frames give the same files
    opened = [trajectory.open_trajectory(t) for t in trajs]
    budget = 7 * max(geometry.align_frame_bytes(t, ext == ".dcd") for t in opened) + 8
    assert all(budget // geometry.align_frame_bytes(t, ext == ".dcd") == 7 for t in opened)
    out7 = str(tmp_path / "aligned7")
    chunked, chunked_tops = tools.align_trajectories(trajs, systems["pdbs"], ref_topology=systems["pdbs"][0], output_folder=out7,
                                                     memory_budget=budget)
    for a, b in zip(got_trajs + got_tops, chunked + chunked_tops):
        assert open(a, "rb").read() == open(b, "rb").read(), os.path.basename(a)
