"""The XTC encoder on the device: dcv_xtc_encode / dcv_xtc_pack / hip.xtc_encode against the CPU oracle
(tests/xtc_encode_oracle.py), bit for bit: descriptors, slot bytes, the packed file image, guard bands around every
output, the coordinate layouts, the frame gather, marked frames, the refusals -- and traj_cluster's extraction, which is
the encoder's first user.  Shapes: 65 frames (a full wave and a partial one), 1 and 64; 10 atoms (the smallest compressed
form), 11, the staging block of 16, 17, and 104; the raw form at 9 atoms and 1."""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

from deep_cartograph_amd import _lib
from tests import xtc_encode_oracle as eo
from tests import xtc_oracle as xo
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

BAND = 256   # guard bytes on either side of an output
PDB_BOUND = 0.0005 + 2.0 ** -18   # the %8.3f of the format, and half a float32 step below 128 Angstrom when the text is read back


@functools.lru_cache(maxsize=None)
def reference(name: str, n: int, natoms: int):
    """(xyz, bodies, descriptors, status, precision) of a case, computed once and shared; callers leave it unchanged."""
    precision = eo.case_precision(name)
    xyz = eo.synthetic(name, n, natoms)
    return (xyz, *eo.encode(xyz, precision), precision)


def banded(nbytes: int):
    """A 0xFF-filled device buffer and the view of its middle ``nbytes``."""
    whole = torch.full((nbytes + 2 * BAND,), 0xFF, dtype=torch.uint8, device="cuda")
    return whole, whole[BAND:BAND + nbytes]


def check_slots(whole, bodies, desc, natoms):
    """The slot bytes equal the oracle's payloads; the bands and the tail of every slot are untouched."""
    raw = whole.cpu().numpy()
    slot = eo.slot_bytes(natoms)
    assert np.all(raw[:BAND] == 0xFF) and np.all(raw[BAND + len(bodies) * slot:] == 0xFF)
    for f, body in enumerate(bodies):
        got = raw[BAND + f * slot:BAND + (f + 1) * slot].tobytes()
        want = eo.slot_payload(body, natoms)
        assert got[:len(want)] == want, f"frame {f}: slot bytes differ"
        assert got[len(want):] == b"\xff" * (slot - len(want)), f"frame {f}: the tail of the slot was written"


def check_desc(got, want, status, want_status):
    np.testing.assert_array_equal(status.cpu().numpy(), want_status)
    for field in eo.FRAME_DTYPE.names:
        np.testing.assert_array_equal(got[field], want[field], err_msg=field)
    assert got["precision"].view(np.uint32).tolist() == want["precision"].view(np.uint32).tolist()


def encode_and_check(xyz_d, natoms, ref, strides=None, frames=None):
    """hip.xtc_encode_slots + hip.xtc_pack inside bands against the oracle of ``ref``; returns the image bytes."""
    from deep_cartograph_amd import hip

    _, bodies, desc, status, precision = ref
    n = len(bodies)
    whole, slots = banded(n * eo.slot_bytes(natoms))
    _, got, st = hip.xtc_encode_slots(xyz_d, natoms, strides=strides, frames=frames, precision=precision, slots=slots)
    torch.cuda.synchronize()
    check_desc(got, desc, st, status)
    check_slots(whole, bodies, desc, natoms)
    source = np.arange(n) if frames is None else np.asarray(frames)
    want = eo.file_image(bodies, status, natoms, frames=source)
    offsets, size = hip.xtc_image_offsets(got, status, natoms)
    assert size == len(want)
    whole_image, image = banded(size)
    hip.xtc_pack(slots, got, offsets, natoms, source, source.astype(np.float32), image=image)
    torch.cuda.synchronize()
    raw = whole_image.cpu().numpy()
    assert np.all(raw[:BAND] == 0xFF) and np.all(raw[BAND + size:] == 0xFF)
    assert raw[BAND:BAND + size].tobytes() == want
    return want


def decode_back(image: bytes, natoms: int, tmp_path):
    """The image written to a file, indexed and decoded by the project's own reader: (index, xyz [n, A, 3])."""
    from deep_cartograph_amd import hip, trajectory as tr

    path = str(tmp_path / "back.xtc")
    with tr.write_xtc(path, natoms) as w:
        w.append(image)
    idx = tr.index_xtc(path, natoms)
    first, last, desc = idx.span(np.arange(idx.n_frames))
    data = torch.from_numpy(np.frombuffer(image, dtype=np.uint8)[first:last].copy()).cuda()
    return idx, hip.xtc_decode(data, desc, natoms).cpu().numpy()


# ------------------------------------------------------------------------------------------------ cases and shapes
@pytest.mark.parametrize("natoms", [10, 11, 16, 17, 104])
@pytest.mark.parametrize("name", eo.CASES)
def test_cases_against_the_oracle(name, natoms, tmp_path):
    ref = reference(name, 65, natoms)
    xyz, _, desc, status, precision = ref
    assert not status.any()
    if name != "identical":    # identical atoms cost the same in every frame; everywhere else the lengths differ and leave the 4-byte grid
        assert len(set(desc["nbytes"].tolist())) > 1 and np.any(desc["nbytes"] % 4)
    image = encode_and_check(torch.from_numpy(xyz).cuda(), natoms, ref)
    idx, back = decode_back(image, natoms, tmp_path)
    np.testing.assert_array_equal(back.view(np.uint32), xo.to_float(eo.quantise(xyz, precision)[0], precision).view(np.uint32))
    assert idx.step.tolist() == list(range(65)) and idx.time.tolist() == [float(f) for f in range(65)] and not idx.box.any()


@pytest.mark.parametrize("n", [1, 64])
def test_frame_counts(n):
    for name, natoms in (("chain", 17), ("water", 104)):
        ref = reference(name, n, natoms)
        encode_and_check(torch.from_numpy(ref[0]).cuda(), natoms, ref)


@pytest.mark.parametrize("natoms", [9, 1])
def test_raw_form(natoms, tmp_path):
    from deep_cartograph_amd import hip

    ref = reference("chain", 65, natoms)
    xyz = ref[0]
    image = encode_and_check(torch.from_numpy(xyz).cuda(), natoms, ref)
    assert len(image) == 65 * (56 + 12 * natoms)
    idx, back = decode_back(image, natoms, tmp_path)
    assert idx.raw
    np.testing.assert_array_equal(back.view(np.uint32), (eo.scaled(xyz) * np.float32(10.0)).view(np.uint32))
    planes = torch.from_numpy(np.ascontiguousarray(xyz.transpose(0, 2, 1)).reshape(-1)).cuda()
    assert encode_and_check(planes, natoms, ref, strides=(65, 0, 3 * natoms, 1, natoms)) == image
    bad = xyz.copy()
    bad[7, 0, 2] = np.inf
    got, desc, status = hip.xtc_encode(torch.from_numpy(bad).cuda(), natoms, return_status=True)
    assert status.cpu().numpy().tolist() == [0] * 7 + [eo.NONFINITE] + [0] * 57 and got.numel() == 64 * (56 + 12 * natoms)


def dcd_records(xyz: np.ndarray, cell: bool):
    """The frames as DCD frame records viewed as float32 (markers and the unit-cell block hold NaN patterns), and the
    layout (n, offset, frame, atom, comp) of the coordinates inside."""
    n, A = xyz.shape[:2]
    head = 14 if cell else 0
    words = head + 3 * (A + 2)
    buf = np.full((n, words), np.uint32(0x7FC0BEEF), dtype=np.uint32).view(np.float32)
    for c in range(3):
        buf[:, head + c * (A + 2) + 1:head + c * (A + 2) + 1 + A] = xyz[:, :, c]
    return buf.reshape(-1), (n, head + 1, words, 1, A + 2)


@pytest.mark.parametrize("name,natoms", [("chain", 17), ("scattered", 104), ("tight", 16), ("bigsize", 11)])
def test_layouts_give_the_same_bytes(name, natoms):
    ref = reference(name, 65, natoms)
    for cell in (False, True):
        buf, layout = dcd_records(ref[0], cell)
        encode_and_check(torch.from_numpy(buf).cuda(), natoms, ref, strides=layout)   # the same oracle bytes as the dense rows
    strided = torch.from_numpy(ref[0]).cuda()[:, :, None, :].expand(-1, -1, 2, -1).contiguous()[:, :, 1, :]   # dense rows with gaps
    assert strided.stride() == (6 * natoms, 6, 1)
    encode_and_check(strided, natoms, ref)


@pytest.mark.parametrize("name,natoms", [("water", 17), ("negative", 104)])
def test_frame_indices_gather(name, natoms):
    from deep_cartograph_amd import hip

    xyz = reference(name, 65, natoms)[0]
    frames = np.array([64, 3, 3, 0, 17, 63, 1, 64, 40], dtype=np.int64)   # unsorted, with repeats
    precision = eo.case_precision(name)
    ref = (xyz[frames], *eo.encode(xyz[frames], precision), precision)
    image = encode_and_check(torch.from_numpy(xyz).cuda(), natoms, ref, frames=frames)
    buf, layout = dcd_records(xyz, True)
    assert encode_and_check(torch.from_numpy(buf).cuda(), natoms, ref, strides=layout, frames=frames) == image
    # the one-call form: the same file, steps and times from the source indices
    assert hip.xtc_encode(torch.from_numpy(xyz).cuda(), natoms, frames=frames, precision=precision).cpu().numpy().tobytes() == image
    assert [fr["step"] for fr in xo.frames(image)] == frames.tolist()


def test_marked_frames_between_good_ones():
    from deep_cartograph_amd import hip

    natoms = 17
    xyz = reference("chain", 65, natoms)[0].copy()
    xyz[5, 16, 1] = np.nan       # the last atom of a frame
    xyz[63, 0, 0] = 3.0e9        # the first atom, in the last lane of the full wave
    xyz[64, 3, 2] = -np.inf      # the only frame of the partial wave
    bodies, desc, status = eo.encode(xyz, 1000.0)
    assert status[[5, 63, 64]].tolist() == [eo.NONFINITE, eo.RANGE, eo.NONFINITE] and status.sum() == 4
    image = encode_and_check(torch.from_numpy(xyz).cuda(), natoms, (xyz, bodies, desc, status, 1000.0))   # nothing in the marked slots
    assert len(xo.frames(image)) == 62 and [fr["step"] for fr in xo.frames(image)] == [f for f in range(65) if f not in (5, 63, 64)]
    with pytest.raises(_lib.DcvError, match="frame 5 of the 65 given cannot be written: a coordinate is NaN or infinite"):
        hip.xtc_encode(torch.from_numpy(xyz).cuda(), natoms)
    got, _, st = hip.xtc_encode(torch.from_numpy(xyz).cuda(), natoms, return_status=True)
    assert got.cpu().numpy().tobytes() == image and st.cpu().numpy().tolist() == status.tolist()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_every_output_untouched():
    lib = _lib.load()
    natoms, n = 17, 8
    xyz = torch.from_numpy(reference("chain", 65, natoms)[0][:n].copy()).cuda()
    slot = lib.dcv_xtc_encode_slot_bytes(natoms)
    slots = torch.full((n * slot,), 0xFF, dtype=torch.uint8, device="cuda")
    desc = torch.full((n * 48,), 0xFF, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ws = torch.full((lib.dcv_xtc_encode_workspace(n),), 0xFF, dtype=torch.uint8, device="cuda")
    image = torch.full((n * (92 + slot),), 0xFF, dtype=torch.uint8, device="cuda")
    frames = np.arange(n, dtype=np.int64)[::-1].copy()
    stream = torch.cuda.current_stream().cuda_stream

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == 0xFF).all()) for t in (slots, desc, ws, image)) and bool((status == -7).all())

    def call(**kw):
        a = dict(xyz=xyz.data_ptr(), n_src=n, fs=3 * natoms, as_=3, cs=1, natoms=natoms, frames=frames.ctypes.data, n=n, inv_scale=0.1,
                 precision=1000.0, slots=slots.data_ptr(), slots_bytes=slots.numel(), desc=desc.data_ptr(), status=status.data_ptr(),
                 ws=ws.data_ptr(), ws_bytes=ws.numel())
        a.update(kw)
        return lib.dcv_xtc_encode(a["xyz"], a["n_src"], a["fs"], a["as_"], a["cs"], a["natoms"], a["frames"], a["n"], a["inv_scale"], a["precision"],
                                  a["slots"], a["slots_bytes"], a["desc"], a["status"], a["ws"], a["ws_bytes"], stream)

    for bad in (dict(xyz=None), dict(slots=None), dict(desc=None), dict(status=None), dict(natoms=0), dict(n=-1),
                dict(xyz=xyz.data_ptr() + 2), dict(slots=slots.data_ptr() + 1), dict(status=status.data_ptr() + 2), dict(desc=desc.data_ptr() + 4),
                dict(fs=0), dict(as_=0), dict(cs=0), dict(cs=-1),
                dict(precision=0.0), dict(precision=-1000.0), dict(precision=float("nan")), dict(precision=float("inf")),
                dict(slots=xyz.data_ptr()), dict(status=slots.data_ptr() + 8), dict(desc=slots.data_ptr()),
                dict(frames=None, n=n + 1)):
        assert call(**bad) == -1 and untouched(), bad
    for index in (-1, n):
        wrong = frames.copy()
        wrong[3] = index
        assert call(frames=wrong.ctypes.data) == -1 and b"frame index" in lib.dcv_last_error() and untouched()
    assert call(ws_bytes=ws.numel() - 1) == -3 and untouched()           # DCV_ENOMEM: a short workspace
    assert call(ws=None) == -3 and untouched()
    assert call(slots_bytes=n * slot - 1) == -3 and untouched()          # a short slot buffer
    assert call(n=0) == 0 and call(n=0, frames=None, xyz=None) == 0 and untouched()
    assert call(frames=None, ws=None, ws_bytes=0) == 0                   # without indices no workspace is needed
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any() and bool((ws == 0xFF).all())
    desc_h = desc.cpu().numpy().view(_lib.XTC_FRAME_DTYPE)
    offsets = np.cumsum(92 + (desc_h["nbytes"].astype(np.int64) + 3) // 4 * 4)
    offsets = np.concatenate([[0], offsets[:-1]])
    step, time = np.arange(n, dtype=np.int32), np.arange(n, dtype=np.float32)
    pws = torch.full((lib.dcv_xtc_pack_workspace(n),), 0xFF, dtype=torch.uint8, device="cuda")

    def pack(**kw):
        a = dict(slots=slots.data_ptr(), slots_bytes=slots.numel(), desc=desc_h.ctypes.data, offsets=offsets.ctypes.data, step=step.ctypes.data,
                 time=time.ctypes.data, box=None, n=n, natoms=natoms, image=image.data_ptr(), image_bytes=image.numel(), ws=pws.data_ptr(),
                 ws_bytes=pws.numel())
        a.update(kw)
        return lib.dcv_xtc_pack(a["slots"], a["slots_bytes"], a["desc"], a["offsets"], a["step"], a["time"], a["box"], a["n"], a["natoms"], a["image"],
                                a["image_bytes"], a["ws"], a["ws_bytes"], stream)

    def image_untouched():
        torch.cuda.synchronize()
        return bool((image == 0xFF).all()) and bool((pws == 0xFF).all())

    overlap, off_grid, raw_flag, long_payload = offsets.copy(), offsets.copy(), desc_h.copy(), desc_h.copy()
    overlap[2] -= 4
    off_grid[1:] += 2
    raw_flag["raw"][1] = 1
    long_payload["nbytes"][0] = slot + 1
    for bad in (dict(slots=None), dict(image=None), dict(step=None), dict(time=None), dict(offsets=None), dict(desc=None), dict(natoms=0), dict(n=-1),
                dict(image=image.data_ptr() + 2), dict(slots=slots.data_ptr() + 2), dict(offsets=overlap.ctypes.data), dict(offsets=off_grid.ctypes.data),
                dict(desc=raw_flag.ctypes.data), dict(desc=long_payload.ctypes.data), dict(image_bytes=int(offsets[-1]) + 91),
                dict(slots_bytes=int(desc_h["offset"][-1])), dict(image=slots.data_ptr(), image_bytes=slots.numel())):
        assert pack(**bad) == -1 and image_untouched(), bad
    assert pack(ws_bytes=pws.numel() - 1) == -3 and pack(ws=None) == -3 and image_untouched()
    assert pack(n=0) == 0 and image_untouched()
    assert pack() == 0
    torch.cuda.synchronize()
    ref = eo.encode(xyz.cpu().numpy(), 1000.0)
    want = eo.file_image(ref[0], ref[2], natoms)
    assert image.cpu().numpy()[:len(want)].tobytes() == want and bool((image[len(want):] == 0xFF).all())


def test_wrapper_refusals():
    from deep_cartograph_amd import hip

    xyz = torch.from_numpy(reference("chain", 65, 17)[0]).cuda()
    with pytest.raises(_lib.DcvError, match="float32"):
        hip.xtc_encode(xyz.double(), 17)
    with pytest.raises(_lib.DcvError, match=r"expected a \(n, 16, 3\)"):
        hip.xtc_encode(xyz, 16)
    with pytest.raises(_lib.DcvError, match="frame index 65"):
        hip.xtc_encode(xyz, 17, frames=[0, 65])
    with pytest.raises(_lib.DcvError, match="precision"):
        hip.xtc_encode(xyz, 17, precision=0.0)
    with pytest.raises(_lib.DcvError, match="CPU tensor"):
        hip.xtc_encode(xyz.cpu(), 17)
    with pytest.raises(_lib.DcvError, match="slots must be"):
        hip.xtc_encode_slots(xyz, 17, slots=torch.zeros(10, device="cuda"))
    empty, desc, status = hip.xtc_encode(xyz, 17, frames=[], return_status=True)
    assert empty.numel() == 0 and len(desc) == 0 and status.numel() == 0


# ------------------------------------------------------------------------------------------------ the tool
@pytest.fixture(scope="module")
def cluster_case(tmp_path_factory):
    """Two short trajectories cut from the CA_example fixture -- its coordinates on the XTC grid, so that the .xtc and the
    .dcd of the first hold the same numbers --, their topology, and a CSV of two collective variables per trajectory."""
    from deep_cartograph_amd import trajectory as tr

    g = load_golden("compute_features_golden.npz")
    d = tmp_path_factory.mktemp("cluster_case")
    pdb, whole = str(d / "CA_example.pdb"), str(d / "whole.dcd")
    with open(pdb, "w") as f:
        f.write(str(g["pdb"]))
    with open(whole, "wb") as f:
        f.write(g["dcd"].tobytes())
    xyz = tr.open_trajectory(whole).frames()
    q = eo.quantise(xyz)[0]
    grid = xo.to_float(q, 1000.0)
    assert np.array_equal(eo.quantise(grid)[0], q)     # the grid is a fixed point of the quantisation
    cuts = {"run_a": slice(0, 40, 2), "run_b": slice(100, 131, 2)}
    paths = {}
    for name, cut in cuts.items():
        paths[name] = str(d / f"{name}.dcd")
        with tr.write_dcd(paths[name], 104) as w:
            img = w.image(len(grid[cut]))
            off, fs, as_, cs = w.layout()
            for c in range(3):
                img.reshape(-1, fs)[:, off + c * cs:off + c * cs + 104] = grid[cut][:, :, c]
            w.append(img)
        rg = np.sqrt(((grid[cut] - grid[cut].mean(1, keepdims=True)) ** 2).sum(2).mean(1))
        cv = np.round(np.stack([rg, np.linalg.norm(grid[cut][:, 0] - grid[cut][:, -1], axis=1)], axis=1), 4)
        pd.DataFrame(cv, columns=["CV 1", "CV 2"]).to_csv(str(d / f"{name}.csv"), index=False)
    bodies, _, status = eo.encode(grid[cuts["run_a"]])
    os.makedirs(d / "as_xtc")
    xtc_a = str(d / "as_xtc" / "run_a.xtc")
    with open(xtc_a, "wb") as f:
        f.write(eo.file_image(bodies, status, 104))
    return dict(pdb=pdb, dcd=[paths["run_a"], paths["run_b"]], xtc_a=xtc_a, csv=[str(d / "run_a.csv"), str(d / "run_b.csv")],
                grid={"run_a": grid[cuts["run_a"]], "run_b": grid[cuts["run_b"]]})


def test_traj_cluster_extracts_centroids_and_ensembles(cluster_case, tmp_path):
    from deep_cartograph_amd import tools, trajectory as tr

    cfg = {"output_structures": "all", "algorithm": "kmeans", "search_interval": [3, 3], "n_init": 3}
    out = tools.traj_cluster(cfg, cluster_case["csv"], trajectories=cluster_case["dcd"], topologies=[cluster_case["pdb"]],
                             output_folder=str(tmp_path / "from_dcd"), memory_budget=40000)   # several chunks a cluster
    assert out == {name: [str(tmp_path / "from_dcd" / name / "projected_trajectory.csv")] for name in ("run_a", "run_b")}
    top = tr.read_topology(cluster_case["pdb"])
    tables = {name: pd.read_csv(out[name][0]) for name in out}
    centroids = pd.concat([t.assign(traj=name) for name, t in tables.items()])
    centroids = centroids[centroids["centroid"] == True]   # noqa: E712
    assert sorted(centroids["cluster"]) == [0, 1, 2]
    assert sorted(os.listdir(tmp_path / "from_dcd" / "centroids")) == ["cluster_0.pdb", "cluster_1.pdb", "cluster_2.pdb"]
    for _, row in centroids.iterrows():
        got = tr.read_topology(str(tmp_path / "from_dcd" / "centroids" / f"cluster_{int(row['cluster'])}.pdb"))
        assert got.names == top.names and got.resids.tolist() == top.resids.tolist() and got.bonds is None
        want = cluster_case["grid"][row["traj"]][int(row["frame"])]
        assert np.max(np.abs(got.positions.astype(np.float64) - want.astype(np.float64))) <= PDB_BOUND
    for name, table in tables.items():
        files = sorted(f for f in os.listdir(tmp_path / "from_dcd" / name) if f.endswith(".xtc"))
        assert files == [f"cluster_{k}.xtc" for k in sorted(table["cluster"].unique())] and not any(
            f.endswith(".partial") for f in os.listdir(tmp_path / "from_dcd" / name))
        for k in table["cluster"].unique():
            frames = np.sort(table.loc[table["cluster"] == k, "frame"].to_numpy())
            path = str(tmp_path / "from_dcd" / name / f"cluster_{k}.xtc")
            idx = tr.index_xtc(path, 104)
            assert idx.step.tolist() == frames.tolist() and idx.time.tolist() == [float(f) for f in frames]
            back = tools.import_trajectories([path], str(tmp_path / "back" / name / str(k)))
            np.testing.assert_array_equal(tr.open_trajectory(back[0], 104).frames().view(np.uint32),
                                          cluster_case["grid"][name][frames].view(np.uint32))
            ints = xo.decode(open(path, "rb").read())[0]           # and the oracle reads the same integers
            np.testing.assert_array_equal(ints, eo.quantise(cluster_case["grid"][name][frames])[0])
    # an .xtc input gives the same files as its .dcd
    tools.traj_cluster(cfg, cluster_case["csv"], trajectories=[cluster_case["xtc_a"], cluster_case["dcd"][1]], topologies=[cluster_case["pdb"]] * 2,
                       output_folder=str(tmp_path / "from_xtc"))
    assert os.path.exists(tmp_path / "from_xtc" / "xtc_import" / "run_a.dcd")
    for folder in ("centroids", "run_a", "run_b"):
        names = sorted(os.listdir(tmp_path / "from_dcd" / folder))
        assert names == sorted(os.listdir(tmp_path / "from_xtc" / folder))
        for f in names:
            assert open(tmp_path / "from_dcd" / folder / f, "rb").read() == open(tmp_path / "from_xtc" / folder / f, "rb").read(), (folder, f)
    # "centroids" writes the structures only; without the option nothing is extracted
    tools.traj_cluster(dict(cfg, output_structures="centroids"), cluster_case["csv"], trajectories=cluster_case["dcd"], topologies=[cluster_case["pdb"]],
                       output_folder=str(tmp_path / "centroids_only"))
    assert sorted(os.listdir(tmp_path / "centroids_only")) == ["centroids", "configuration.yml", "run_a", "run_b"]
    assert os.listdir(tmp_path / "centroids_only" / "run_a") == ["projected_trajectory.csv"]
    tools.traj_cluster(dict(cfg, output_structures=None), cluster_case["csv"], trajectories=cluster_case["dcd"], topologies=[cluster_case["pdb"]],
                       output_folder=str(tmp_path / "none"))
    assert sorted(os.listdir(tmp_path / "none")) == ["configuration.yml", "run_a", "run_b"]

