"""The XTC writer without a device: the oracle encoder (tests/xtc_encode_oracle.py: quantisation, policy) against the
oracle decoder, the losslessness of re-encoding a decoded file, the size of the policy's streams against the reference
writer's, the exported symbols, the file writer, the frame extraction's host side and the tool's warnings."""
import logging
import os
import struct

import numpy as np
import pandas as pd
import pytest
import torch

from tests import xtc_encode_oracle as eo
from tests import xtc_oracle as xo
from tests.conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("protein", "aladip")


@pytest.fixture(scope="module")
def golden():
    g = load_golden("xtc_golden.npz")
    return {"aladip": g["aladip_xtc"].tobytes(), "protein": g["protein_xtc"].tobytes()}


@pytest.fixture(scope="module")
def decoded(golden):
    """(file integers, decoded Angstrom, frame headers) of both fixtures, computed once."""
    return {name: (*xo.decode(golden[name])[:2], xo.frames(golden[name])) for name in FIXTURES}


@pytest.fixture(scope="module")
def ca_example(tmp_path_factory):
    g = load_golden("compute_features_golden.npz")
    d = tmp_path_factory.mktemp("ca_example")
    dcd, pdb = str(d / "CA_example.dcd"), str(d / "CA_example.pdb")
    with open(dcd, "wb") as f:
        f.write(g["dcd"].tobytes())
    with open(pdb, "w") as f:
        f.write(str(g["pdb"]))
    return dcd, pdb


def roundtrip(x, precision):
    """decode(encode(x)) == quantise(x) for one frame; returns the descriptor fields."""
    body, d, status = eo.encode_frame(x, precision)
    assert status == eo.OK
    q, _ = eo.quantise(x, precision)
    ints, _, st = xo.decode(xo.header(len(x)) + body)
    assert st[0] == xo.OK and np.array_equal(ints[0], q)
    assert d["nbytes"] <= eo.slot_bytes(len(x))
    return d


@pytest.mark.parametrize("natoms", [10, 11, 37, 104])
@pytest.mark.parametrize("name", ["chain", "water", "scattered", "tight", "identical", "negative", "run_at_end", "precision100"])
def test_decode_of_encode_is_the_quantised_input(name, natoms):
    for x in eo.synthetic(name, 4, natoms):
        roundtrip(x, eo.case_precision(name))


def test_wide_frames_take_the_two_full_range_forms():
    for x in eo.synthetic("bigsize", 4, 12):    # extents over 0xffffff: three bit fields instead of one product
        d = roundtrip(x, 1.0e5)
        assert max(d["maxint"][k] - d["minint"][k] + 1 for k in range(3)) > 0xffffff
    for x in eo.synthetic("bits72", 4, 12):     # sizeint just below 2^24 in every component: a 72-bit pack3
        d = roundtrip(x, 1000.0)
        size = [d["maxint"][k] - d["minint"][k] + 1 for k in range(3)]
        assert max(size) <= 0xffffff and (size[0] * size[1] * size[2]).bit_length() == 72


def test_the_cases_reach_every_branch_of_the_policy():
    scripts = {name: [eo.policy(eo.quantise(x, eo.case_precision(name))[0])[0] for x in eo.synthetic(name, 8, 37)] for name in eo.CASES}
    groups = lambda name: [g for s in scripts[name] for g in s]
    assert any(r == 1 for r, _, _ in groups("water"))                                  # swap runs of 2
    assert any(step == 1 for _, step, _ in groups("scattered")) and any(step == -1 for _, step, _ in groups("scattered"))
    assert any(r == 8 for r, _, _ in groups("tight")) and any(reuse for _, _, reuse in groups("identical"))
    assert sum(s[-1][0] > 0 for s in scripts["run_at_end"]) >= 4                      # the last group is a run that ends the frame


def test_ca_example_frames_round_trip(ca_example):
    from deep_cartograph_amd import trajectory as tr

    xyz = tr.open_trajectory(ca_example[0]).frames()
    for x in xyz[::7]:
        roundtrip(x, 1000.0)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_requantises_to_its_own_integers_and_round_trips(name, decoded):
    ints, xyz, frames = decoded[name]
    total = own = 0
    for f, fr in enumerate(frames):
        q, status = eo.quantise(xyz[f], fr["precision"])
        assert status == eo.OK and np.array_equal(q, ints[f])          # a trajectory that came from an .xtc is re-encoded losslessly
        d = roundtrip(xyz[f], fr["precision"])
        assert d["smallidx"] == fr["smallidx"] and d["minint"] == tuple(fr["minint"]) and d["maxint"] == tuple(fr["maxint"])
        total, own = total + d["nbytes"], own + fr["nbytes"]
    # a condition, not a measurement: the policy's payload does not exceed the reference writer's (0.9919 and 0.9990 of it)
    assert total <= own, (total, own)


def test_marked_frames_and_raw_frames():
    x = eo.synthetic("chain", 3, 12)
    x[0, 4, 1], x[1, 2, 0], x[2, 7, 2] = np.nan, 3.0e9, np.inf
    bodies, desc, status = eo.encode(x, 1000.0)
    assert status.tolist() == [eo.NONFINITE, eo.RANGE, eo.NONFINITE] and bodies == [b"", b"", b""] and not desc["nbytes"].any()
    edge = np.float32(2147483520.0)                  # lf on the limit itself (scale and precision 1): refused; one float below: encoded
    assert eo.quantise([edge], 1.0, 1.0)[1] == eo.RANGE and eo.quantise([-edge], 1.0, 1.0)[1] == eo.RANGE
    q, status = eo.quantise([np.nextafter(edge, np.float32(0)), -np.nextafter(edge, np.float32(0))], 1.0, 1.0)
    assert status == eo.OK and q.tolist() == [2147483392, -2147483392]
    assert eo.quantise(np.float32([0.5, -0.5, 1.4999, 2.5, -2.5]), 1.0, 1.0)[0].tolist() == [1, -1, 1, 3, -3]   # half away from zero
    raw = eo.synthetic("chain", 2, 9)
    bodies, desc, status = eo.encode(raw, 1000.0)
    assert not status.any() and desc["raw"].tolist() == [1, 1] and len(bodies[0]) == 108
    _, back, _ = xo.decode(eo.file_image(bodies, status, 9))
    assert np.array_equal(back, eo.scaled(raw) * np.float32(10.0))


def test_library_exports_the_encoder():
    import __graft_entry__ as ge
    from deep_cartograph_amd import _lib

    ge.build()
    lib = _lib.load()
    for s in ("dcv_xtc_encode", "dcv_xtc_encode_workspace", "dcv_xtc_encode_slot_bytes", "dcv_xtc_pack", "dcv_xtc_pack_workspace"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert lib.dcv_abi_version() == 5
    for natoms in (1, 9, 10, 11, 104, 457):
        assert lib.dcv_xtc_encode_slot_bytes(natoms) == eo.slot_bytes(natoms)
    assert lib.dcv_xtc_encode_slot_bytes(0) == 0 and lib.dcv_xtc_encode_workspace(-1) == 0 and lib.dcv_xtc_pack_workspace(-1) == 0
    assert lib.dcv_xtc_encode_workspace(65) == 768 and lib.dcv_xtc_pack_workspace(3) == 512
    assert eo.FRAME_DTYPE == _lib.XTC_FRAME_DTYPE


def test_xtc_writer_partial_file_rename_and_bytes(tmp_path):
    from deep_cartograph_amd import trajectory as tr

    x = eo.synthetic("water", 5, 23)
    bodies, _, status = eo.encode(x, 1000.0)
    image = eo.file_image(bodies, status, 23)
    path = str(tmp_path / "out" / "cluster_0.xtc")
    os.makedirs(tmp_path / "out")
    first = len(eo.file_image(bodies[:2], status[:2], 23))
    with tr.write_xtc(path, 23) as w:
        w.append(image[:first])
        assert os.listdir(tmp_path / "out") == ["cluster_0.xtc.partial"]
        w.append(np.frombuffer(image[first:], dtype=np.uint8))
        with pytest.raises(ValueError, match="23"):
            w.append(eo.file_image(*eo.encode(eo.synthetic("water", 1, 11))[::2], 11))
        with pytest.raises(ValueError, match="whole number"):
            w.append(image[:57])
    assert os.listdir(tmp_path / "out") == ["cluster_0.xtc"]
    assert open(path, "rb").read() == image
    idx = tr.index_xtc(path, 23)
    assert idx.n_frames == 5 and idx.step.tolist() == [0, 1, 2, 3, 4] and idx.time.tolist() == [0, 1, 2, 3, 4] and not idx.box.any()
    ints, _, st = xo.decode(image)
    assert not st.any() and np.array_equal(ints, eo.quantise(x)[0])
    with pytest.raises(RuntimeError):                       # an interrupted run leaves neither name behind
        with tr.write_xtc(str(tmp_path / "out" / "broken.xtc"), 23) as w:
            w.append(image[:first])
            raise RuntimeError("interrupted")
    assert os.listdir(tmp_path / "out") == ["cluster_0.xtc"]


def test_extraction_chunks_and_refusals(ca_example, tmp_path, caplog):
    from deep_cartograph_amd import trajectory as tr
    from deep_cartograph_amd._lib import DcvError

    dcd, pdb = ca_example
    n = tr.open_trajectory(dcd).n_frames
    # chunks: ascending ranges that cover every frame once; the span from the first to the last source frame counts
    frames = np.array([0, 1, 2, 10, 11, 40])
    assert tr.extraction_chunks(frames, 100, 10, 10 ** 9) == [(0, 6)]
    assert tr.extraction_chunks(frames, 100, 10, 1) == [(i, i + 1) for i in range(6)]
    assert tr.extraction_chunks(frames, 100, 10, 330) == [(0, 3), (3, 5), (5, 6)]
    with pytest.raises(ValueError, match=rf"CA_example\.dcd: frame {n} "):
        tr.extract_frames(dcd, pdb, [3, n, 1], str(tmp_path / "a.xtc"))
    with pytest.raises(ValueError, match=r"CA_example\.dcd: frame -1 "):
        tr.extract_frames(dcd, pdb, [3, -1], str(tmp_path / "a.xtc"))
    with caplog.at_level(logging.WARNING):
        assert tr.extract_frames(dcd, pdb, [], str(tmp_path / "a.xtc")) is None
    assert "No frames to extract" in caplog.text
    assert os.listdir(tmp_path) == []
    if not torch.cuda.is_available():                        # a tool-level call without a GPU raises as the other tools do
        with pytest.raises(DcvError, match="no CPU fallback"):
            tr.extract_frames(dcd, pdb, [2, 0], str(tmp_path / "a.xtc"))
        assert os.listdir(tmp_path) == []


def test_extract_frames_sorts_before_it_encodes(ca_example, tmp_path, monkeypatch):
    """The device call replaced by a recorder: the frames arrive ascending, relative to the first frame of their chunk, with
    the source indices as steps and times, and the image is appended as it comes back."""
    from deep_cartograph_amd import hip
    from deep_cartograph_amd import trajectory as tr

    dcd, pdb = ca_example
    A = tr.open_trajectory(dcd).n_atoms
    calls = []

    class FakeTensor:
        def __init__(self, a):
            self.a = a

        def cuda(self):
            return self

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    def fake_encode(buf, n_atoms, strides=None, frames=None, precision=1000.0, step=None, time=None, **kw):
        calls.append((n_atoms, tuple(strides), frames.tolist(), step.tolist(), time.tolist()))
        return FakeTensor(np.frombuffer(xo.header(n_atoms, 0, 0.0, np.zeros(9)), dtype=np.uint8))

    monkeypatch.setattr(hip, "xtc_encode", fake_encode)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch, "from_numpy", lambda a: FakeTensor(a))
    out = tr.extract_frames(dcd, pdb, [9, 2, 5, 2], str(tmp_path / "c.xtc"), memory_budget=10 ** 9)
    assert out == str(tmp_path / "c.xtc") and os.path.getsize(out) == 56
    (n_atoms, strides, frames, step, time), = calls
    assert n_atoms == A and frames == [0, 0, 3, 7] and step == [2, 2, 5, 9] and time == [2.0, 2.0, 5.0, 9.0] and strides[0] == 8


def test_traj_cluster_without_topologies_warns_and_returns_the_csv_paths(tmp_path, monkeypatch, caplog):
    from deep_cartograph_amd import statistics, tools

    rng = np.random.default_rng(0)
    pts = np.round(np.concatenate([rng.normal(c, 0.05, size=(10, 2)) for c in ((0, 0), (1, 1))]), 4)
    csv = str(tmp_path / "cv.csv")
    pd.DataFrame(pts, columns=["PC 1", "PC 2"]).to_csv(csv, index=False)
    labels = np.repeat([0, 1], 10)

    def fake_find_centroids(data, centroids, features):
        data["centroid"] = False
        data.loc[[3, 14], "centroid"] = True
        return data

    monkeypatch.setattr(statistics, "optimize_clustering", lambda X, cfg: (labels, np.array([[0.0, 0.0], [1.0, 1.0]])))
    monkeypatch.setattr(statistics, "find_centroids", fake_find_centroids)
    with caplog.at_level(logging.WARNING):
        out = tools.traj_cluster({"output_structures": "all"}, csv, trajectories=["run_a.dcd"], output_folder=str(tmp_path / "tc"), frames_per_sample=5)
    assert out == {"run_a": [str(tmp_path / "tc" / "run_a" / "projected_trajectory.csv")]}
    assert "Skipping extraction of centroids" in caplog.text and "Skipping extraction of cluster ensembles" in caplog.text
    assert sorted(os.listdir(tmp_path / "tc")) == ["configuration.yml", "run_a"] and os.listdir(tmp_path / "tc" / "run_a") == ["projected_trajectory.csv"]
    df = pd.read_csv(out["run_a"][0])
    assert df["frame"].tolist() == list(range(0, 100, 5)) and df["cluster"].tolist() == labels.tolist()
    with pytest.raises(ValueError, match="2 trajectories and 2 topologies for 1 CV"):
        tools.traj_cluster({}, csv, trajectories=["a.dcd", "b.dcd"], topologies=["a.pdb"], output_folder=str(tmp_path / "bad"))
