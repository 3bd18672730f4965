"""analyze_geometry without a device: the float64 oracle against scipy, the configuration schema, the refusal to run on
the CPU, and the tool's loop, keys and CSV files from a stubbed computation."""
import os
import re

import numpy as np
import pytest
import torch

from tests import geometry_oracle as go
from tests.conftest import ROOT, load_golden


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


def test_oracle_agrees_with_scipy():
    """SVD-Kabsch with the determinant correction against scipy's Rotation.align_vectors (also an SVD, written
    independently): rotation entries and the RMSD, on general, weighted and mirrored frames.  Both are float64 on the
    same input; 1e-9 is the tolerance the device tests grant the kernel, the oracle must sit far inside it."""
    from scipy.spatial.transform import Rotation

    worst_r = worst_d = 0.0
    for n_fit in (3, 4, 5, 64, 257):
        xyz, ref = go.synthetic(14, n_fit, 100 + n_fit)
        xyz[::7, :, 0] *= -1            # mirror images: the best PROPER rotation is wanted
        w = np.random.Generator(np.random.PCG64(n_fit)).uniform(0.1, 3.0, n_fit)
        for weights in (None, w):
            for f in range(len(xyz)):
                R, c_mob, c_ref = go.kabsch(xyz[f], ref, weights)
                wv = np.ones(n_fit) if weights is None else weights
                rot, rssd = Rotation.align_vectors(ref - c_ref, xyz[f].astype(np.float64) - c_mob, weights=wv)
                assert abs(np.linalg.det(R) - 1.0) < 1e-12
                worst_r = max(worst_r, np.abs(rot.as_matrix().T - R).max())
                res = (xyz[f] - c_mob) @ R - (ref - c_ref)
                mine = np.sqrt((wv * (res ** 2).sum(1)).sum())
                worst_d = max(worst_d, abs(mine - rssd))
    print(f"oracle vs scipy: rotation {worst_r:.2e}, weighted root sum of squares {worst_d:.2e}")
    assert worst_r < 1e-9 and worst_d < 1e-9


def test_oracle_superpose_is_consistent():
    xyz, ref = go.synthetic(5, 12, 3)
    fit, sel = np.arange(0, 12, 2), np.arange(3, 9)
    out = go.superpose(xyz, fit, ref[fit], sel, ref[sel])
    R = out["transform"][:, :9].reshape(-1, 3, 3)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14
    d = out["aligned"] - ref[sel]
    assert np.allclose(out["moments"][:, :, 0], d.sum(0), atol=1e-12) and np.allclose(out["moments"][:, :, 1], (d ** 2).sum(0), atol=1e-10)
    assert np.allclose(out["rmsd"][:, 1], np.sqrt((d ** 2).sum((1, 2)) / len(sel)), atol=1e-13)
    # 1 Angstrom of noise per coordinate: the RMSD is near sqrt(3), and a frame that IS the reference gives 0
    assert 0.8 < out["rmsd"][:, 0].mean() < 2.5
    assert go.superpose(ref[None].astype(np.float32), fit, ref[fit].astype(np.float32))["rmsd"][0, 0] < 1e-12


def test_schema_defaults():
    from deep_cartograph_amd.schemas import AnalyzeGeometrySchema

    assert AnalyzeGeometrySchema().model_dump() == {"analysis": {"RMSD": {}, "RMSF": {}, "dRMSD": {}}, "dt_per_frame": 1.0, "run": True}
    cfg = AnalyzeGeometrySchema(analysis={"RMSD": {"a": {}}, "RMSF": {"b": {"selection": "resid 3:9 and name CA"}}, "dRMSD": {"c": {}}}).model_dump()
    assert cfg["analysis"]["RMSD"]["a"] == {"title": "Protein Backbone RMSD", "selection": "name CA", "fit_selection": "name CA"}
    assert cfg["analysis"]["RMSF"]["b"] == {"title": "Protein Backbone RMSF", "selection": "resid 3:9 and name CA", "fit_selection": "name CA"}
    assert cfg["analysis"]["dRMSD"]["c"] == {"title": "Protein Backbone dRMSD", "selection": "name CA", "selection_stride": 5}


def test_header_and_binding_agree_on_the_group_cap():
    from deep_cartograph_amd import _lib

    text = open(os.path.join(ROOT, "include", "dcv.h")).read()
    assert int(re.search(r"#define DCV_SUPERPOSE_MAX_GROUPS (\d+)", text).group(1)) == _lib.SUPERPOSE_MAX_GROUPS
    assert "dcv_superpose" in _lib.SIGNATURES and "dcv_superpose_workspace" in _lib.SIGNATURES


def test_no_cpu_fallback(fixture_files, tmp_path, monkeypatch):
    from deep_cartograph_amd import geometry, hip, tools
    from deep_cartograph_amd._lib import DcvError

    dcd, pdb = fixture_files
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = {"analysis": {"RMSD": {"ca": {}}}}
    with pytest.raises(DcvError, match="no CPU fallback"):
        tools.analyze_geometry(cfg, [dcd], [pdb], output_folder=str(tmp_path / "out"))
    assert not [f for f in os.listdir(tmp_path / "out") if f.endswith(".csv")]
    for call in (lambda: geometry.rmsd(dcd, pdb, "name CA", "name CA"), lambda: geometry.rmsf(dcd, pdb, "name CA", "name CA"),
                 lambda: geometry.average_structure(dcd, pdb, "name CA"), lambda: geometry.drmsd(dcd, pdb, "name CA", 5, pdb)):
        with pytest.raises(DcvError, match="no CPU fallback"):
            call()
    with pytest.raises(DcvError, match="cuda"):
        hip.superpose(torch.zeros(2, 4, 3), 4, [0, 1, 2], np.zeros((3, 3)))
    # with nothing to compute, or run: false, the tool needs no device and writes no series
    assert tools.analyze_geometry({}, [dcd], [pdb], output_folder=str(tmp_path / "empty")) == {}
    assert tools.analyze_geometry({**cfg, "run": False}, [dcd], [pdb], output_folder=str(tmp_path / "off")) == {}


def test_selections_must_match_between_topologies(fixture_files, tmp_path):
    from deep_cartograph_amd import geometry

    dcd, pdb = fixture_files
    with open(pdb) as f:
        lines = [l for l in f if l.startswith("ATOM")]
    short = str(tmp_path / "short.pdb")
    with open(short, "w") as f:
        f.writelines(lines[:-5])
    with pytest.raises(ValueError, match="do not match"):
        geometry.rmsd(dcd, pdb, "name CA", "name CA", ref_top=short)
    with pytest.raises(ValueError, match="empty"):
        geometry.rmsd(dcd, pdb, "name XX", "name CA")
    with pytest.raises(ValueError, match="protein"):
        geometry.rmsd(dcd, pdb, "protein and name CA", "name CA")


def test_tool_keys_files_and_headers_from_a_stubbed_computation(fixture_files, tmp_path, monkeypatch):
    """The reference's loop: RMSD per trajectory and reference, RMSF per trajectory over residue numbers, dRMSD per
    trajectory and reference (the topology when none is given); x = arange(n) * dt_per_frame * 1e-3; save_data's CSV."""
    from deep_cartograph_amd import geometry, tools

    dcd, pdb = fixture_files
    ref = str(tmp_path / "state_B.pdb")
    with open(pdb) as src, open(ref, "w") as dst:
        dst.write(src.read())
    calls = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(geometry, "rmsd", lambda traj, top, sel, fit, ref_top=None, budget=None: calls.append(("rmsd", sel, fit, ref_top)) or np.array([0.5, 1.5, 2.5]))
    monkeypatch.setattr(geometry, "rmsf", lambda traj, top, sel, fit, budget=None: calls.append(("rmsf", sel, fit)) or (np.array([0.25, 0.75]), np.array([7, 9])))
    monkeypatch.setattr(geometry, "drmsd", lambda traj, top, sel, stride, ref_top, budget=None: calls.append(("drmsd", sel, stride, ref_top)) or np.array([0.125, 0.375]))
    cfg = {"dt_per_frame": 20.0, "analysis": {"RMSD": {"all_ca": {}, "loop": {"selection": "resid 10:20 and name CA"}}, "RMSF": {"ca": {}},
                                              "dRMSD": {"contacts": {"selection_stride": 3}}}}
    out = tools.analyze_geometry(cfg, [dcd], [pdb], output_folder=str(tmp_path / "first"))
    assert sorted(out) == ["all_ca_RMSD_CA_examplefirst_frame", "ca_RMSF_CA_example", "contacts_dRMSD_CA_example_to_CA_example",
                           "loop_RMSD_CA_examplefirst_frame"]
    assert all(path == str(tmp_path / "first" / (stem + ".csv")) and os.path.exists(path) for stem, path in out.items())
    assert ("rmsd", "resid 10:20 and name CA", "name CA", None) in calls and ("drmsd", "name CA", 3, pdb) in calls
    text = open(out["all_ca_RMSD_CA_examplefirst_frame"]).read().split("\n")
    assert text[0] == "Time (ns),RMSD (A)" and len(text) == 5 and text[4] == ""
    got = np.loadtxt(out["all_ca_RMSD_CA_examplefirst_frame"], delimiter=",", skiprows=1)
    assert np.array_equal(got, np.column_stack((np.arange(3) * 20.0 * 1e-3, [0.5, 1.5, 2.5])))
    assert open(out["ca_RMSF_CA_example"]).readline() == "Residue,RMSF (A)\n"
    assert np.array_equal(np.loadtxt(out["ca_RMSF_CA_example"], delimiter=",", skiprows=1), [[7, 0.25], [9, 0.75]])
    assert open(out["contacts_dRMSD_CA_example_to_CA_example"]).readline() == "Time (ns),dRMSD (A)\n"
    assert os.path.exists(tmp_path / "first" / "configuration.yml")
    # with reference topologies: one RMSD and one dRMSD series per reference
    out = tools.analyze_geometry(cfg, [dcd], [pdb], ref_topologies=[ref], output_folder=str(tmp_path / "second"))
    assert sorted(out) == ["all_ca_RMSD_CA_example_to_state_B", "ca_RMSF_CA_example", "contacts_dRMSD_CA_example_to_state_B",
                           "loop_RMSD_CA_example_to_state_B"]
    assert ("rmsd", "name CA", "name CA", ref) in calls and ("drmsd", "name CA", 3, ref) in calls
    with pytest.raises(ValueError, match="do not match"):
        tools.analyze_geometry(cfg, [dcd, dcd], [pdb, pdb, pdb], output_folder=str(tmp_path / "third"))
    with pytest.raises(FileNotFoundError):
        tools.analyze_geometry(cfg, [dcd], [str(tmp_path / "none.pdb")], output_folder=str(tmp_path / "fourth"))
