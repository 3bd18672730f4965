"""project_trajectory on the reference's 164-frame fixture (tests/golden): the fused launch against the two-step path,
the linear models' projections from coordinates against the reference's own CSVs, the Deep-TICA and AE models against
the reference's outputs, chunking, the tool and the command line."""
import io
import json
import re
import zipfile

import numpy as np
import pandas as pd
import pytest
import torch

from tests import project_trajectory_oracle as po
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

LINEAR = ("pca", "tica", "htica")
TEXT = 5.1e-5   # PLUMED's '%.4f' feature text: the golden projections were computed from features that far from ours (5.0024e-5 measured)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The fixture's files, topology, model feature names and records, and -- computed once -- the float32 features the
    device forms from the coordinates (hip.featurize in label order), which every bound below starts from."""
    from deep_cartograph_amd import hip
    from deep_cartograph_amd import trajectory as tr

    g = load_golden("compute_features_golden.npz")
    d = tmp_path_factory.mktemp("ca_example")
    dcd, pdb = str(d / "CA_example.dcd"), str(d / "CA_example.pdb")
    with open(dcd, "wb") as f:
        f.write(g["dcd"].tobytes())
    with open(pdb, "w") as f:
        f.write(str(g["pdb"]))
    names = [str(s) for s in load_golden("features_164x54.npz")["names"]]
    top = tr.read_topology(pdb)
    traj = tr.open_trajectory(dcd, top.n_atoms)
    rec = tr.definitions_from_labels(names, top)
    defs, n_columns, src, dst = tr.records_to_featurize_defs(rec, len(names))
    flat = torch.from_numpy(np.array(traj.data)).cuda()
    wide = torch.empty(traj.n_frames, n_columns, dtype=torch.float32, device="cuda")
    hip.featurize(flat, defs, top.n_atoms, strides=traj.layout(), out=wide)
    wide[:, torch.from_numpy(dst).cuda()] = wide[:, torch.from_numpy(src).cuda()]
    X = wide[:, :len(names)].contiguous()
    return {"dcd": dcd, "pdb": pdb, "names": names, "top": top, "traj": traj, "rec": rec, "flat": flat, "X": X, "dir": d}


def linear_zip(path, cv, names):
    g = load_golden("linear_models.npz")
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("model/metadata.json", json.dumps({"cv_name": cv, "cv_dimension": 2}))
        z.writestr("model/features_labels.txt", "\n".join(names) + "\n")
        for arr in ("cv_weights", "cv_norm_mean", "cv_norm_range", "features_norm_mean", "features_norm_range"):
            buf = io.BytesIO()
            np.save(buf, g[f"{cv}.{arr}"])
            z.writestr(f"model/{arr}.npy", buf.getvalue())
    return str(path)


def neural_zip(folder, cv, names):
    """The reference's bundled Deep-TICA / AE parameters and buffers as a model.zip in its TorchScript format."""
    from deep_cartograph_amd import export

    g = load_golden("nn_models.npz")
    acts, drops = ["leaky_relu", "leaky_relu", None], [0.0, 0.0, None]
    norm = export.Normalization(g[f"{cv}.buffer.norm_in.mean"], g[f"{cv}.buffer.norm_in.range"])
    post = export.Normalization(g[f"{cv}.buffer.postprocessing.mean"], g[f"{cv}.buffer.postprocessing.range"])
    if cv == "deep_tica":
        lin = [(g[f"deep_tica.param.nn.nn.{i}.weight"], g[f"deep_tica.param.nn.nn.{i}.bias"]) for i in (0, 3, 6)]
        tica = export.TICA(g["deep_tica.buffer.tica.evecs"], g["deep_tica.buffer.tica.mean"])
        module = export.DeepTICA(norm, export.FeedForward(lin, acts, drops), tica, post)
    else:
        enc, dec = ([(g[f"ae.param.{part}.nn.{i}.weight"], g[f"ae.param.{part}.nn.{i}.bias"]) for i in (0, 3, 6)] for part in ("encoder", "decoder"))
        module = export.AutoEncoderCV(norm, export.FeedForward(enc, acts, drops), export.FeedForward(dec, acts, drops), post)
    pt = folder / f"{cv}_weights.pt"
    export.save_torchscript(module, len(names), str(pt))
    zpath = folder / f"{cv}_model.zip"
    with zipfile.ZipFile(zpath, "w") as z:
        z.writestr("model/metadata.json", json.dumps({"cv_name": cv, "cv_dimension": 2}))
        z.writestr("model/features_labels.txt", "\n".join(names) + "\n")
        z.write(pt, "model/cv_weights.pt")
    return str(zpath)


def linear_vectors(cv):
    g = load_golden("linear_models.npz")
    return g[f"{cv}.cv_weights"], dict(fmean=g[f"{cv}.features_norm_mean"], frange=g[f"{cv}.features_norm_range"],
                                       cvmean=g[f"{cv}.cv_norm_mean"], cvrange=g[f"{cv}.cv_norm_range"])


# ------------------------------------------------------------------------------------------------ fused vs two-step
@pytest.mark.parametrize("cv", LINEAR)
def test_fused_launch_against_featurize_then_project(case, cv):
    """Both paths form the same float32 features (one copy of the arithmetic, feat_math.h), so both are held against the
    float64 projection of THOSE features: the fused launch within the oracle's bound, the two-step one within
    dcv_project_linear's (float32 fma chain), their difference within the sum."""
    from deep_cartograph_amd import hip

    W, v = linear_vectors(cv)
    dev = {k: torch.from_numpy(x).cuda() for k, x in v.items()}
    Wd = torch.from_numpy(np.ascontiguousarray(W)).cuda()
    two_step, _ = hip.project_linear(case["X"], Wd, **dev)
    fused, mm = hip.featurize_project(case["flat"], case["rec"], case["top"].n_atoms, len(case["names"]), Wd, strides=case["traj"].layout(),
                                      want_minmax=True, **dev)
    two_step, fused, mm = two_step.cpu().numpy().astype(np.float64), fused.cpu().numpy(), mm.cpu().numpy()
    assert np.array_equal(mm, np.stack([fused.min(0), fused.max(0)]))
    f32 = case["X"].cpu().numpy()
    ref, bound = po.project(f32, np.ascontiguousarray(W), **v)
    bound2 = po.two_step_bound(f32, np.ascontiguousarray(W), **v)
    e1, e2, e12 = np.abs(fused - ref), np.abs(two_step - ref), np.abs(fused - two_step)
    print(f"{cv}: fused error / bound {np.max(e1 / bound):.3f}, two-step error / bound {np.max(e2 / bound2):.3f}, "
          f"difference / (sum of bounds) {np.max(e12 / (bound + bound2)):.3f}")
    assert np.all(e1 <= bound) and np.all(e2 <= bound2) and np.all(e12 <= bound + bound2)
    # and the device's features are the oracle's up to one float32 ulp (what the bound's third term allows)
    from tests import features_oracle as fo
    oracle = po.features(case["traj"].frames(), case["rec"], len(case["names"])).astype(np.float32)
    assert fo.ulp_distance_f32(f32, oracle).max() <= 1


# ------------------------------------------------------------------------------------------------ the pipeline
@pytest.mark.parametrize("path", ["two_step", "fused"])
@pytest.mark.parametrize("cv", LINEAR)
def test_linear_models_project_the_trajectory_to_the_reference_csv(case, cv, path, tmp_path):
    """model.zip + coordinates -> the reference's projected_trajectory.csv within, per column j,
    5.1e-5 sum_i |W_ij| / (frange_i |cvrange_j|) + 5e-5: every feature within PLUMED's '%.4f' text of ours, and the CSV's
    own four decimals.  A memory budget of 50 to 70 frames per chunk gives the same bits as one chunk.  Both paths of the
    linear calculators: the default (featurize, then project_linear) and the fused launch."""
    from deep_cartograph_amd.cv_calculator import CVCalculator

    calc = CVCalculator.load(linear_zip(tmp_path / f"{cv}.zip", cv, case["names"]), str(tmp_path / "load"))
    assert calc.trajectory_path == "two_step"
    calc.trajectory_path = path
    df = calc.project_trajectory(case["dcd"], case["pdb"])
    assert list(df.columns) == calc.cv_labels and df.shape == (164, 2) and df.to_numpy().dtype == np.float32
    W, v = linear_vectors(cv)
    frange, cvrange = np.abs(v["frange"].astype(np.float64)), np.abs(v["cvrange"].astype(np.float64))
    bound = TEXT * (np.abs(W.astype(np.float64)) / frange[:, None]).sum(0) / cvrange + 5e-5
    err = np.abs(df.to_numpy().astype(np.float64) - load_golden("train_colvars_golden.npz")[cv]).max(0)
    print(f"{cv} {path}: worst |projection - reference CSV| per column {err}, bound {bound}, ratio {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    per_frame = 4 * (case["traj"].frame_stride + 100)   # the two-step path's: the record and the 98 + 2 floats of its matrix and result
    chunked = calc.project_trajectory(case["dcd"], case["pdb"], memory_budget=50 * per_frame + 100)
    assert np.array_equal(chunked.to_numpy(), df.to_numpy())
    strided = calc.project_trajectory(case["dcd"], case["pdb"], traj_stride=5, memory_budget=10 * 5 * per_frame)
    assert np.array_equal(strided.to_numpy(), df.to_numpy()[::5])


@pytest.mark.parametrize("cv", ["deep_tica", "ae"])
def test_neural_models_project_the_trajectory_to_the_reference_output(case, cv, tmp_path):
    """The reference's Deep-TICA / AE model on features computed from the coordinates against its own output on the
    '%.4f' features: the 2e-5 of the infer golden test (tests/test_mlp_gpu.py) plus the feature-text term pushed through
    the network with absolute weights (leaky_relu is 1-Lipschitz): 5.1e-5 / |range| through |W0|, |W1|, |W2|, then |evecs|
    (Deep-TICA) and 1 / |postprocessing range|."""
    from deep_cartograph_amd.cv_calculator import CVCalculator

    g = load_golden("nn_models.npz")
    prefix = "deep_tica.param.nn.nn" if cv == "deep_tica" else "ae.param.encoder.nn"
    delta = TEXT / np.abs(g[f"{cv}.buffer.norm_in.range"].astype(np.float64))
    for i in (0, 3, 6):
        delta = np.abs(g[f"{prefix}.{i}.weight"].astype(np.float64)) @ delta
    if cv == "deep_tica":
        delta = delta @ np.abs(g["deep_tica.buffer.tica.evecs"].astype(np.float64))
    tol = 2e-5 + delta / np.abs(g[f"{cv}.buffer.postprocessing.range"].astype(np.float64))
    calc = CVCalculator.load(neural_zip(tmp_path, cv, case["names"]), str(tmp_path / "load"))
    df = calc.project_trajectory(case["dcd"], case["pdb"])
    assert list(df.columns) == calc.cv_labels and df.shape == (164, 2)
    err = np.abs(df.to_numpy().astype(np.float64) - g[f"{cv}.output"]).max(0)
    print(f"{cv}: worst |projection - reference output| per column {err}, tolerance {tol}, ratio {np.max(err / tol):.3f}")
    assert np.all(err <= tol)
    # the same launches on the device's feature matrix, through project_data: the same bits
    assert np.array_equal(calc.project_data(case["X"]).numpy(), df.to_numpy())
    per_frame = 4 * (case["traj"].frame_stride + 200)
    chunked = calc.project_trajectory(case["dcd"], case["pdb"], memory_budget=50 * per_frame)   # chunks of 50 to 60 frames
    assert chunked.shape == (164, 2) and np.all(np.abs(chunked.to_numpy().astype(np.float64) - g[f"{cv}.output"]).max(0) <= tol)


def test_non_finite_coordinates_are_reported(case, tmp_path):
    from deep_cartograph_amd.cv_calculator import CVCalculator

    xyz = case["traj"].frames(0, 40)
    xyz[17, 29, 1] = np.nan      # atom 29 is @CA_533, which the model's features name
    np.save(tmp_path / "bad.npy", xyz)
    for zpath, path in ((linear_zip(tmp_path / "pca.zip", "pca", case["names"]), "two_step"), (str(tmp_path / "pca.zip"), "fused"),
                        (neural_zip(tmp_path, "ae", case["names"]), None)):
        calc = CVCalculator.load(zpath, str(tmp_path / "load"))
        if path:
            calc.trajectory_path = path
        with pytest.raises(ValueError, match=r"NaNs in the features of frames \d+\.\.\d+ of .*bad\.npy") as e:
            calc.project_trajectory(str(tmp_path / "bad.npy"), case["pdb"], memory_budget=25000)   # several chunks for either model
        lo, hi = (int(x) for x in re.search(r"frames (\d+)\.\.(\d+) of", str(e.value)).groups())
        assert lo <= 17 <= hi and hi - lo < 39


# ------------------------------------------------------------------------------------------------ tool and command line
def test_tool_writes_skips_and_the_command_line_gives_the_same_bytes(case, tmp_path):
    from deep_cartograph_amd import project, tools
    from deep_cartograph_amd.cv_calculator import CVCalculator

    models = [linear_zip(tmp_path / f"{cv}.zip", cv, case["names"]) for cv in ("pca", "tica")]
    out = tools.traj_projection({}, None, topologies=[case["pdb"]], model_paths=models, output_folder=str(tmp_path / "tool"),
                                trajectories=[case["dcd"]])
    assert out == {cv: [str(tmp_path / "tool" / cv / "CA_example" / "projected_trajectory.csv")] for cv in ("pca", "tica")}
    calc = CVCalculator.load(models[0], str(tmp_path / "load"))
    csv = pd.read_csv(out["pca"][0])
    assert list(csv.columns) == calc.cv_labels
    assert np.abs(csv.to_numpy() - calc.project_trajectory(case["dcd"], case["pdb"]).to_numpy().astype(np.float64)).max() <= 5e-5 + 1e-7
    # a second call keeps what is there
    with open(out["pca"][0], "w") as f:
        f.write("kept\n")
    again = tools.traj_projection({}, [], topologies=[case["pdb"]], model_paths=models, output_folder=str(tmp_path / "tool"),
                                  trajectories=[case["dcd"]], trajectory_names=["CA_example"])
    assert again == out and open(out["pca"][0]).read() == "kept\n"
    # one topology per trajectory, names given
    named = tools.traj_projection({}, None, topologies=[case["pdb"], case["pdb"]], model_paths=models[1:], trajectory_names=["a", "b"],
                                  output_folder=str(tmp_path / "named"), trajectories=[case["dcd"], case["dcd"]])
    assert [p.split("/")[-2] for p in named["tica"]] == ["a", "b"]
    assert open(named["tica"][0], "rb").read() == open(named["tica"][1], "rb").read() == open(out["tica"][0], "rb").read()
    # the command line
    project.main(["-traj", case["dcd"], "-top", case["pdb"], "-model", *models, "-out", str(tmp_path / "cli")])
    cli = {cv: open(tmp_path / "cli" / cv / "CA_example" / "projected_trajectory.csv", "rb").read() for cv in ("pca", "tica")}
    assert cli["tica"] == open(out["tica"][0], "rb").read()
    assert cli["pca"] == calc.project_trajectory(case["dcd"], case["pdb"]).to_csv(index=False, float_format="%.4f").encode()
