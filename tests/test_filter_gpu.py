"""filter_features on the MI355X: histogram counts equal to NumPy's, entropy / std against the reference expressions,
the dip kernel against the float64 restatement (tests/filter_oracle.py), p-values against a NumPy null within the
Monte-Carlo bound, the whole tool on the reference's fixture, a 2M x 256 run and the deep_carto pre-step."""
import json
import os
import zipfile

import numpy as np
import pandas as pd
import pytest
import torch

from tests import filter_oracle as fo
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

BINS = 100


@pytest.fixture(scope="module")
def golden():
    g = load_golden("filter_golden.npz")
    return {"X": np.ascontiguousarray(g["X"]), "names": [str(s) for s in g["names"]],
            "filtered": [str(s) for s in g["filtered"]], "summary_names": [str(s) for s in g["summary_names"]],
            "summary_pass": g["summary_pass"], "summary_hdtp": g["summary_hdtp"]}


def reference_test_configuration():
    """The configuration of the reference's own filter_features test (unknown fields are dropped by the schema)."""
    return {"filter_settings": {"compute_diptest": True, "compute_entropy": False, "compute_std": False,
                                "diptest_significance_level": 0.05, "entropy_quantile": 0, "std_quantile": 0},
            "sampling_settings": {"relaxation_time": 1}}


def device_counts(Xd):
    """counts [F, 100] of the device histogram over NumPy's own edges, and the edges."""
    from deep_cartograph_amd import features, hip

    raw = hip.col_stats_raw(Xd).cpu().numpy()
    edges = features.histogram_edges(raw[2], raw[3], BINS)
    counts = hip.col_histogram(Xd, torch.from_numpy(edges).cuda())
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (Xd.shape[1], BINS)
    return counts.cpu().numpy(), edges


def assert_counts_equal_numpy(X, Xd=None):
    Xd = torch.from_numpy(X).cuda() if Xd is None else Xd
    counts, edges = device_counts(Xd)
    for c in range(X.shape[1]):
        ref, ref_edges = np.histogram(X[:, c], bins=BINS)
        assert np.array_equal(edges[c], ref_edges), f"column {c}: edges differ"
        assert np.array_equal(counts[c], ref), f"column {c}: {np.flatnonzero(counts[c] != ref)[:5]}"
    return counts, edges


# ------------------------------------------------------------------------------------------------ 1. histogram
def test_histogram_golden_matrix(golden):
    assert_counts_equal_numpy(golden["X"])


@pytest.mark.parametrize("F", [1, 3, 54, 512, 515])
def test_histogram_synthetic(F):
    rng = np.random.Generator(np.random.PCG64(F))
    n = 200000
    X = rng.standard_normal((n, F)).astype(np.float32)
    X = X * rng.uniform(1e-3, 1e3, F).astype(np.float32) + rng.uniform(-100, 100, F).astype(np.float32)
    assert_counts_equal_numpy(X)


@pytest.mark.parametrize("F,ld,offset", [(54, 64, 0), (512, 520, 0), (12, 16, 1), (512, 516, 3), (5, 9, 2)])
def test_histogram_leading_dimension_and_unaligned_base(F, ld, offset):
    rng = np.random.Generator(np.random.PCG64(7 * F + ld))
    n = 200000
    big = (rng.standard_normal((n, ld), dtype=np.float32) * np.float32(3) + np.float32(1))
    buf = torch.from_numpy(big).cuda()
    Xd = buf[:, offset:offset + F]           # row stride ld > F; an offset that is not a multiple of 4 breaks the 16-byte alignment
    assert Xd.stride(0) == ld and (offset == 0 or Xd.data_ptr() % 16 != 0)
    assert_counts_equal_numpy(np.ascontiguousarray(big[:, offset:offset + F]), Xd)


def test_histogram_constant_edge_and_two_valued_columns():
    n = 5000
    rng = np.random.Generator(np.random.PCG64(11))
    X = np.empty((n, 8), dtype=np.float32)
    X[:, 0] = 2.5                                         # constant: range expanded by +-0.5
    X[:, 1] = -7.0
    edges = np.histogram_bin_edges(np.array([-3.0, 11.0], dtype=np.float32), bins=BINS)
    X[:, 2] = edges[rng.integers(0, BINS + 1, n)]        # every value sits exactly on an edge
    X[:2, 2] = edges[[0, BINS]]
    X[:, 3] = np.where(rng.random(n) < 0.3, 1.0, 4.0)    # two values
    X[:, 4] = np.where(rng.random(n) < 0.5, -1e-3, 1e-3)
    X[:, 5] = np.nextafter(edges[rng.integers(1, BINS, n)], np.float32(-np.inf))   # one ulp below the edges
    X[:2, 5] = edges[[0, BINS]]
    X[:, 6] = rng.integers(0, 101, n).astype(np.float32) / np.float32(100.0)
    X[:, 7] = 0.0
    assert_counts_equal_numpy(X)
    counts, _ = device_counts(torch.from_numpy(np.ascontiguousarray(X[:, :4])).cuda())
    assert counts[0].sum() == n and counts[0].max() == n


# ------------------------------------------------------------------------------------------------ 2. entropy, std
def test_entropy_is_the_reference_expression(golden):
    from scipy.stats import entropy

    from deep_cartograph_amd import features

    rng = np.random.Generator(np.random.PCG64(5))
    big = rng.standard_normal((30000, 20)).astype(np.float32) * rng.uniform(0.1, 10, 20).astype(np.float32)
    big[:, 3] = 1.0
    big[:, 4] = np.round(big[:, 4])
    for X in (golden["X"], big):
        got = features.shannon_entropy((X, [f"f{i}" for i in range(X.shape[1])]))
        assert isinstance(got, list) and len(got) == X.shape[1]
        for c in range(X.shape[1]):
            hist, bin_edges = np.histogram(X[:, c], bins=100, density=True)
            expected = round(entropy(hist * np.diff(bin_edges), base=2), 3)
            assert got[c] == expected, (c, got[c], expected)
    df = pd.DataFrame(golden["X"][:, :5], columns=golden["names"][:5])
    assert features.shannon_entropy(df) == features.shannon_entropy((golden["X"][:, :5], golden["names"][:5]))


def test_std_against_float64_two_pass():
    """Within 1e-9 relative of the float64 two-pass value for |mean| / std up to 1e3: the bound is the float64
    cancellation in sumsq/n - mean^2, about 2e-16 * (mean / std)^2 = 2e-10."""
    from deep_cartograph_amd import features, hip

    rng = np.random.Generator(np.random.PCG64(9))
    n = 200000
    ratios = np.array([0.0, 1.0, 30.0, 300.0, 990.0, -990.0, 3.0, 100.0])
    scale = np.array([1.0, 0.01, 5.0, 2.0, 0.5, 3.0, 1e3, 1e-2])
    X = (rng.standard_normal((n, 8)) * scale + ratios * scale).astype(np.float32)
    Xd = torch.from_numpy(X).cuda()
    got = features.population_std(hip.col_stats_raw(Xd).cpu().numpy(), n)
    X64 = X.astype(np.float64)
    ref = np.sqrt(((X64 - X64.mean(0)) ** 2).mean(0))
    rel = np.abs(got - ref) / ref
    print("std relative errors", rel)
    assert np.all(np.abs(X64.mean(0)) / ref <= 1e3) and np.max(np.abs(X64.mean(0)) / ref) > 9e2
    assert np.all(rel <= 1e-9), rel
    rounded = features.standard_deviation((X, list("abcdefgh")))
    assert rounded == [round(float(s), 3) for s in got]
    assert np.all(np.abs(np.array(rounded) - np.std(X64, axis=0)) <= 0.5e-3 + 1e-9 * ref)


# ------------------------------------------------------------------------------------------------ 3. dip
def dip_columns(n, C, seed):
    """normal, bimodal, heavily tied (2 decimals) and constant columns in turn."""
    rng = np.random.Generator(np.random.PCG64(seed))
    X = np.empty((n, C), dtype=np.float32)
    for c in range(C):
        kind = c % 4
        z = rng.standard_normal(n)
        if kind == 0:
            X[:, c] = z * rng.uniform(0.1, 10) + rng.uniform(-5, 5)
        elif kind == 1:
            X[:, c] = z + np.where(rng.random(n) < rng.uniform(0.3, 0.7), -2.0, 2.0)
        elif kind == 2:
            X[:, c] = np.round(z, 2)
        else:
            X[:, c] = 1.5
    return X


def assert_dip_matches_restatement(X):
    from deep_cartograph_amd import hip

    Xs = torch.sort(torch.from_numpy(X).cuda(), dim=0).values.contiguous()
    dip, lo, hi = hip.dip_sorted(Xs)
    assert dip.dtype == torch.float64 and lo.dtype == torch.int32 and hi.dtype == torch.int32
    dip, lo, hi = dip.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()
    Xs_h = Xs.cpu().numpy()
    ref = [fo.dip_full(Xs_h[:, c].astype(np.float64)) for c in range(X.shape[1])]
    err = np.abs(dip - np.array([r[0] for r in ref]))
    print(f"n={X.shape[0]} C={X.shape[1]} max |dip - restatement| = {err.max():.3e}")
    assert np.all(err <= 1e-10), err.max()
    assert np.array_equal(lo, np.array([r[1] for r in ref])), "lo differs"
    assert np.array_equal(hi, np.array([r[2] for r in ref])), "hi differs"
    return dip


def test_dip_golden_columns(golden):
    assert_dip_matches_restatement(golden["X"])


@pytest.mark.parametrize("n,C", [(2, 5), (3, 7), (4, 65), (5, 130), (164, 100), (1000, 67), (50000, 12)])
def test_dip_synthetic(n, C):
    dip = assert_dip_matches_restatement(dip_columns(n, C, 100 * n + C))
    assert np.all(dip[3::4] == 0.0)                     # constant columns
    assert np.all(dip[np.arange(C) % 4 != 3] >= 1.0 / (2 * n))


def test_dip_exact_cases():
    from deep_cartograph_amd import hip

    n = 200
    grid = np.arange(n, dtype=np.float32)
    half = np.concatenate([np.linspace(0.0, 1e-3, n // 2), np.linspace(1.0, 1.0 + 1e-3, n // 2)]).astype(np.float32)
    X = np.stack([grid, half, np.full(n, 4.0, dtype=np.float32)], axis=1)
    dip, lo, hi = hip.dip_sorted(torch.from_numpy(X).cuda())
    dip = dip.cpu().numpy()
    assert dip[0] == 1.0 / (2 * n)
    assert abs(dip[1] - 0.25) <= 1.0 / (2 * n)
    assert dip[2] == 0.0
    one = hip.dip_sorted(torch.zeros(1, 3, device="cuda"))[0].cpu().numpy()
    assert np.all(one == 0.0)


# ------------------------------------------------------------------------------------------------ 4. p-values
def test_pvalues_within_the_monte_carlo_bound(golden):
    """Device p (torch generator) against the restatement's p (NumPy generator): two independent Monte-Carlo
    estimates with B samples each differ by a variable of variance 2 p (1 - p) / B; four standard deviations plus
    one count."""
    from deep_cartograph_amd import features

    B = 20000
    X = golden["X"]
    p_dev = np.array(features.dip_test((X, golden["names"]), null_samples=B, seed=0))
    p_ref = fo.pvalues(fo.column_dips(X), fo.null_dips(X.shape[0], B, 0))
    p = 0.5 * (p_dev + p_ref)
    bound = 4.0 * np.sqrt(2.0 * p * (1.0 - p) / B) + 1.0 / B
    excess = np.abs(p_dev - p_ref) - bound
    print("max |dp|", np.abs(p_dev - p_ref).max(), "max excess over the bound", excess.max())
    assert np.all(excess <= 0), (np.abs(p_dev - p_ref).max(), excess.max())
    # cached per (m, samples, seed); a second call gives the same p-values
    assert (X.shape[0], B, 0) in features._null_cache
    assert features.dip_test(pd.DataFrame(X, columns=golden["names"]), null_samples=B, seed=0) == list(p_dev)


# ------------------------------------------------------------------------------------------------ 5. whole tool
def test_filter_features_tool_on_the_reference_fixture(golden, tmp_path):
    """The reference's own test: its configuration, its colvars matrix, its filtered list in order -- after removing
    from both sides the features whose golden hdtp lies in (0.04, 0.06), at most 2 of 202.

    The summary columns follow the reference's Filter: that configuration carries entropy_quantile = std_quantile = 0,
    which is not None, so the entropy and std columns are computed and written (and filter nothing); the committed
    reference summary (name, pass, hdtp) corresponds to the schema defaults, which are checked for those exact columns."""
    from deep_cartograph_amd import colvars, tools
    from deep_cartograph_amd.common import read_features_list

    path = str(tmp_path / "virtual_dihedrals.npy")
    colvars.write_binary_matrix(path, golden["X"], golden["names"])
    hdtp = dict(zip(golden["summary_names"], golden["summary_hdtp"]))
    borderline = {n for n, h in hdtp.items() if 0.04 < h < 0.06}
    assert len(borderline) <= 2
    expected = [f for f in golden["filtered"] if f not in borderline]

    out = str(tmp_path / "out")
    result = tools.filter_features(configuration=reference_test_configuration(), colvars_paths=[path], output_folder=out)
    assert result == os.path.join(out, "filtered_features.txt")
    assert [f for f in read_features_list(result) if f not in borderline] == expected
    assert read_features_list(os.path.join(out, "all_features.txt")) == golden["names"]
    summary = pd.read_csv(os.path.join(out, "filter_summary.csv"))
    assert list(summary.columns) == ["name", "pass", "entropy", "std", "hdtp"]
    assert summary["name"].tolist() == golden["names"]
    assert summary.loc[summary["pass"], "name"].tolist() == read_features_list(result)
    assert ((summary["hdtp"] <= 0.05) == summary["pass"]).all()
    # a second call returns early: nothing is rewritten
    stamp = os.path.getmtime(result)
    os.remove(os.path.join(out, "filter_summary.csv"))
    assert tools.filter_features(configuration=reference_test_configuration(), colvars_paths=[path], output_folder=out) == result
    assert os.path.getmtime(result) == stamp and not os.path.exists(os.path.join(out, "filter_summary.csv"))

    # schema defaults (dip test only): the columns of the reference's committed summary
    out2 = str(tmp_path / "out_defaults")
    result2 = tools.filter_features(configuration={}, colvars_paths=path, output_folder=out2)
    assert read_features_list(result2) == read_features_list(result)
    summary2 = pd.read_csv(os.path.join(out2, "filter_summary.csv"))
    assert list(summary2.columns) == ["name", "pass", "hdtp"]
    assert np.array_equal(summary2["hdtp"].to_numpy(), summary["hdtp"].to_numpy())
    # p-values against the golden column: not a tight pin (see the CPU tests), but the same ranking
    col = {n: i for i, n in enumerate(summary2["name"])}
    mine = np.array([summary2["hdtp"][col[n]] for n in golden["summary_names"]])
    assert np.mean(np.abs(mine - golden["summary_hdtp"])) < 0.03


@pytest.mark.parametrize("entropy_quantile,std_quantile", [(0.25, None), (None, 0.5), (0.3, 0.6)])
def test_quantile_filters_match_the_reference_expressions(golden, tmp_path, entropy_quantile, std_quantile):
    from scipy.stats import entropy

    from deep_cartograph_amd import colvars, tools

    X, names = golden["X"], golden["names"]
    path = str(tmp_path / "m.npy")
    colvars.write_binary_matrix(path, X, names)
    cfg = {"filter_settings": {"diptest_significance_level": None, "entropy_quantile": entropy_quantile, "std_quantile": std_quantile}}
    out = str(tmp_path / "out")
    tools.filter_features(cfg, [path], output_folder=out)
    summary = pd.read_csv(os.path.join(out, "filter_summary.csv"))
    ref = pd.DataFrame({"name": names, "pass": True})
    if entropy_quantile is not None:
        ent = []
        for c in range(X.shape[1]):
            hist, bin_edges = np.histogram(X[:, c], bins=100, density=True)
            ent.append(round(entropy(hist * np.diff(bin_edges), base=2), 3))
        ref["entropy"] = ent
    if std_quantile is not None:
        ref["std"] = [round(np.std(X[:, c]), 3) for c in range(X.shape[1])]
    if entropy_quantile is not None:
        ref.loc[ref["entropy"] < ref["entropy"].quantile(q=entropy_quantile), "pass"] = False
    if std_quantile is not None:
        ref.loc[ref["std"] < ref["std"].quantile(q=std_quantile), "pass"] = False
    assert list(summary.columns) == list(ref.columns)
    assert summary["pass"].tolist() == ref["pass"].tolist()
    assert 0 < summary["pass"].sum() < len(names)


def test_waypoint_filter_through_the_tool(golden, tmp_path):
    from deep_cartograph_amd import colvars, tools
    from deep_cartograph_amd.common import read_features_list

    X, names = golden["X"], golden["names"]
    path = str(tmp_path / "m.npy")
    colvars.write_binary_matrix(path, X, names)
    way = str(tmp_path / "way.npy")
    colvars.write_binary_matrix(way, X[[0, 80, 163]], names)
    out = str(tmp_path / "out")
    kept = read_features_list(tools.filter_features({}, [path], waypoint_colvars_paths=[way], output_folder=out))
    summary = pd.read_csv(os.path.join(out, "filter_summary.csv"))
    assert list(summary.columns) == ["name", "pass", "hdtp", "waypoint_difference"]
    # features the waypoint filter removed are not analysed: they keep hdtp = 1
    removed = summary[~summary["waypoint_difference"].astype(bool)]
    assert len(removed) > 0 and (removed["hdtp"] == 1.0).all() and not removed["pass"].any()
    assert kept == summary.loc[summary["pass"], "name"].tolist()


# ------------------------------------------------------------------------------------------------ 6. scale
def test_filter_at_scale(tmp_path):
    """2 000 000 x 256: 32 planted two-normal mixtures (means 3 standard deviations apart) among 224 normal columns of
    varied mean and scale; exactly the planted columns pass at 0.05.  The separation was chosen with the restatement
    on 50 000 rows (dip 0.0166 against a largest null dip of 0.0036 in 1000 samples; normal columns p >= 0.99), and
    that choice is asserted below."""
    import time

    from deep_cartograph_amd import colvars, features

    n, F, planted_count, sep = 2_000_000, 256, 32, 3.0
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    rng = np.random.Generator(np.random.PCG64(6))
    planted = np.sort(rng.choice(F, planted_count, replace=False))
    scale = torch.from_numpy(rng.uniform(0.05, 20.0, F).astype(np.float32)).cuda()
    mean = torch.from_numpy(rng.uniform(-50.0, 50.0, F).astype(np.float32)).cuda()
    Xd = torch.randn(n, F, generator=gen, device="cuda", dtype=torch.float32)
    side = (torch.rand(n, planted_count, generator=gen, device="cuda") < 0.5).to(torch.float32) * sep - sep / 2
    Xd[:, torch.from_numpy(planted).cuda()] += side
    Xd = Xd * scale + mean
    X = Xd.cpu().numpy()
    del Xd, side
    torch.cuda.empty_cache()
    names = [f"feat-{i}" for i in range(F)]
    path = str(tmp_path / "big.npy")
    colvars.write_binary_matrix(path, X, names)

    # the design criterion, on a 50 000-row subsample with the restatement
    sub = X[:: n // 50000][:50000]
    p_sub = fo.pvalues(fo.column_dips_parallel(sub), fo.null_dips_parallel(50000, 1000, 0))
    is_planted = np.zeros(F, dtype=bool)
    is_planted[planted] = True
    assert np.all(p_sub[is_planted] < 1e-3) and np.all(p_sub[~is_planted] > 0.3), (p_sub[is_planted].max(), p_sub[~is_planted].min())

    settings = {"diptest_significance_level": 0.05, "entropy_quantile": 0, "std_quantile": 0}
    t0 = time.time()
    flt = features.Filter(settings, [path], output_dir=str(tmp_path / "out"))
    kept = flt.run(csv_summary=True)
    print(f"Filter.run 2M x 256: {time.time() - t0:.1f} s")
    assert kept == [names[i] for i in planted]
    summary = pd.read_csv(os.path.join(str(tmp_path / "out"), "filter_summary.csv"))
    assert (summary["hdtp"][is_planted] < 1e-3).all() and (summary["hdtp"][~is_planted] > 0.3).all()

    cols = np.sort(rng.choice(F, 8, replace=False))
    counts, edges = device_counts(torch.from_numpy(X).cuda())
    for c in cols:
        ref, ref_edges = np.histogram(X[:, c], bins=BINS)
        assert np.array_equal(edges[c], ref_edges) and np.array_equal(counts[c], ref), c
    assert np.all(counts.sum(1) == n)


# ------------------------------------------------------------------------------------------------ 7. deep_carto
def _labels(model_zip):
    with zipfile.ZipFile(model_zip) as z:
        return [s for s in z.read("model/features_labels.txt").decode().split("\n") if s]


def test_deep_carto_filters_before_training(golden, tmp_path):
    from deep_cartograph_amd import colvars, deep_carto, tools
    from deep_cartograph_amd.common import read_features_list

    path = str(tmp_path / "virtual_dihedrals.npy")
    colvars.write_binary_matrix(path, golden["X"], golden["names"])
    train = {"cvs": ["pca", "tica"], "common": {"dimension": 2, "features_normalization": "mean_std"}}
    cfg = {"filter_features": reference_test_configuration(), "train_colvars": train, "traj_cluster": {"run": False}}
    out = deep_carto.deep_cartograph(json.loads(json.dumps(cfg)), [path], output_folder=str(tmp_path / "with_filter"))
    run = tmp_path / "with_filter"
    kept = read_features_list(str(run / "filter_features" / "filtered_features.txt"))
    assert 50 <= len(kept) <= 58 and len(set(kept) ^ set(golden["filtered"])) <= 2
    for cv in ("pca", "tica"):
        assert _labels(str(run / "train_colvars" / cv / "model.zip")) == kept
    # the same as training on that list directly
    direct = tools.train_colvars(json.loads(json.dumps(train)), [path], features_list=kept, output_folder=str(tmp_path / "direct"))
    for cv in ("pca", "tica"):
        a, b = pd.read_csv(out["train_colvars"][cv][0]), pd.read_csv(direct[cv][0])
        assert a.equals(b)

    # without the section nothing changes: no filter folder, every feature is used
    cfg.pop("filter_features")
    out2 = deep_carto.deep_cartograph(json.loads(json.dumps(cfg)), [path], output_folder=str(tmp_path / "without"))
    assert not os.path.exists(tmp_path / "without" / "filter_features")
    assert _labels(str(tmp_path / "without" / "train_colvars" / "pca" / "model.zip")) == golden["names"]
    full = tools.train_colvars(json.loads(json.dumps(train)), [path], output_folder=str(tmp_path / "direct_full"))
    assert pd.read_csv(out2["train_colvars"]["pca"][0]).equals(pd.read_csv(full["pca"][0]))
    # a features list given by the caller wins over the section
    cfg["filter_features"] = reference_test_configuration()
    deep_carto.deep_cartograph(json.loads(json.dumps(cfg)), [path], features_list=golden["names"][:10], output_folder=str(tmp_path / "given"))
    assert not os.path.exists(tmp_path / "given" / "filter_features")
    assert _labels(str(tmp_path / "given" / "train_colvars" / "pca" / "model.zip")) == golden["names"][:10]
