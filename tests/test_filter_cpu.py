"""filter_features without a GPU: the float64 restatement of the dip statistic (tests/filter_oracle.py) on exact
cases and on the reference's fixture, the schema defaults, the host-only waypoint filters and threshold rules, and
the absence of a CPU fallback."""
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

from tests import filter_oracle as fo
from tests.conftest import load_golden


@pytest.fixture(scope="module")
def golden():
    g = load_golden("filter_golden.npz")
    return {"X": np.ascontiguousarray(g["X"]), "names": [str(s) for s in g["names"]],
            "filtered": [str(s) for s in g["filtered"]], "summary_names": [str(s) for s in g["summary_names"]],
            "summary_pass": g["summary_pass"], "summary_hdtp": g["summary_hdtp"],
            "schema_defaults": json.loads(str(g["schema_defaults"]))}


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n", [2, 3, 10, 50, 1000])
def test_dip_of_an_equally_spaced_grid_is_the_minimum(n):
    assert fo.dip(np.arange(n, dtype=np.float64)) == 1.0 / (2 * n)


@pytest.mark.parametrize("n", [0, 1, 2, 7, 100])
def test_dip_of_a_constant_column_is_zero(n):
    assert fo.dip(np.full(n, 3.25)) == 0.0


@pytest.mark.parametrize("n", [2, 3])
def test_dip_of_two_and_three_points(n):
    x = np.sort(np.random.RandomState(n).uniform(size=n))
    assert fo.dip(x) == 1.0 / (2 * n)


@pytest.mark.parametrize("n", [20, 200])
def test_dip_of_two_tight_clusters_is_a_quarter(n):
    half = n // 2
    x = np.concatenate([np.linspace(0.0, 1e-3, half), np.linspace(1.0, 1.0 + 1e-3, half)])
    d = fo.dip(x)
    assert abs(d - 0.25) <= 1.0 / (2 * n), d
    assert abs(d - 0.24975) < 5e-6, d


def test_restatement_reproduces_the_reference_list(golden):
    """Dips of the restatement + a NumPy null of 20 000 uniform samples (seed 0) give the reference's filtered list
    exactly, in order."""
    import time

    t0 = time.time()
    dips = fo.column_dips(golden["X"])
    p = fo.pvalues(dips, fo.null_dips(golden["X"].shape[0], 20000, 0))
    kept = [n for n, pv in zip(golden["names"], p) if not pv > 0.05]
    assert kept == golden["filtered"]
    assert time.time() - t0 < 30.0


def test_restatement_dips_rank_like_the_golden_pvalues(golden):
    """Rank correlation of the dips with -golden hdtp (no Monte-Carlo enters).  Measured 0.9968."""
    dips = fo.column_dips(golden["X"])
    col = {n: i for i, n in enumerate(golden["names"])}
    d = np.array([dips[col[n]] for n in golden["summary_names"]])
    rho = fo.spearman(d, -golden["summary_hdtp"])
    print("rank correlation", rho)
    assert rho >= 0.99


def test_golden_summary_is_consistent(golden):
    passed = {n for n, p in zip(golden["summary_names"], golden["summary_pass"]) if p}
    assert passed == set(golden["filtered"])
    h = golden["summary_hdtp"]
    assert int(((h > 0.04) & (h < 0.06)).sum()) <= 2


# ------------------------------------------------------------------------------------------------ schema
def test_schema_defaults(golden):
    from deep_cartograph_amd.schemas import FilterFeaturesSchema

    assert FilterFeaturesSchema().model_dump() == golden["schema_defaults"]
    # unknown fields (the reference's own test passes compute_diptest etc.) are dropped, as in the reference
    cfg = FilterFeaturesSchema(**{"filter_settings": {"compute_diptest": True, "entropy_quantile": 0}}).model_dump()
    assert cfg["filter_settings"] == {"local_distance_threshold": None, "diptest_significance_level": 0.05,
                                      "entropy_quantile": 0.0, "std_quantile": None}


# ------------------------------------------------------------------------------------------------ host-only pieces
def _waypoints():
    ang_moving = np.array([0.1, 0.1 + np.pi / 8 + 0.05, 0.2])
    ang_still = np.array([1.0, 1.0 + np.pi / 8 - 0.05, 1.1])
    cols = {
        "sin-a": np.sin(ang_moving), "cos-a": np.cos(ang_moving),
        "sin-b": np.sin(ang_still), "cos-b": np.cos(ang_still),
        "sin-c": np.array([0.0, 0.1, 0.2]),                            # no cosine partner: kept
        "tor-a": np.array([0.0, 0.5, 0.2]), "tor-b": np.array([0.0, 0.3, 0.2]),
        "coord-@CA_1.x": np.array([0.0, 0.15, 0.0]), "coord-@CA_1.y": np.array([0.0, 0.15, 0.0]),
        "coord-@CA_1.z": np.array([0.0, 0.0, 0.0]),                    # largest distance 0.212 >= 0.2
        "coord-@CA_2.x": np.array([0.0, 0.1, 0.0]), "coord-@CA_2.z": np.array([0.0, 0.1, 0.0]),   # 0.141, y missing
        "dist-a": np.array([0.5, 0.75, 0.6]), "dist-b": np.array([0.5, 0.65, 0.6]),
    }
    return pd.DataFrame(cols)


def test_difference_filter_by_feature_type():
    from deep_cartograph_amd.features import difference_filter

    df = _waypoints()
    expected = {"sin-a": True, "cos-a": True, "sin-b": False, "cos-b": False, "sin-c": True, "tor-a": True, "tor-b": False,
                "coord-@CA_1.x": True, "coord-@CA_1.y": True, "coord-@CA_1.z": True, "coord-@CA_2.x": False,
                "coord-@CA_2.z": False, "dist-a": True, "dist-b": False}
    got = difference_filter(df)
    assert dict(zip(df.columns, got)) == expected
    # the (ndarray, names) form gives the same
    assert difference_filter((df.to_numpy(), list(df.columns))) == got
    assert difference_filter(pd.DataFrame()) == []


def test_min_value_filter():
    from deep_cartograph_amd.features import min_value_filter

    df = _waypoints()[["dist-a", "dist-b", "tor-a"]]
    assert min_value_filter(df, 0.5) == [True, True, True]
    assert min_value_filter(df, 0.4) == [False, False, True]
    assert min_value_filter((df.to_numpy(), list(df.columns)), 0.4) == [False, False, True]


def test_threshold_rules_on_a_synthetic_summary():
    """filter.py:258-272: strictly below the quantile of entropy / std fails, p strictly above the level fails, a
    quantile or level of 0 switches the rule off, failures accumulate."""
    from deep_cartograph_amd.features import apply_thresholds

    def summary():
        return pd.DataFrame({"name": list("abcde"), "pass": [True, True, True, True, False],
                             "entropy": [1.0, 2.0, 3.0, 4.0, 5.0], "std": [0.5, 0.4, 0.3, 0.2, 0.1],
                             "hdtp": [0.0, 0.05, 0.0500001, 0.9, 0.0]})

    assert apply_thresholds(summary(), None, None, 0.05)["pass"].tolist() == [True, True, False, False, False]
    assert apply_thresholds(summary(), None, None, 0)["pass"].tolist() == [True, True, True, True, False]
    # entropy quantile 0.5 -> threshold 3.0: 1.0 and 2.0 fail
    assert apply_thresholds(summary(), 0.5, None, None)["pass"].tolist() == [False, False, True, True, False]
    # std quantile 0.25 -> threshold 0.2: 0.1 fails (already failed)
    assert apply_thresholds(summary(), 0, 0.25, None)["pass"].tolist() == [True, True, True, True, False]
    assert apply_thresholds(summary(), 0.5, 0.5, 0.05)["pass"].tolist() == [False, False, False, False, False]
    s = summary()
    q = s["std"].quantile(q=0.5)
    assert apply_thresholds(s, None, 0.5, None)["pass"].tolist() == [bool(p and v >= q) for p, v in zip(summary()["pass"], summary()["std"])]


def test_entropy_from_counts_is_the_reference_expression():
    from scipy.stats import entropy

    from deep_cartograph_amd.features import entropy_from_counts, histogram_edges

    rng = np.random.Generator(np.random.PCG64(3))
    for col in (rng.standard_normal(5000).astype(np.float32) * 3 + 7, np.full(10, 2.5, dtype=np.float32),
                rng.integers(0, 2, 300).astype(np.float32)):
        hist, bin_edges = np.histogram(col, bins=100, density=True)
        expected = round(entropy(hist * np.diff(bin_edges), base=2), 3)
        edges = histogram_edges([col.min()], [col.max()])
        assert edges.dtype == np.float32 and np.array_equal(edges[0], bin_edges)
        counts = np.histogram(col, bins=100)[0]
        assert entropy_from_counts(counts, edges[0]) == expected


# ------------------------------------------------------------------------------------------------ no CPU fallback
def test_filter_features_needs_a_gpu(golden, tmp_path):
    from deep_cartograph_amd import features, hip, tools
    from deep_cartograph_amd._lib import DcvError
    from deep_cartograph_amd.colvars import write_binary_matrix

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    path = os.path.join(str(tmp_path), "features.npy")
    write_binary_matrix(path, golden["X"], golden["names"])
    with pytest.raises(DcvError):
        tools.filter_features({}, [path], output_folder=os.path.join(str(tmp_path), "out"))
    assert not os.path.exists(os.path.join(str(tmp_path), "out", "filtered_features.txt"))
    X = torch.zeros(8, 4)
    with pytest.raises(DcvError):
        hip.col_histogram(X, torch.zeros(4, 101))
    with pytest.raises(DcvError):
        hip.dip_sorted(X)
    for fn in (features.shannon_entropy, features.standard_deviation, features.dip_test):
        with pytest.raises(DcvError):
            fn((golden["X"], golden["names"]))
