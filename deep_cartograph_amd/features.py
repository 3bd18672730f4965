"""Feature filtering with the reference's semantics (deep_cartograph/modules/features/filter.py and the feature
statistics of modules/statistics/statistics.py:381-635), computed on the MI355X.

The reference re-reads every colvars file once per feature and runs np.histogram, np.std and Hartigan's dip test
per feature on one core.  Here the frames x features matrix is loaded ONCE (colvars.load_feature_matrix), kept on
the device and reduced in a few passes:

  entropy   dcv_col_histogram counts (equal to np.histogram's), then the reference's float64 expressions on the host
  std       dcv_col_stats sums, population standard deviation
  dip test  torch.sort per column chunk (plumbing) + dcv_dip_sorted; the p-value comes from a simulated null
            distribution of the dip of uniform samples, computed through the same kernel (what the diptest package
            does under boot_pval=True; its table of critical values is not used)

The two waypoint filters look at a handful of structures and stay on the host.  There is no CPU path for the
device statistics: without a GPU they raise DcvError."""
from __future__ import annotations

import logging
import os
import sys
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import pandas as pd

from ._lib import DcvError

logger = logging.getLogger(__name__)

HISTOGRAM_BINS = 100          # np.histogram(bins=100) of the reference's shannon_entropy
NULL_MAX_SAMPLE_SIZE = 72000  # the diptest package's table stops here too; beyond it sqrt(n) * dip is compared
NULL_GENERATION_BLOCK = 1024  # columns drawn per torch.rand call: the null does not depend on the memory budget

FeaturesInput = Union[pd.DataFrame, Tuple[np.ndarray, Sequence[str]]]

_null_cache: Dict[Tuple[int, int, int], np.ndarray] = {}


# ------------------------------------------------------------------------------------------------ inputs
def _as_matrix(features) -> Tuple[np.ndarray, List[str]]:
    if isinstance(features, pd.DataFrame):
        return features.to_numpy(), [str(c) for c in features.columns]
    X, names = features
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] != len(names):
        raise ValueError(f"expected an (n x F matrix, F names) pair, got shape {X.shape} and {len(names)} names")
    return X, list(names)


def _device():
    import torch

    if not torch.cuda.is_available():
        raise DcvError("the feature statistics run on an MI355X (cuda) device; none is available and there is no CPU fallback")
    return torch.device("cuda")


def _to_device(features):
    """n x F float32 device tensor of a DataFrame, an (ndarray, names) pair or a device tensor."""
    import torch

    if isinstance(features, torch.Tensor):
        if not features.is_cuda:
            raise DcvError("the feature statistics need the matrix on an MI355X (cuda) device; got a CPU tensor")
        return features
    X, _ = _as_matrix(features)
    dev = _device()
    return torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)


# ------------------------------------------------------------------------------------------------ entropy, std
def histogram_edges(col_min: np.ndarray, col_max: np.ndarray, bins: int = HISTOGRAM_BINS) -> np.ndarray:
    """[F, bins + 1] float32: the edges np.histogram(column, bins) uses for a float32 column with that minimum and
    maximum (they depend on nothing else), built by NumPy itself, +-0.5 expansion of a constant column included."""
    mn = np.asarray(col_min, dtype=np.float32)
    mx = np.asarray(col_max, dtype=np.float32)
    edges = np.empty((mn.size, bins + 1), dtype=np.float32)
    for f in range(mn.size):
        edges[f] = np.histogram_bin_edges(np.array([mn[f], mx[f]], dtype=np.float32), bins=bins)
    return edges


def entropy_from_counts(counts: np.ndarray, edges: np.ndarray) -> float:
    """round(scipy.stats.entropy(hist * diff(edges), base=2), 3) with hist = np.histogram(..., density=True)[0],
    from the counts and the float32 edges, in the reference's order of operations (statistics.py:560-564)."""
    from scipy.stats import entropy

    n = np.asarray(counts)
    db = np.array(np.diff(edges), float)
    hist = n / db / n.sum()
    prob_distribution = hist * np.diff(edges)
    return round(entropy(prob_distribution, base=2), 3)


def _column_stats(Xd):
    from . import hip

    return hip.col_stats_raw(Xd).cpu().numpy()


def _shannon_entropy_device(Xd, raw: Optional[np.ndarray] = None) -> List[float]:
    import torch

    from . import hip

    if raw is None:
        raw = _column_stats(Xd)
    edges = histogram_edges(raw[2], raw[3])
    counts = hip.col_histogram(Xd, torch.from_numpy(edges).to(Xd.device)).cpu().numpy()
    return [entropy_from_counts(counts[f], edges[f]) for f in range(edges.shape[0])]


def population_std(raw: np.ndarray, n: int) -> np.ndarray:
    """float64 standard deviation (ddof = 0) of every column from the raw sums of dcv_col_stats."""
    mean = raw[0] / n
    return np.sqrt(np.maximum(raw[1] / n - mean * mean, 0.0))


def _standard_deviation_device(Xd, raw: Optional[np.ndarray] = None) -> List[float]:
    if raw is None:
        raw = _column_stats(Xd)
    return [round(float(s), 3) for s in population_std(raw, Xd.shape[0])]


def shannon_entropy(features_df: FeaturesInput) -> List[float]:
    """Shannon entropy (bits) of the 100-bin histogram of each feature (statistics.py:514-566)."""
    return _shannon_entropy_device(_to_device(features_df))


def standard_deviation(features_df: FeaturesInput) -> List[float]:
    """Population standard deviation of each feature, rounded to 3 decimals (statistics.py:568-593)."""
    return _standard_deviation_device(_to_device(features_df))


# ------------------------------------------------------------------------------------------------ dip test
def _dip_budget(device, memory_budget: Optional[int]) -> int:
    import torch

    if memory_budget is not None:
        return int(memory_budget)
    torch.cuda.empty_cache()   # blocks torch's allocator caches count as used otherwise
    free, _ = torch.cuda.mem_get_info(device)
    return int(free // 2)


def _chunk_columns(n: int, F: int, budget: int) -> int:
    # per column: sorted values (4 B), torch.sort's indices (8 B) and a strided-input copy (4 B) per row, and the
    # four int32 work arrays of dcv_dip_sorted (16 B per row)
    C = max(1, min(F, budget // (32 * (n + 1))))
    if C >= 64:
        C -= C % 64   # whole waves
    return C


def dip_statistic(Xd, memory_budget: Optional[int] = None) -> np.ndarray:
    """float64 dip statistic of every column of the n x F float32 device matrix: sort (torch) and dcv_dip_sorted per
    chunk of columns; the chunk is sized so that the sort's temporaries and the kernel's workspace fit the budget
    (default: half of the free device memory)."""
    import torch

    from . import hip

    n, F = Xd.shape
    C = _chunk_columns(n, F, _dip_budget(Xd.device, memory_budget))
    out = np.empty(F, dtype=np.float64)
    for c0 in range(0, F, C):
        Xs = torch.sort(Xd[:, c0:c0 + C], dim=0).values
        dip, _, _ = hip.dip_sorted(Xs if Xs.is_contiguous() else Xs.contiguous())
        out[c0:c0 + C] = dip.cpu().numpy()
        del Xs, dip
    return out


def dip_null_distribution(m: int, null_samples: int = 20000, seed: int = 0, memory_budget: Optional[int] = None) -> np.ndarray:
    """Sorted float64 dips of `null_samples` samples of m U(0,1) values, drawn on the device with a seeded torch
    generator in blocks of NULL_GENERATION_BLOCK columns and reduced by dcv_dip_sorted.  Cached per
    (m, null_samples, seed) within the process."""
    import torch

    from . import hip

    key = (int(m), int(null_samples), int(seed))
    if key in _null_cache:
        return _null_cache[key]
    dev = _device()
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    # besides what a data chunk needs, the uniform draws themselves (4 B per row) live next to the sort
    per_chunk = max(NULL_GENERATION_BLOCK, _chunk_columns(m, null_samples, _dip_budget(dev, memory_budget) * 8 // 9))
    per_chunk -= per_chunk % NULL_GENERATION_BLOCK
    out = np.empty(null_samples, dtype=np.float64)
    done = 0
    while done < null_samples:
        take = min(per_chunk, null_samples - done)
        blocks = [torch.rand(m, min(NULL_GENERATION_BLOCK, take - b), generator=gen, device=dev, dtype=torch.float32)
                  for b in range(0, take, NULL_GENERATION_BLOCK)]
        U = blocks[0] if len(blocks) == 1 else torch.cat(blocks, dim=1)
        del blocks
        Us = torch.sort(U, dim=0).values
        del U
        dip, _, _ = hip.dip_sorted(Us)
        out[done:done + take] = dip.cpu().numpy()
        del Us, dip
        done += take
    out.sort()
    _null_cache[key] = out
    return out


def dip_pvalues(dips: np.ndarray, n: int, null_sorted: np.ndarray, m: int) -> np.ndarray:
    """p = mean(null_dip >= dip); for n > m both sides are compared as sqrt(sample size) * dip."""
    dips = np.asarray(dips, dtype=np.float64)
    if n == m:
        ref, val = null_sorted, dips
    else:
        ref, val = np.sqrt(float(m)) * null_sorted, np.sqrt(float(n)) * dips
    below = np.searchsorted(ref, val, side="left")   # number of null dips strictly below
    return (ref.size - below) / float(ref.size)


def _dip_test_device(Xd, null_samples: int, seed: int, memory_budget: Optional[int] = None) -> List[float]:
    n = int(Xd.shape[0])
    dips = dip_statistic(Xd, memory_budget)
    m = min(n, NULL_MAX_SAMPLE_SIZE)
    null = dip_null_distribution(m, null_samples, seed, memory_budget)
    return [float(p) for p in dip_pvalues(dips, n, null, m)]


def dip_test(features_df: FeaturesInput, null_samples: int = 20000, seed: int = 0) -> List[float]:
    """p-value of Hartigan's dip test of each feature (statistics.py:595-635); small = evidence against unimodality.
    The p-value is the fraction of `null_samples` simulated uniform samples of min(n, 72000) points whose dip is at
    least the feature's."""
    return _dip_test_device(_to_device(features_df), null_samples, seed)


# ------------------------------------------------------------------------------------------------ waypoint filters (host)
def difference_filter(features_df: FeaturesInput) -> List[bool]:
    """Does each feature change across the samples (waypoint structures) by more than a threshold that depends on
    its type: pi/8 for sin-/cos- pairs (through the angle) and tor- features, 0.2 nm for coord- triples (largest
    pairwise distance of the atom) and for every other feature (statistics.py:382-485)."""
    from scipy.spatial import distance_matrix

    angle_threshold = np.pi / 8
    distance_threshold = 0.2
    X, names = _as_matrix(features_df)
    if X.size == 0:
        logger.warning("Features dataframe is empty. Returning empty list.")
        return []
    col = {n: X[:, i] for i, n in enumerate(names)}
    above: Dict[str, object] = {n: np.nan for n in names}
    atoms_touched = set()
    for name in names:
        parts = name.split("-")
        if not len(parts) > 1:
            logger.error(f"Feature name {name} does not contain a '-' character. Skipping this feature.")
            continue
        kind = parts[0]
        if kind == "sin":
            cosine_name = name.replace("sin", "cos")
            if cosine_name in col:
                angles = np.arctan2(col[name], col[cosine_name]) + np.pi
                delta = np.abs(np.max(angles) - np.min(angles))
            else:
                logger.warning(f"Cosine component {cosine_name} not found for sine component {name}. Skipping this feature.")
                delta = 10
            above[name] = bool(delta >= angle_threshold)
            if cosine_name in col:
                above[cosine_name] = bool(delta >= angle_threshold)
        elif kind == "cos":
            continue
        elif kind == "tor":
            above[name] = bool(np.max(col[name]) - np.min(col[name]) >= angle_threshold)
        elif kind == "coord":
            atom = parts[1].split(".")[0]
            if atom in atoms_touched:
                continue
            atoms_touched.add(atom)
            axes = [f"coord-{atom}.{a}" for a in "xyz"]
            coordinates = np.vstack([col[a] if a in col else np.zeros(X.shape[0]) for a in axes]).T
            big = bool(np.max(distance_matrix(coordinates, coordinates)) >= distance_threshold)
            for a in axes:
                if a in col:
                    above[a] = big
        else:
            above[name] = bool(np.abs(np.max(col[name]) - np.min(col[name])) >= distance_threshold)
    return [above[n] for n in names]


def min_value_filter(features_df: FeaturesInput, threshold: float) -> List[bool]:
    """Is the minimum of each feature across the samples at most `threshold` (statistics.py:487-511)."""
    X, names = _as_matrix(features_df)
    return [bool(np.min(X[:, i]) <= threshold) for i in range(len(names))]


# ------------------------------------------------------------------------------------------------ pass logic
def apply_thresholds(features_data: pd.DataFrame, entropy_quantile: Optional[float], std_quantile: Optional[float],
                     diptest_significance_level: Optional[float]) -> pd.DataFrame:
    """The reference's threshold rules on a summary with columns name, pass and any of entropy, std, hdtp
    (filter.py:258-272): below the quantile of entropy / std fails, a dip-test p-value above the level fails."""
    if entropy_quantile is not None and entropy_quantile > 0:
        entropy_threshold = features_data["entropy"].quantile(q=entropy_quantile)
        logger.info(f"    Entropy threshold: {entropy_threshold:.2f} bits (quantile: {entropy_quantile:.2f})")
        features_data.loc[(features_data["entropy"] < entropy_threshold), "pass"] = False
    if std_quantile is not None and std_quantile > 0:
        std_threshold = features_data["std"].quantile(q=std_quantile)
        logger.info(f"    Standard deviation threshold: {std_threshold:.2f} a.u. (quantile: {std_quantile:.2f})")
        features_data.loc[(features_data["std"] < std_threshold), "pass"] = False
    if diptest_significance_level is not None and diptest_significance_level > 0:
        features_data.loc[(features_data["hdtp"] > diptest_significance_level), "pass"] = False
    return features_data


class Filter:
    """Reads colvars files with feature time series and filters the features by entropy, standard deviation,
    Hartigan's dip test or their values across waypoint structures (the reference's Filter: same constructor, same
    run(), same summary).  Topologies are accepted and recorded, feature names are not translated between them:
    the files are expected to share feature names, as in CVCalculator.load_training_data."""

    def __init__(self, settings: Dict, colvars_paths: List[str], waypoint_colvars_paths: Optional[List[str]] = None,
                 topologies: Optional[List[str]] = None, waypoint_topologies: Optional[List[str]] = None,
                 reference_topology: Optional[str] = None, output_dir: Optional[str] = "filter_features") -> None:
        from .common import save_list

        self.colvars_paths = [colvars_paths] if isinstance(colvars_paths, str) else list(colvars_paths)
        self.waypoint_colvars_paths = waypoint_colvars_paths
        self.output_dir = output_dir
        if topologies and reference_topology is None:
            reference_topology = topologies[0]
        self.topology_paths = topologies
        self.waypoint_topologies = waypoint_topologies
        self.ref_topology_path = reference_topology
        if self.topology_paths:
            if len(self.colvars_paths) != len(self.topology_paths):
                logger.error("The number of colvars files must be equal to the number of topology files.")
                sys.exit(1)
            logger.warning("Topology-based feature-name translation is not performed: the colvars files must share feature names.")

        self.common_ref_features = self.find_common_features()
        logger.info(f"Initial size of features set (only common features): {len(self.common_ref_features)}.")
        os.makedirs(self.output_dir, exist_ok=True)
        save_list(self.common_ref_features, os.path.join(self.output_dir, "all_features.txt"))

        distance_threshold_angstroms = settings.get("local_distance_threshold", None)
        self.local_distance_threshold = distance_threshold_angstroms / 10 if distance_threshold_angstroms is not None else None
        self.diptest_significance_level = settings["diptest_significance_level"]
        self.entropy_quantile = settings["entropy_quantile"]
        self.std_quantile = settings["std_quantile"]
        self.diptest_filter = self.diptest_significance_level is not None
        self.entropy_filter = self.entropy_quantile is not None
        self.std_filter = self.std_quantile is not None
        self.local_contact_filter = self.local_distance_threshold is not None
        self.filter_features = self.diptest_filter or self.entropy_filter or self.std_filter or (self.waypoint_colvars_paths is not None)
        # keyword arguments of dip_test, not YAML fields
        self.null_samples = 20000
        self.null_seed = 0
        self.memory_budget: Optional[int] = None

        self.features_data = pd.DataFrame({"name": self.common_ref_features, "pass": True})
        if self.entropy_filter:
            self.features_data["entropy"] = 0.0
        if self.std_filter:
            self.features_data["std"] = 0.0
        if self.diptest_filter:
            self.features_data["hdtp"] = 1.0
        if self.waypoint_colvars_paths is not None:
            self.features_data["waypoint_difference"] = True
        if self.local_contact_filter:
            self.features_data["is_local_contact"] = True

    def find_common_features(self) -> List[str]:
        """Features present in every colvars file, in the order of the first file."""
        from .colvars import read_column_names

        common_features = None
        for colvars_path in self.colvars_paths:
            feature_names = read_column_names(colvars_path, features_only=True)
            if common_features:
                present = set(feature_names)
                common_features = [f for f in common_features if f in present]
            else:
                common_features = feature_names
        if not common_features:
            logger.error("No common features found in the colvars files.")
            sys.exit(1)
        return list(common_features)

    def run(self, csv_summary: bool = False) -> list:
        """Filter the features; returns the names that pass, in order.  csv_summary: write filter_summary.csv."""
        from .colvars import load_feature_matrix

        total_num_features = len(self.common_ref_features)
        if self.filter_features:
            if self.waypoint_colvars_paths is not None:
                W, _, _ = load_feature_matrix(self.waypoint_colvars_paths, features_list=self.common_ref_features)
                waypoints = (W, self.common_ref_features)
                self.features_data["waypoint_difference"] = difference_filter(waypoints)
                self.features_data.loc[(self.features_data["waypoint_difference"] == False), "pass"] = False  # noqa: E712
                if self.local_contact_filter:
                    self.features_data["is_local_contact"] = min_value_filter(waypoints, self.local_distance_threshold)
                    self.features_data.loc[(self.features_data["is_local_contact"] == False), "pass"] = False  # noqa: E712
            if self.entropy_filter or self.std_filter or self.diptest_filter:
                import torch

                dev = _device()
                # features the waypoint filters removed are not analysed and keep the initial values, as in the reference
                todo = np.flatnonzero(self.features_data["pass"].to_numpy(dtype=bool))
                if todo.size:
                    names = [self.common_ref_features[i] for i in todo]
                    X, _, _ = load_feature_matrix(self.colvars_paths, features_list=names)   # one read of every file
                    Xd = torch.from_numpy(X).to(dev)
                    del X
                    raw = _column_stats(Xd) if (self.entropy_filter or self.std_filter) else None
                    rows = self.features_data.index[todo]
                    if self.entropy_filter:
                        self.features_data.loc[rows, "entropy"] = _shannon_entropy_device(Xd, raw)
                    if self.std_filter:
                        self.features_data.loc[rows, "std"] = _standard_deviation_device(Xd, raw)
                    if self.diptest_filter:
                        self.features_data.loc[rows, "hdtp"] = _dip_test_device(Xd, self.null_samples, self.null_seed, self.memory_budget)
                    del Xd

        apply_thresholds(self.features_data, self.entropy_quantile if self.entropy_filter else None,
                         self.std_quantile if self.std_filter else None,
                         self.diptest_significance_level if self.diptest_filter else None)
        if csv_summary:
            self.features_data.to_csv(os.path.join(self.output_dir, "filter_summary.csv"), index=False)
        self.features_data = self.features_data[self.features_data["pass"] == 1]
        logger.info(f"Filtered {total_num_features - len(self.features_data)} features.")
        return self.features_data["name"].tolist()
