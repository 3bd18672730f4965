"""Collective-variable calculators: host-side mirror of the reference's
deep_cartograph/modules/cv_learning/cv_calculator.py (class tree, method names, argument meaning,
output files and error behaviour) over the HIP kernels of libdcv.so.

    cv_calculators_map[name](configuration, output_path)
        .load_training_data(paths, topologies, ref_topology, features_list)
        .run(dimension) -> DataFrame of the projected training frames (None = fit failed)
        .project_colvars(...) / .project_data(...)
    CVCalculator.load(model.zip, output_path)

The frames x features matrix lives on the GPU from load_training_data on; statistics,
normalisation, covariance, projection and the AE / Deep-TICA training are HIP kernels, the
F x F (or d x d) eigen-solves run on the host in float64 (linalg.py).  With torch.distributed
initialised every rank holds a contiguous block of frames and the small result buffers are
all-reduced (parallel.py).  There is no CPU fallback.
"""
from __future__ import annotations

import copy
import json
import logging
import os
import shutil
from abc import ABC, abstractmethod
from pathlib import Path
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import pandas as pd
import torch

from . import export, hip, linalg
from .colvars import load_feature_matrix
from .common import closest_power_of_two, remove_files, unzip_files, zip_files
from .fit import FitPlan, Try, _Batches, _HostLRScheduler, _torch_threads  # noqa: F401  (the training driver; names importable from here)
from .parallel import Comm, append_halo, reduce_col_stats, reduce_minmax

logger = logging.getLogger(__name__)


def _to_host(t: torch.Tensor) -> torch.Tensor:
    """Device -> host copy of a projection through page-locked memory of torch's caching host allocator: a fresh
    pageable buffer of tens of MB costs its page faults on every call (measured 3.5 ms against 60-90 ms for 5M x 2)."""
    host = torch.empty(t.shape, dtype=t.dtype, device="cpu", pin_memory=True)
    host.copy_(t)
    return host


def _dev(a, device, dtype=torch.float32) -> torch.Tensor:
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(device)


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise hip.DcvError("deep_cartograph_amd needs an MI355X: torch.cuda.is_available() is False and there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


class CVCalculator(ABC):
    """Base class (reference: cv_calculator.py:23-747)."""

    def __init__(self, configuration: Optional[Dict] = None, output_path: Optional[str] = None):
        self.configuration: Dict = copy.deepcopy(configuration) if configuration is not None else {}
        self.architecture_config: Dict = self.configuration.get("architecture", {})
        self.training_reading_settings: Dict = self.configuration.get("input_colvars", {}) or {}
        self.feats_norm_mode = self.configuration.get("features_normalization", None)
        self.bias: Dict = self.configuration.get("bias", {})
        self.ref_topology_path: Optional[str] = None
        self.training_data: Optional[torch.Tensor] = None      # device, [frames of this rank, F]
        self.training_data_labels: Optional[np.ndarray] = None
        self.validation_data: Optional[torch.Tensor] = None
        self.projection_data_labels: Optional[np.ndarray] = None
        self.features_ref_labels: List[str] = []
        self.features_stats: Dict[str, np.ndarray] = {}
        self.features_norm_mean: Optional[np.ndarray] = None
        self.features_norm_range: Optional[np.ndarray] = None
        self.num_features: int = 0
        self.num_frames_global: int = 0
        self.cv = None
        self.cv_dimension: int = self.configuration.get("dimension")
        self.cv_labels: List[str] = []
        self.cv_name: str = None
        self.cv_range: List[Tuple[float, float]] = []
        self.parent_output_path: str = output_path
        self.plumed_files: List[str] = []
        self.temp_model_path: Optional[str] = None
        self.comm = Comm()

    def __del__(self):
        try:
            if self.temp_model_path and os.path.exists(self.temp_model_path):
                shutil.rmtree(self.temp_model_path)
        except Exception:
            pass

    # ------------------------------------------------------------------ loading a saved model
    @classmethod
    def load(cls, model_path: str, output_path: str):
        """Factory: model.zip -> the right calculator, ready to project (reference :92-149)."""
        if not os.path.exists(model_path):
            raise FileNotFoundError(f"Model file not found: {model_path}")
        temp_model_path = os.path.join(output_path, "model")
        unzip_files(model_path, output_path)
        metadata_path = os.path.join(temp_model_path, "metadata.json")
        cv_name = None
        if os.path.exists(metadata_path):
            with open(metadata_path) as f:
                cv_name = json.load(f).get("cv_name")
        else:
            logger.error(f"Metadata file not found in the model: {metadata_path}")
        if not cv_name:
            raise ValueError("Could not determine the CV name from the model file.")
        klass = calculator_class(cv_name)
        if not klass:
            raise TypeError(f"Unknown CV calculator name: {cv_name}")
        inst = klass(output_path=output_path)
        inst._load_from_folder(temp_model_path)
        inst.temp_model_path = temp_model_path
        return inst

    def _load_from_folder(self, folder_path: str):
        with open(os.path.join(folder_path, "metadata.json")) as f:
            meta = json.load(f)
        self.cv_dimension = meta.get("cv_dimension")
        self.cv_name = meta.get("cv_name")
        self.set_labels()
        self.model_output_folder = os.path.join(self.parent_output_path, self.cv_name, "model")
        if os.path.exists(self.model_output_folder):
            shutil.rmtree(self.model_output_folder)
        shutil.copytree(folder_path, self.model_output_folder)
        with open(os.path.join(self.model_output_folder, "features_labels.txt")) as f:
            self.features_ref_labels = f.read().strip().split("\n")
        self.num_features = len(self.features_ref_labels)
        ref = os.path.join(self.model_output_folder, "ref_topology.pdb")
        self.ref_topology_path = ref if os.path.exists(ref) else None

    def create_output_folders(self):
        self.output_path = Path(self.parent_output_path) / self.cv_name
        self.sensitivity_output_folder = self.output_path / "sensitivity_analysis"
        self.training_output_folder = self.output_path / "training"
        self.model_output_folder = self.output_path / "model"
        if self.comm.rank == 0:
            for p in (self.output_path, self.sensitivity_output_folder, self.training_output_folder, self.model_output_folder):
                p.mkdir(parents=True, exist_ok=True)
        self.comm.barrier()

    # ------------------------------------------------------------------ data
    def _read(self, paths, features_list):
        """Colvars files -> (this rank's contiguous block of the frames, names, labels of ALL frames)."""
        s = self.training_reading_settings
        shard = (self.comm.world, self.comm.rank) if self.comm.active else None
        return load_feature_matrix(paths, features_list, start=s.get("start", 0), stop=s.get("stop"), stride=s.get("stride", 1), shard=shard)

    def load_training_data(self, train_colvars_paths: List[str], train_topology_paths: Optional[List[str]] = None,
                           ref_topology_path: Optional[str] = None, features_list: Optional[List[str]] = None):
        """Read the colvars files, keep the matrix on the GPU, compute the feature statistics
        with the HIP column-statistics kernel (reference :248-300)."""
        self.ref_topology_path = ref_topology_path
        if train_topology_paths is not None and self.ref_topology_path is None:
            self.ref_topology_path = train_topology_paths[0]
        logger.info("Reading training data from colvars files...")
        X, names, labels = self._read(train_colvars_paths, features_list)
        self.set_training_matrix(X, names, labels)

    def set_training_matrix(self, X, feature_names: Optional[List[str]] = None, labels: Optional[np.ndarray] = None):
        """Entry point for callers that already hold the (shard of the) feature matrix: a float32
        array / tensor of this rank's frames (under torch.distributed: the rank's contiguous block, blocks
        in rank order forming the trajectory).  A device tensor is adopted without a copy.  `labels`:
        trajectory index of every frame of ALL ranks."""
        dev = _device()
        if isinstance(X, torch.Tensor):
            Xd = X.to(device=dev, dtype=torch.float32)
        else:
            Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
        if Xd.dim() != 2:
            raise ValueError("feature matrix must be 2-D")
        self.training_data = Xd.contiguous()
        n_local, F = self.training_data.shape
        self.features_ref_labels = list(feature_names) if feature_names is not None else [f"f{i}" for i in range(F)]
        self.num_features = F
        logger.info(f"Number of features: {self.num_features}")
        raw = reduce_col_stats(hip.col_stats_raw(self.training_data), self.comm)
        self.num_frames_global = int(round(self.comm.sum_scalar(n_local, device=dev)))
        self.training_data_labels = labels if labels is not None else np.zeros(self.num_frames_global, dtype=np.int64)
        if len(self.training_data_labels) != self.num_frames_global:
            raise ValueError(f"{len(self.training_data_labels)} trajectory labels for {self.num_frames_global} frames")
        self.features_stats = hip.finalize_stats(raw, self.num_frames_global)
        self.features_norm_mean, self.features_norm_range = self.prepare_normalization()

    def load_validation_data(self, val_colvars_paths: List[str], val_topology_paths: Optional[List[str]] = None,
                             ref_topology_path: Optional[str] = None, features_list: Optional[List[str]] = None):
        """Separate validation set (reference :208-246): the fit then trains on ALL training samples and
        evaluates on these frames instead of splitting (:1485-1492)."""
        logger.info("Reading validation data from colvars files...")
        X, _, _ = self._read(val_colvars_paths, features_list)
        self.set_validation_matrix(X)

    def set_validation_matrix(self, X):
        dev = _device()
        Xd = X.to(device=dev, dtype=torch.float32) if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
        if Xd.dim() != 2 or (self.num_features and Xd.shape[1] != self.num_features):
            raise ValueError("validation matrix must be 2-D with the training features")
        self.validation_data = Xd.contiguous()

    def cv_ready(self) -> bool:
        return self.cv is not None

    def prepare_normalization(self) -> Tuple[np.ndarray, np.ndarray]:
        """(mean, range) of the chosen mode; |range| < 1e-8 -> 1 (reference :308-363)."""
        st = self.features_stats
        mode = self.feats_norm_mode
        if mode is None:
            means = np.zeros(len(st["mean"]))
            ranges = np.ones(len(st["mean"]))
        elif mode == "mean_std":
            means, ranges = st["mean"], st["std"]
        elif mode == "min_max_range1":
            means, ranges = st["min"], st["max"] - st["min"]
        elif mode == "min_max_range2":
            means, ranges = (st["min"] + st["max"]) / 2, (st["max"] - st["min"]) / 2
        else:
            logger.error(f"Normalization mode {mode} not recognized. Exiting...")
            raise ValueError(f"Normalization mode {mode} not recognized.")
        ranges = np.array(ranges, copy=True)
        for i in np.where(np.abs(ranges) < 1e-8)[0]:
            ranges[i] = 1.0
            logger.warning(f"Range for feature {i} is close to zero. Setting it to 1.0.")
        return np.asarray(means), ranges

    # ------------------------------------------------------------------ driver
    def run(self, cv_dimension: Union[int, None] = None) -> Union[pd.DataFrame, None]:
        """compute_cv -> normalize_cv -> project the training frames -> save_model ->
        sensitivity_analysis (reference :366-414).  Returns None when the fit failed."""
        if self.training_data is None:
            logger.error("Training data not loaded. Cannot compute CV.")
            return None
        self.create_output_folders()
        if cv_dimension:
            self.cv_dimension = cv_dimension
        self.compute_cv()
        self.set_labels()
        projection_df = None
        if self.cv is not None:
            self.normalize_cv()
            projection = self.project_data(self.training_data, normalize_data=False)
            if self.comm.active:   # every rank returns the projection of ALL training frames (rank order = frame order)
                projection = _to_host(self.comm.all_gather_rows(projection.to(self.training_data.device)))
            if self.comm.rank == 0:
                self.save_model()
            self.sensitivity_analysis()   # every rank computes (collectives inside), rank 0 writes
            self.comm.barrier()
            projection_df = pd.DataFrame(projection.numpy(), columns=self.cv_labels)
        return projection_df

    @abstractmethod
    def compute_cv(self):
        raise NotImplementedError

    @abstractmethod
    def save_weights(self, weights_path: str):
        raise NotImplementedError

    def save_model(self):
        """Files common to every calculator: metadata.json, features_labels.txt,
        ref_topology.pdb (reference :436-452)."""
        with open(os.path.join(self.model_output_folder, "metadata.json"), "w") as f:
            json.dump({"cv_name": self.cv_name, "cv_dimension": self.cv_dimension}, f)
        np.savetxt(os.path.join(self.model_output_folder, "features_labels.txt"), self.features_ref_labels, fmt="%s")
        if self.ref_topology_path is not None and os.path.exists(self.ref_topology_path):
            shutil.copyfile(self.ref_topology_path, os.path.join(self.model_output_folder, "ref_topology.pdb"))

    @abstractmethod
    def get_cv_parameters(self) -> Dict:
        raise NotImplementedError

    @abstractmethod
    def get_cv_type(self) -> str:
        raise NotImplementedError

    @abstractmethod
    def project_data(self, data, normalize_data: bool = True) -> torch.Tensor:
        raise NotImplementedError

    @abstractmethod
    def normalize_cv(self):
        raise NotImplementedError

    def sensitivity_analysis(self):
        return

    def project_colvars(self, colvars_paths: Union[List[str], str], topology_paths: Union[List[str], str, None] = None
                        ) -> Union[pd.DataFrame, None]:
        """Project colvars files with a fitted / loaded CV (reference :478-526).  Unlike the
        reference a model without reference topology still projects:
        the files must then carry the training feature names."""
        if self.ref_topology_path is None:
            logger.warning("Reference topology not set. Make sure the colvars file matches the training data.")
        X, _, labels = load_feature_matrix(colvars_paths, self.features_ref_labels)
        self.projection_data_labels = labels
        projected = self.project_data(torch.from_numpy(X))
        return pd.DataFrame(projected.numpy(), columns=self.cv_labels)

    def project_trajectory(self, trajectory_path: str, topology_path: str, traj_stride: int = 1,
                           memory_budget: Optional[int] = None) -> pd.DataFrame:
        """Project a trajectory (.dcd / .npy; a GROMACS .xtc is imported first) with a fitted / loaded CV straight from its coordinates: the model's own
        feature names are turned back into atoms of ``topology_path`` (trajectory.definitions_from_labels), so neither a
        colvars file nor the features configuration of the training run is needed.  Frames are streamed in chunks
        (frame_io.stream: ``memory_budget`` bytes of device memory per chunk, DCD records read in
        place); only the frames x d result leaves the device.  Columns: the CV labels, as project_colvars.  No CPU fallback."""
        from . import frame_io, trajectory, xtc
        from .tools import ANGSTROM_TO_NM

        if self.cv is None:
            raise ValueError("CV has not been computed. Cannot project a trajectory.")
        trajectory_path = xtc.route(trajectory_path, str(self.parent_output_path), memory_budget)   # a GROMACS .xtc is imported first
        for path in (trajectory_path, topology_path):
            if not os.path.exists(path):
                raise FileNotFoundError(f"File not found: {path}")
        if not torch.cuda.is_available():
            raise hip.DcvError("project_trajectory needs an MI355X (cuda) device: the features are computed by libdcv.so, there is no CPU fallback")
        stride = int(traj_stride)
        if stride < 1:
            raise ValueError(f"traj_stride must be at least 1, got {stride}")
        top = trajectory.read_topology(topology_path)
        records = trajectory.definitions_from_labels(self.features_ref_labels, top)
        traj = trajectory.open_trajectory(trajectory_path, top.n_atoms)
        n = traj.layout(0, None, stride)[0]
        if n == 0:
            raise ValueError(f"{trajectory_path}: no frames")
        dev = _device()
        row_floats, project_chunk = self._trajectory_projector(records, top.n_atoms, ANGSTROM_TO_NM, dev)
        chunk, ranges = frame_io.plan_chunks(n, 4 * (stride * traj.frame_stride + row_floats), frame_io.resolve_budget(memory_budget))
        logger.info(f"Projecting {n} frames of {Path(trajectory_path).name} onto {self.cv_name} in chunks of {chunk} frames")
        rows = np.empty((n, self.cv_dimension), dtype=np.float32)
        for lo, hi, buf, layout in frame_io.stream(traj, ranges, stride):
            block, finite = project_chunk(buf, layout)
            rows[lo:hi] = block.cpu().numpy()
            if not finite or not np.isfinite(rows[lo:hi]).all():
                raise ValueError(f"NaNs in the features of frames {lo * stride}..{(hi - 1) * stride} of {trajectory_path}: check the coordinates")
            del buf
        return pd.DataFrame(rows, columns=self.cv_labels)

    def _trajectory_projector(self, records: np.ndarray, n_atoms: int, unit: float, dev):
        """(device floats per frame beside the coordinates, f(buffer, layout) -> (device [m, d] projection of one chunk,
        False when a feature of the chunk was seen to be non-finite)) -- the per-model half of project_trajectory."""
        raise NotImplementedError

    def _trajectory_features(self, records: np.ndarray, n_atoms: int, unit: float, dev):
        """(columns of the device matrix, f(buffer, layout) -> (chunk x F view of it in label order, all finite)): hip.featurize
        of one chunk; a sine or cosine without its partner goes through a scratch pair of columns behind the features."""
        from . import trajectory

        F = self.num_features
        defs, n_columns, src, dst = trajectory.records_to_featurize_defs(records, F)
        src_d, dst_d = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)

        def features(buf, layout):
            wide = torch.empty(int(layout[0]), n_columns, dtype=torch.float32, device=dev)
            hip.featurize(buf, defs, n_atoms, strides=layout, unit=unit, out=wide)
            if len(src):
                wide[:, dst_d] = wide[:, src_d]
            X = wide[:, :F]
            return X, bool(torch.isfinite(X).all())

        return n_columns, features

    def set_labels(self):
        self.cv_labels = [f"{cv_components_map[self.cv_name]} {i + 1}" for i in range(self.cv_dimension)]

    def get_labels(self) -> List[str]:
        return self.cv_labels

    def get_cv_dimension(self) -> int:
        return self.cv_dimension

    def get_range(self) -> List[Tuple[float, float]]:
        return self.cv_range

    def write_plumed_files(self, topology: Optional[str], output_folder: str, waypoint_structures=None):
        """PLUMED input that tracks this CV (reference cv_calculator.py:545-681 -> ComputeCVBuilder).
        Without a topology the reference returns early (:569-571).  Written here: the header, the CV
        section exactly as the reference's assembler composes it (assembler.py:333-431 with
        command.combine / command.pytorch_model, command.py:357-420, 1149-1178) and the PRINT line
        (command.py:520-564, traj_stride 1), zipped as plumed_<cv>_unbiased.zip together with the
        TorchScript weights of a neural CV.  The MOLINFO / WHOLEMOLECULES / per-feature commands and
        the feature-name translation between topologies need MDAnalysis (out of scope): the feature
        labels are used as the PLUMED argument names, and the enhanced-sampling input is not built."""
        if topology is None:
            logger.warning("Topology not provided. Skipping PLUMED files creation.")
            return
        os.makedirs(output_folder, exist_ok=True)
        self.plumed_files = []
        if self.get_cv_type() == "non-linear":
            self.weights_path = os.path.join(output_folder, f"{self.cv_name}_weights.pt")
            self.save_weights(self.weights_path)
            self.plumed_files.append(self.weights_path)
        path = os.path.join(output_folder, f"plumed_input_{self.cv_name}.dat")
        text = "# PLUMED input file generated with Deep Cartograph\n"
        text += self.plumed_cv_lines()
        text += "\n" + plumed_print(self.plumed_cv_labels(), f"{self.cv_name}_out.dat", 1)
        with open(path, "w") as f:
            f.write(text)
        self.plumed_files.append(path)
        zip_files(os.path.join(output_folder, f"plumed_{self.cv_name}_unbiased.zip"), *self.plumed_files)
        remove_files(*self.plumed_files)

    def plumed_cv_lines(self) -> str:
        raise NotImplementedError

    def plumed_cv_labels(self) -> List[str]:
        raise NotImplementedError


def plumed_combine(label: str, arguments, coefficients=None, parameters=None, periodic: bool = False) -> str:
    """PLUMED COMBINE line in the reference's format (command.py:357-420): %.17g coefficients / parameters."""
    line = label + ": COMBINE ARG=" + ",".join(arguments)
    if coefficients is not None:
        line += " COEFFICIENTS=" + ",".join(f"{c:.17g}" for c in coefficients)
    if parameters is not None:
        line += " PARAMETERS=" + ",".join(f"{a:.17g}" for a in parameters)
    return line + (" PERIODIC=YES" if periodic else " PERIODIC=NO") + "\n"


def plumed_print(arguments, file_path: str, stride: int = 1, fmt: str = "%.4f") -> str:
    """PLUMED PRINT line in the reference's format (command.py:520-564)."""
    return "PRINT ARG=" + ",".join(arguments) + " FILE=" + file_path + " STRIDE=" + str(stride) + f" FMT={fmt}\n"


# ======================================================================================= linear
class LinearCalculator(CVCalculator):
    """Linear CVs: weights F x d (reference :749-1047)."""

    def __init__(self, configuration: Optional[Dict] = None, output_path: Optional[str] = None):
        super().__init__(configuration, output_path)
        self.cv: Optional[np.ndarray] = None
        self.weights_path: Optional[str] = None
        self.cv_stats: Dict[str, np.ndarray] = {}
        self.cv_norm_mean: Optional[np.ndarray] = None
        self.cv_norm_range: Optional[np.ndarray] = None

    def _load_from_folder(self, folder_path: str):
        super()._load_from_folder(folder_path)
        f = self.model_output_folder
        self.cv = np.load(os.path.join(f, "cv_weights.npy"))
        self.cv_norm_mean = np.load(os.path.join(f, "cv_norm_mean.npy"))
        self.cv_norm_range = np.load(os.path.join(f, "cv_norm_range.npy"))
        self.features_norm_mean = np.load(os.path.join(f, "features_norm_mean.npy"))
        self.features_norm_range = np.load(os.path.join(f, "features_norm_range.npy"))

    def set_training_matrix(self, X, feature_names=None, labels=None):
        super().set_training_matrix(X, feature_names, labels)
        # linear models normalise the stored training matrix in place (reference :800-804)
        dev = self.training_data.device
        hip.normalize(self.training_data, _dev(self.features_norm_mean, dev), _dev(self.features_norm_range, dev),
                      out=self.training_data)

    def normalize_data(self, data: torch.Tensor, normalizing_mean, normalizing_range) -> torch.Tensor:
        """(data - mean) / range in float32 on the GPU (in place, as the reference)."""
        dev = _device()
        d = data if data.is_cuda else data.to(dev)
        return hip.normalize(d, _dev(normalizing_mean, dev), _dev(normalizing_range, dev), out=d)

    def save_weights(self, weights_path: str):
        np.save(weights_path, self.cv)

    def save_model(self):
        super().save_model()
        if self.cv is None:
            raise ValueError("No Linear CV weights to save. Please compute the CV before saving the model.")
        f = self.model_output_folder
        self.save_weights(os.path.join(f, "cv_weights.npy"))
        if self.cv_norm_mean is None or self.cv_norm_range is None:
            raise ValueError("CV normalization parameters have not been computed. Cannot save model.")
        np.save(os.path.join(f, "cv_norm_mean.npy"), self.cv_norm_mean)
        np.save(os.path.join(f, "cv_norm_range.npy"), self.cv_norm_range)
        np.save(os.path.join(f, "features_norm_mean.npy"), self.features_norm_mean)
        np.save(os.path.join(f, "features_norm_range.npy"), self.features_norm_range)
        model_path = os.path.join(self.output_path, "model.zip")
        zip_files(model_path, str(f))
        shutil.rmtree(f)
        logger.info(f"Model saved to {model_path}")

    def get_cv_parameters(self):
        return {"cv_name": self.cv_name, "cv_dimension": self.cv_dimension, "features_norm_mode": self.feats_norm_mode,
                "features_norm_mean": self.features_norm_mean, "features_norm_range": self.features_norm_range,
                "cv_stats": self.cv_stats, "weights": self.cv}

    def get_cv_type(self) -> str:
        return "linear"

    def _weights_dev(self, dev):
        return _dev(np.ascontiguousarray(self.cv, dtype=np.float32), dev)

    def project_data(self, data, normalize_data: bool = True) -> torch.Tensor:
        """((x - fmean)/frange) @ W, then (. - cv_mean)/cv_range -- one HBM-bound HIP pass
        (reference :918-972).  Returns a CPU tensor; the caller's data is left untouched."""
        if self.cv is None:
            raise ValueError("CV has not been computed. Cannot project data.")
        if self.cv_norm_mean is None or self.cv_norm_range is None:
            raise ValueError("CV normalization parameters have not been computed. Cannot normalize projected data.")
        dev = _device()
        X = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.asarray(data, dtype=np.float32))
        X = X.to(device=dev, dtype=torch.float32).contiguous()
        kw = {}
        if normalize_data:
            if self.features_norm_mean is None or self.features_norm_range is None:
                raise ValueError("Feature normalization parameters have not been computed. Cannot normalize data.")
            kw = dict(fmean=_dev(self.features_norm_mean, dev), frange=_dev(self.features_norm_range, dev))
        out, _ = hip.project_linear(X, self._weights_dev(dev), cvmean=_dev(self.cv_norm_mean, dev),
                                    cvrange=_dev(self.cv_norm_range, dev), **kw)
        return _to_host(out)

    # project_trajectory's path: "two_step" = hip.featurize into a chunk x F matrix, then hip.project_linear; "fused" = one
    # hip.featurize_project launch per chunk, no matrix (float64 accumulation, a chunk costs d instead of F + d floats per
    # frame).  At 762 features the two launches measured 0.85 - 0.90 of the fused one's time, hence the default.
    trajectory_path: str = "two_step"

    def _trajectory_projector(self, records, n_atoms, unit, dev):
        if self.cv_norm_mean is None or self.cv_norm_range is None:
            raise ValueError("CV normalization parameters have not been computed. Cannot normalize projected data.")
        if self.trajectory_path not in ("two_step", "fused"):
            raise ValueError(f"trajectory_path '{self.trajectory_path}' not recognized (two_step, fused)")
        W = self._weights_dev(dev)
        kw = dict(cvmean=_dev(self.cv_norm_mean, dev), cvrange=_dev(self.cv_norm_range, dev))
        if self.features_norm_mean is not None and self.features_norm_range is not None:
            kw.update(fmean=_dev(self.features_norm_mean, dev), frange=_dev(self.features_norm_range, dev))
        if self.trajectory_path == "fused":   # a non-finite feature shows in its output row
            return W.shape[1], lambda buf, layout: (hip.featurize_project(buf, records, n_atoms, self.num_features, W, strides=layout,
                                                                          unit=unit, **kw)[0], True)
        n_columns, features = self._trajectory_features(records, n_atoms, unit, dev)

        def project_chunk(buf, layout):
            X, finite = features(buf, layout)
            return hip.project_linear(X, W, **kw)[0], finite

        return n_columns + W.shape[1], project_chunk

    def normalize_cv(self):
        """min / max of Xn @ W over all training frames -> [-1, 1] (reference :974-991)."""
        if self.training_data is None:
            raise ValueError("Training data not loaded. Cannot compute CV statistics for normalization.")
        _, mm = hip.project_linear(self.training_data, self._weights_dev(self.training_data.device), want_out=False, want_minmax=True)
        mm = reduce_minmax(mm, self.comm).cpu().numpy()
        self.cv_stats = {"min": mm[0], "max": mm[1]}
        self.cv_norm_mean = (mm[1] + mm[0]) / 2
        self.cv_norm_range = (mm[1] - mm[0]) / 2
        self.cv_range = [(-1.0, 1.0)] * self.cv_dimension

    def sensitivity_analysis(self):
        """|W| per feature, ascending, one CSV per CV dimension (reference :993-1047, without
        the plots and the per-atom mapping, which need matplotlib / MDAnalysis)."""
        if self.comm.rank != 0:
            return
        sens = np.abs(self.cv)
        for i in range(sens.shape[1]):
            out = Path(self.sensitivity_output_folder) / f"sensitivity_analysis_{i + 1}"
            out.mkdir(parents=True, exist_ok=True)
            order = np.argsort(sens[:, i])
            pd.DataFrame({"sensitivity": sens[order, i]}, index=list(np.array(self.features_ref_labels)[order])).to_csv(
                out / "sensitivity_analysis.csv")

    # covariance blocks of the (normalised) training matrix, global over ranks
    def _covariances(self, lag: int):
        X = self.training_data
        n_local, F = X.shape
        dev = X.device
        # z = xn - shift with shift ~ column mean of xn keeps the fp32 products well conditioned
        shift = (self.features_stats["mean"].astype(np.float64) - np.asarray(self.features_norm_mean, dtype=np.float64)) / \
            np.asarray(self.features_norm_range, dtype=np.float64)
        # always passed, even when the standardisation already centred the columns (shift ~ 0): with a shift the kernel
        # knows its operand is centred and takes the column sums of z_t from its own fragments (cov.hip), no extra pass
        shift_t = _dev(shift.astype(np.float32), dev)
        Xh, n_pairs_local = append_halo(X, lag, self.comm)
        if n_pairs_local <= 0:
            raise ValueError("not enough frames for the requested lag time")
        raw = self.comm.sum_(hip.lagged_cov_raw(Xh, n_pairs_local, lag, shift_t))
        n_pairs = int(round(self.comm.sum_scalar(n_pairs_local, device=dev)))
        delta, C0, Ct = hip.covariances_from_raw(raw.cpu().numpy(), n_pairs, F)
        return delta, C0, Ct, n_pairs

    def plumed_cv_lines(self) -> str:
        """The linear CV section of the reference's assembler (assembler.py:333-381): one COMBINE per
        normalised feature, one per CV component over them, one per min-max normalised component."""
        text = ""
        feats = list(self.features_ref_labels)
        if self.feats_norm_mode is not None:
            text += "\n# Normalized features\n"
            normalized = []
            for i, feat in enumerate(feats):
                text += plumed_combine(f"feat_{i}", [feat], [1 / self.features_norm_range[i]], [self.features_norm_mean[i]])
                normalized.append(f"feat_{i}")
        else:
            normalized = feats
        text += "\n# Collective variable\n"
        for i in range(self.cv.shape[1]):
            text += plumed_combine(f"{self.cv_name}_{i}", normalized, self.cv[:, i])
        # reference assembler.py:367-370: offset = (min + max) / 2, scale = 2 / (max - min) from cv_stats, in the float32 of
        # the pandas min / max they come from (the '%.17g' text shows every bit); a model loaded from model.zip carries
        # the same two numbers as cv_norm_mean / cv_norm_range
        if self.cv_stats:
            cmin, cmax = np.asarray(self.cv_stats["min"], dtype=np.float32), np.asarray(self.cv_stats["max"], dtype=np.float32)
        else:
            cmin = np.asarray(self.cv_norm_mean, dtype=np.float32) - np.asarray(self.cv_norm_range, dtype=np.float32)
            cmax = np.asarray(self.cv_norm_mean, dtype=np.float32) + np.asarray(self.cv_norm_range, dtype=np.float32)
        offset = (cmin + cmax) / 2
        scale = 2 / (cmax - cmin)
        text += "\n# Normalized Collective variable\n"
        for i in range(self.cv.shape[1]):
            text += plumed_combine(f"norm_{self.cv_name}_{i}", [f"{self.cv_name}_{i}"], [scale[i]], [offset[i]])
        return text

    def plumed_cv_labels(self) -> List[str]:
        return [f"norm_{self.cv_name}_{i}" for i in range(self.cv.shape[1])]


class PCACalculator(LinearCalculator):
    """Principal component analysis (reference :2174-2215): eigenvectors of the covariance of
    the normalised features, covariance accumulated by the FP32-MFMA kernel."""

    def __init__(self, configuration: Optional[Dict] = None, output_path: Optional[str] = None):
        super().__init__(configuration, output_path)
        self.cv_name = "pca"

    def compute_cv(self):
        if self.training_data is None:
            logger.error("No training data available to compute PCA.")
            return
        _, C0, _, _ = self._covariances(lag=0)
        self.cv = linalg.pca_components(C0, self.cv_dimension).astype(np.float32)


class TICACalculator(LinearCalculator):
    """Time-lagged independent component analysis (reference :2217-2267)."""

    def __init__(self, configuration: Optional[Dict] = None, output_path: Optional[str] = None):
        super().__init__(configuration, output_path)
        self.cv_name = "tica"
        self.tica_eigenvalues: Optional[np.ndarray] = None

    def compute_cv(self):
        try:
            _, C0, Ct, _ = self._covariances(lag=int(self.configuration.get("lag_time")))
            evals, evecs = linalg.tica_eigh(C0, Ct, reg=1e-6, n_eig=min(self.cv_dimension, C0.shape[0]))
        except Exception as e:  # the reference logs and skips the CV (:2259-2264)
            logger.error(f"TICA could not be computed. Error message: {e}")
            return
        self.tica_eigenvalues = evals
        self.cv = evecs.astype(np.float32)


class HTICACalculator(LinearCalculator):
    """Hierarchical TICA (reference :2269-2384).  The level-1 covariances are the diagonal blocks
    of the global C0 / Ctau and the level-2 ones are T^T C0 T, T^T Ctau T with
    T = block_diag(level-1 eigenvectors): one data pass in total."""

    def __init__(self, configuration: Optional[Dict] = None, output_path: Optional[str] = None):
        super().__init__(configuration, output_path)
        self.cv_name = "htica"
        self.num_subspaces = self.configuration.get("num_subspaces")
        self.subspaces_dimension = self.configuration.get("subspaces_dimension")

    def compute_cv(self):
        F = self.num_features
        split = F // self.num_subspaces
        if split == 0:
            logger.error(f"Number of subspaces {self.num_subspaces} is larger than number of features {F}. Exiting...")
            return
        try:
            _, C0, Ct, _ = self._covariances(lag=int(self.configuration.get("lag_time")))
            level1 = []
            for a in range(0, F, split):  # torch.split semantics: last chunk may be narrower
                b = min(F, a + split)
                _, ev = linalg.tica_eigh(C0[a:b, a:b], Ct[a:b, a:b], reg=1e-6, n_eig=min(self.subspaces_dimension, b - a))
                level1.append(ev)
            T = linalg.block_diag(level1)
            C0_2 = T.T @ C0 @ T
            Ct_2 = T.T @ Ct @ T
            _, ev2 = linalg.tica_eigh(C0_2, Ct_2, reg=1e-6, n_eig=min(self.cv_dimension, T.shape[1]))
        except Exception as e:
            logger.error(f"TICA could not be computed. Error message: {e}")
            return
        self.cv = (T @ ev2).astype(np.float32)


# ======================================================================================= neural
# torch.optim defaults of the optimisers the HIP engine implements (torch 2.x signatures)
_OPTIMIZERS = {
    "Adam": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, decoupled_weight_decay=False),
    "AdamW": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False),
    "SGD": dict(lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False),
    "RMSprop": dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False),
    "Adagrad": dict(lr=1e-2, lr_decay=0.0, weight_decay=0.0, initial_accumulator_value=0.0, eps=1e-10),
    "Adamax": dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    "NAdam": dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum_decay=4e-3, decoupled_weight_decay=False),
    "RAdam": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False),
    "Adadelta": dict(lr=1.0, rho=0.9, eps=1e-6, weight_decay=0.0),
    "ASGD": dict(lr=1e-2, lambd=1e-4, alpha=0.75, t0=1e6, weight_decay=0.0),
    "Rprop": dict(lr=1e-2, etas=(0.5, 1.2), step_sizes=(1e-6, 50.0)),
}
# torch.optim classes the reference's `getattr(torch.optim, name)` would also accept and the engine does not run:
# LBFGS re-evaluates the loss through a closure several times per step (not a per-element update), SparseAdam rejects
# the dense gradients of these models inside torch itself (the reference's try fails there too)
_OPTIMIZERS_REFUSED = {"LBFGS": "needs a closure that re-evaluates the model several times per step",
                       "SparseAdam": "torch.optim.SparseAdam does not support dense gradients (the reference's try fails as well)",
                       "Adafactor": "not part of the reference's pinned torch 2.1.2 (environment_detailed.yml): its getattr fails there",
                       "Muon": "not part of the reference's pinned torch 2.1.2 (environment_detailed.yml): its getattr fails there"}
_IMPLEMENTATION_SWITCHES = ("foreach", "fused", "capturable", "differentiable")   # no effect on the arithmetic


class NonLinear(CVCalculator):
    """Neural CVs trained by the HIP MLP engine (reference :1049-1921)."""

    model_kind: str = ""

    def __init__(self, configuration: Optional[Dict] = None, output_path: Optional[str] = None):
        super().__init__(configuration, output_path)
        self.training_config: Dict = self.configuration.get("training", {})
        g = self.training_config.get("general", {})
        es = self.training_config.get("early_stopping", {})
        self.optimizer_config: Dict = self.training_config.get("optimizer", {}) or {}
        self.lr_scheduler: Optional[Dict] = self.training_config.get("lr_scheduler", None) or None
        self.lr_scheduler_config: Dict = dict(self.training_config.get("lr_scheduler_config", None) or {})
        self.model_to_save = self.training_config.get("model_to_save", "best")
        self.num_tries: int = g.get("num_tries", 10)
        self.seed: int = g.get("seed", 42)
        self.training_validation_lengths: List = g.get("lengths", [0.8, 0.2])
        self.batch_size: int = g.get("batch_size", 32)
        self.shuffle: bool = g.get("shuffle", True)
        self.random_split: bool = g.get("random_split", True)
        self.max_epochs: int = g.get("max_epochs", 100)
        self.check_val_every_n_epoch: int = g.get("check_val_every_n_epoch", 1)
        self.save_check_every_n_epoch: int = g.get("save_check_every_n_epoch", 5)
        self.early_stop_patience: int = es.get("patience", 20)
        self.early_stop_delta: float = es.get("min_delta", 1e-5)
        self.encoder_config: Dict = copy.deepcopy(self.architecture_config.get("encoder", {}) or {})
        dec = self.architecture_config.get("decoder", {})
        self.decoder_config: Optional[Dict] = copy.deepcopy(dec) if dec is not None else None
        self.encoder_hidden_layers: List[int] = list(self.encoder_config.get("layers", []))
        self.decoder_hidden_layers: List[int] = list((self.decoder_config or self.encoder_config).get("layers", []))
        self.num_training_samples: Optional[int] = None
        self.num_validation_samples: Optional[int] = None
        self.cv_score: Optional[float] = None
        self.tries: int = 0
        self.metrics: Optional[Dict[str, list]] = None
        self.training_metrics_paths: List[str] = []
        self.weights_path: Optional[str] = None
        self.engine: Optional[hip.Mlp] = None
        self.training_normalized: Optional[torch.Tensor] = None    # norm_in applied once (device)
        self.validation_normalized: Optional[torch.Tensor] = None

    # ---- configuration -> layer lists (reference :1155-1219)
    @staticmethod
    def _fit_list(values, n_hidden: int, what: str):
        """One entry per hidden layer.  mlcolvar's FeedForward insists on exactly n entries per option and raises
        otherwise -- which is what the schema's 3-entry defaults do to any `layers` list that is not 3 long
        (the reference's shipped default_config.yml: layers [15, 15], no activation given).  Here a list that is
        too long is cut and one that is too short repeats its last entry, with a warning."""
        values = list(values)
        if len(values) != n_hidden:
            logger.warning(f"'{what}' has {len(values)} entries for {n_hidden} hidden layers; adjusting it.")
            values = (values + [values[-1] if values else None] * n_hidden)[:n_hidden]
        return values

    @classmethod
    def _layer_options(cls, cfg: Dict, n_hidden: int):
        """(activation, dropout, batchnorm) with one entry per Linear: the hidden layers' lists plus the
        last-layer entries, as set_up_encoder_last_layer / set_up_decoder_last_layer append them."""
        act = cls._fit_list(cfg.get("activation", ["leaky_relu"] * n_hidden), n_hidden, "activation")
        drop = cls._fit_list(cfg.get("dropout", [None] * n_hidden), n_hidden, "dropout")
        bn = cls._fit_list(cfg.get("batchnorm", [False] * n_hidden), n_hidden, "batchnorm")
        act.append(cfg.get("last_layer_activation", None))
        drop.append(cfg.get("last_layer_dropout", None))
        bn.append(cfg.get("last_layer_batchnorm", False))
        drop = [float(d) if d else 0.0 for d in drop]
        if any(d < 0.0 or d >= 1.0 for d in drop):
            raise ValueError("dropout probabilities must lie in [0, 1)")
        return act, drop, [bool(b) for b in bn]

    def _optimizer_options(self) -> Tuple[str, Dict]:
        """(torch.optim class name, its keyword arguments with torch's defaults filled in) -- reference :1376-1380."""
        name = self.optimizer_config.get("name", "Adam")
        if name not in _OPTIMIZERS:
            if not hasattr(torch.optim, name):
                raise ValueError(f"Optimizer {name} not recognized.")
            why = _OPTIMIZERS_REFUSED.get(name, "")
            raise NotImplementedError(f"optimizer {name} is not implemented by the HIP engine{': ' + why if why else ''} (have: {sorted(_OPTIMIZERS)})")
        kw = dict(_OPTIMIZERS[name])
        for k, v in (self.optimizer_config.get("kwargs", {}) or {}).items():
            if k in _IMPLEMENTATION_SWITCHES:
                continue
            if k == "maximize":   # every torch.optim class takes it: the update uses the negated gradient
                kw["maximize"] = bool(v)
                continue
            if k not in kw:
                raise TypeError(f"{name}.__init__() got an unexpected keyword argument '{k}'")
            kw[k] = v
        return name, kw

    @staticmethod
    def _engine_optimizer_kwargs(name: str, kw: Dict) -> Dict:
        if name == "Adam" and kw.get("decoupled_weight_decay"):   # newer torch: Adam(decoupled_weight_decay=True) is AdamW's update
            name = "AdamW"
        out = dict(optimizer=name, lr=float(kw["lr"]), weight_decay=float(kw.get("weight_decay", 0.0)))
        if "betas" in kw:
            out["betas"] = (float(kw["betas"][0]), float(kw["betas"][1]))
        for k in ("eps", "momentum", "dampening", "alpha", "lr_decay", "initial_accumulator_value"):
            if k in kw:
                out[k] = float(kw[k])
        for k in ("amsgrad", "nesterov", "centered", "maximize"):
            if k in kw:
                out[k] = bool(kw[k])
        # further constants, in the order of dcv.h's DCV_OPT_* comments
        extra = {"NAdam": [kw.get("momentum_decay", 4e-3), 1.0 if kw.get("decoupled_weight_decay") else 0.0],
                 "RAdam": [0.0, 1.0 if kw.get("decoupled_weight_decay") else 0.0],
                 "Adadelta": [kw.get("rho", 0.9)],
                 "ASGD": [kw.get("lambd", 1e-4), kw.get("alpha", 0.75), kw.get("t0", 1e6)],
                 "Rprop": list(kw.get("etas", (0.5, 1.2))) + list(kw.get("step_sizes", (1e-6, 50.0)))}.get(name)
        if extra is not None:
            out["opt_params"] = [float(v) for v in extra]
        if name == "ASGD":
            out.pop("alpha", None)   # ASGD's alpha is the eta exponent (opt_params), not RMSprop's smoothing constant
        return out

    def _scheduler_options(self, steps_per_epoch: int) -> Optional[Tuple[str, Dict, Dict]]:
        """(name, kwargs, lr_scheduler_config) after adjust_lr_scheduler (reference :1228-1273)."""
        if self.lr_scheduler is None:
            return None
        name = self.lr_scheduler.get("name", "")
        kwargs = dict(self.lr_scheduler.get("kwargs", {}) or {})
        config = dict(self.lr_scheduler_config)
        if name == "OneCycleLR":
            kwargs.setdefault("max_lr", 1e-3)
            kwargs.setdefault("epochs", self.max_epochs)
            kwargs.setdefault("steps_per_epoch", steps_per_epoch)
            config["interval"] = "step"
        elif name == "ReduceLROnPlateau":
            kwargs.setdefault("patience", self.early_stop_patience // 4)
            kwargs.setdefault("cooldown", self.early_stop_patience // 8)
            config["interval"] = "epoch"
        return name, kwargs, config

    # ---- data
    def _norm_tensors(self, dev):
        return _dev(self.features_norm_mean, dev), _dev(self.features_norm_range, dev)

    def set_training_matrix(self, X, feature_names=None, labels=None):
        super().set_training_matrix(X, feature_names, labels)
        dev = self.training_data.device
        # norm_in of the model, applied once: (x - mean)/range is elementwise, so the values are
        # bit-identical to applying it inside the forward pass (reference :1366-1374)
        self.training_normalized = hip.normalize(self.training_data, *self._norm_tensors(dev))
        if self.validation_data is not None:
            self.validation_normalized = hip.normalize(self.validation_data, *self._norm_tensors(dev))

    def set_validation_matrix(self, X):
        super().set_validation_matrix(X)
        if self.features_norm_mean is not None:   # the training statistics normalise the validation frames too
            self.validation_normalized = hip.normalize(self.validation_data, *self._norm_tensors(self.validation_data.device))

    # ---- model description, implemented by the subclasses
    def layer_plan(self) -> Tuple[List[int], List[Optional[str]], List[float], List[bool], int]:
        """(dims, activation / dropout / batch-norm flag per Linear, index of the latent layer)."""
        raise NotImplementedError

    def n_samples_local(self) -> int:
        return self.training_data.shape[0]

    def n_val_samples_local(self) -> int:
        return self.validation_data.shape[0]

    def _decoder_options(self):
        """_layer_options of the decoder, its last activation made to cover the range of the normalised features
        (reference :1188-1207)."""
        dec_cfg = self.decoder_config if self.decoder_config is not None else self.encoder_config
        dec_act, dec_drop, dec_bn = self._layer_options(dec_cfg, len(self.decoder_hidden_layers))
        for mode, act, text in (("min_max_range1", "custom_sigmoid", "[0, 1]. Changing the activation function to 'sigmoid'."),
                                ("min_max_range2", "tanh", "[-1, 1]. Changing the activation function to 'tanh'.")):
            if self.feats_norm_mode == mode and dec_act[-1] != act:
                logger.warning(f"The last layer activation function of the decoder is set to {dec_act[-1]}, but the features are "
                               f"normalized using min max with range {text}")
                dec_act[-1] = act
        if dec_drop[-1]:
            logger.warning("Dropout in the last layer of the decoder is not recommended.")
        return dec_act, dec_drop, dec_bn

    def lag(self) -> int:
        return 0

    def check_num_samples(self):
        """reference :1278-1295: counted in FRAMES (len(self.training_data)), also for time-lagged pairs."""
        if self.validation_data is not None:
            self.num_training_samples = self.num_frames_global
            self.num_validation_samples = int(round(self.comm.sum_scalar(self.validation_data.shape[0], device=self.validation_data.device)))
        else:
            self.num_training_samples = int(self.num_frames_global * self.training_validation_lengths[0])
            self.num_validation_samples = self.num_frames_global - self.num_training_samples
        logger.info(f"Number of training samples: {self.num_training_samples}")
        logger.info(f"Number of validation samples: {self.num_validation_samples}")

    def check_batch_size(self) -> int:
        """batch >= number of training samples -> the power of two below it (reference :1297-1309)."""
        if self.batch_size >= self.num_training_samples:
            self.batch_size = closest_power_of_two(self.num_training_samples)
            logger.warning(f"The batch size is larger than the number of samples in the training set. "
                           f"Setting the batch size to the closest power of two: {self.batch_size}")
        return self.batch_size

    def _init_linears(self, dims):
        """torch.nn.Linear default initialisation in construction order, consuming the global
        RNG exactly as create_model() does."""
        lins = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]
        return [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in lins]

    def _records_to_metrics(self, rec: np.ndarray, need_eig: bool = True):
        """(weighted mean loss, weighted mean eigenvalues or None, TICA buffers of the last record)."""
        w = rec[:, 1]
        loss = float((rec[:, 0] * w).sum() / w.sum())
        return loss, None, None

    def train(self) -> bool:
        """Multi-try training driver (reference :1456-1553): seed + try, split, model init,
        epochs with validation, early stopping, best / last snapshot; lowest score wins.  As there, a try
        that raises is logged and the next one runs; no valid try -> False (the CV is skipped)."""
        logger.info(f"Training {cv_names_map[self.cv_name]} ...")
        dev = self.training_data.device
        try:
            model, optimizer = self.layer_plan(), self._optimizer_options()
        except Exception as e:
            logger.error(f"{cv_names_map[self.cv_name]} cannot be set up: {e}")
            return False
        separate_val = self.validation_data is not None
        if separate_val and self.validation_normalized is None:
            self.validation_normalized = hip.normalize(self.validation_data, *self._norm_tensors(dev))
        n_local = self.n_samples_local()
        n_val_local = self.n_val_samples_local() if separate_val else 0
        if self.comm.active:  # identical batch plans on every rank: use the smallest shard size
            n_local = int(self.comm.min_(torch.tensor([n_local], dtype=torch.int64, device=dev)).item())
            n_val_local = int(self.comm.min_(torch.tensor([n_val_local], dtype=torch.int64, device=dev)).item())
        if n_local < 1 or (separate_val and n_val_local < 1):
            logger.error("Not enough samples to train on.")
            return False
        self.check_num_samples()
        self.check_batch_size()
        plan = FitPlan(*model, *optimizer, n_local, n_val_local, max(1, self.batch_size // self.comm.world) if self.batch_size > 0 else 0)
        best = None
        for try_num in range(1, self.num_tries + 1):
            self.tries = try_num
            try:
                # The host side of a try is small torch-CPU work (a randperm and a gather per epoch, the initialisation of a few
                # Linears): with the 128 intra-op threads of a GPU host torch.randperm takes 15 ms for 160 000 indices against
                # 1.3 ms with 8 (its result does not depend on the count: tests/test_host_cpu.py).  Capped once per try --
                # growing the pool back costs ~12 ms, so not per epoch.
                with _torch_threads(8):
                    result = Try(self, plan, try_num).run()
            except Exception as e:
                logger.error(f"Training try {try_num} failed with an exception: {e}")
                continue
            if result is None:
                continue
            logger.info(f"Try {try_num}/{self.num_tries}: score = {result['score']:.5f}")
            if best is None or result["score"] < best["score"]:
                best = result
                logger.info(f"  -> New best model (try {try_num}).")
        if best is None:
            logger.error(f"{cv_names_map[self.cv_name]} did not produce a valid model after {self.num_tries} tries.")
            return False
        self.cv = best["state"]
        self.cv_score = best["score"]
        self.metrics = best["metrics"]
        self.cv["norm_in"] = (self.features_norm_mean, self.features_norm_range)
        self.engine.set_linears(self.cv["linears"], bn=self.cv.get("bn"))
        logger.info(f"Best model score across {self.num_tries} tries: {best['score']:.5f}")
        return True

    # ---- per-model hooks of the epoch loop (the VAE's noise, beta and post-annealing checkpoint; no-ops here)
    def _fit_begin(self, sched, n_val: int, bs: int):
        """Before the first epoch (after the model and the split exist)."""

    def _epoch_begin(self, epoch: int, tb, make_val_batches):
        """Start of an epoch: the training batches exist; returns the validation batches (make_val_batches())."""
        return make_val_batches()

    def _on_validation(self, epoch: int, rec_train: np.ndarray, rec_val: np.ndarray, metrics: Dict, snapshot):
        """After every validation pass (its losses are the last entries of `metrics`); snapshot() returns the current model state."""

    def _choose_model(self, best_state, best_score, last_state, metrics):
        """_finalize_training (reference :1555-1642): "best" = the checkpoint with the lowest monitored loss and that loss;
        "last" = the last checkpoint written, scored with the FINAL validation loss of the run.  (state, score) or None."""
        if self.model_to_save == "best" and best_state is not None:
            return best_state, best_score
        if last_state is not None:
            return last_state, metrics["valid_loss"][-1]
        return None

    def compute_cv(self):
        if self.train():
            if self.comm.rank == 0:
                self.plot_training_metrics()

    metric_files: Tuple[str, ...] = ("train_loss", "valid_loss", "epoch")

    def plot_training_metrics(self):
        """The metrics named by metric_files as .npy -> training_metrics.zip, model_score.txt, eigenvalues.txt (Deep-TICA)
        (reference :1658-1733, 2592-2627; the VAE's: :2880-2893; no figures)."""
        if not self.training_config.get("save_loss", True) or self.metrics is None:
            return
        paths = []
        for key in self.metric_files:
            if key not in self.metrics:   # (only the VAE names metrics that a fit may not have)
                if key == "lr":
                    logger.warning(f"Metric {key} not found in metrics. It will not be saved.")
                continue
            p = os.path.join(self.training_output_folder, f"{key}.npy")
            np.save(p, np.array(self.metrics[key]))
            paths.append(p)
        np.savetxt(os.path.join(self.training_output_folder, "model_score.txt"), np.array([self.cv_score]), fmt="%.7g")
        if "valid_eigval_1" in self.metrics and self.cv_score in self.metrics["valid_loss"]:
            bi = self.metrics["valid_loss"].index(self.cv_score)
            ev = [self.metrics[f"valid_eigval_{i + 1}"][bi] for i in range(self.cv_dimension)]
            np.savetxt(os.path.join(self.training_output_folder, "eigenvalues.txt"), np.array(ev), fmt="%.7g")
        zip_files(os.path.join(self.training_output_folder, "training_metrics.zip"), *paths)
        remove_files(*paths)

    # ---- projection
    def _infer(self, Xn: torch.Tensor, with_post: bool, want_out=True, want_minmax=False):
        st = self.cv
        dev = Xn.device
        kw = {}
        if st.get("tica") is not None:
            kw.update(tmean=_dev(st["tica"][0], dev), tevecs=_dev(np.ascontiguousarray(st["tica"][1]), dev))
        if with_post and st.get("post") is not None:
            kw.update(pmean=_dev(st["post"][0], dev), prange=_dev(st["post"][1], dev))
        return self.engine.infer(Xn, want_out=want_out, want_minmax=want_minmax, **kw)

    def normalize_cv(self):
        """min / max of the raw CV over the training samples -> Normalization(mode='min_max') as
        postprocessing (reference :1735-1754)."""
        rows = self.n_samples_local()
        _, mm = self._infer(self.training_normalized[:rows], with_post=False, want_out=False, want_minmax=True)
        mm = reduce_minmax(mm, self.comm).cpu().numpy()
        self.cv["post"] = ((mm[1] + mm[0]) / 2.0, (mm[1] - mm[0]) / 2.0)
        self.cv_range = [(-1.0, 1.0)] * self.cv_dimension

    def project_data(self, data, normalize_data: bool = True) -> torch.Tensor:
        """model(x) for every row (reference :1842-1891).  norm_in is part of the model, so
        `normalize_data` is ignored as in the reference."""
        if self.cv is None:
            raise ValueError("No collective variable model to project data.")
        logger.info(f"Projecting data onto {cv_names_map[self.cv_name]} ...")
        dev = _device()
        if data is self.training_data and self.training_normalized is not None:
            Xn = self.training_normalized
        else:
            X = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.asarray(data, dtype=np.float32))
            X = X.to(device=dev, dtype=torch.float32).contiguous()
            if self.cv.get("norm_in") is not None:
                Xn = hip.normalize(X, _dev(self.cv["norm_in"][0], dev), _dev(self.cv["norm_in"][1], dev))
            else:
                Xn = X
        out, _ = self._infer(Xn, with_post=True)
        return _to_host(out)

    def _trajectory_projector(self, records, n_atoms, unit, dev):
        """The device-resident chunk x F matrix of _trajectory_features, then the normalisation and infer launches of
        project_data."""
        n_columns, features = self._trajectory_features(records, n_atoms, unit, dev)
        norm = None if self.cv.get("norm_in") is None else (_dev(self.cv["norm_in"][0], dev), _dev(self.cv["norm_in"][1], dev))

        def project_chunk(buf, layout):
            X, finite = features(buf, layout)
            Xn = hip.normalize(X, *norm) if norm is not None else X.contiguous()
            return self._infer(Xn, with_post=True)[0], finite

        return n_columns + self.num_features + self.cv_dimension, project_chunk

    # ---- sensitivity
    def summed_cv_gradient(self) -> np.ndarray:
        """d(sum_j cv_j)/d(network output): the layers behind the network are affine, so this is one
        vector for every frame.  y = (h - tmean) @ evecs (Deep-TICA), cv = (y - pmean) / prange."""
        st = self.cv
        d_lat = st["dims"][st["latent"]]
        inv_range = np.ones(self.cv_dimension if st.get("tica") is not None else d_lat, dtype=np.float64)
        if st.get("post") is not None:
            inv_range = 1.0 / np.asarray(st["post"][1], dtype=np.float64)
        if st.get("tica") is not None:
            return np.asarray(st["tica"][1], dtype=np.float64) @ inv_range
        return inv_range

    def sensitivity_scores(self) -> np.ndarray:
        """mlcolvar.explain.sensitivity_analysis(model, dataset, metric='mean_abs_val') restated
        (reference call site :1903): s_i = mean_r |d(sum_j cv_j)/dx_i(x_r)| * std_i over the samples
        of dataset['data'] (x_t rows for Deep-TICA), normalised to sum to one.  The model takes raw
        features (norm_in is its first layer), so d/dx_i = d/dxn_i / norm_range_i.  One input-gradient
        pass of the HIP engine over the resident normalised matrix."""
        rows = self.n_samples_local()
        dev = self.training_normalized.device
        raw = hip.col_stats_raw(self.training_data[:rows] if self.training_data.is_cuda else self.training_data[:rows].to(dev))
        n_glob = int(self.comm.sum_scalar(float(rows), device=dev))
        std = hip.finalize_stats(reduce_col_stats(raw, self.comm), n_glob)["std"].astype(np.float64)
        scale = std.copy()
        if self.cv.get("norm_in") is not None:
            scale = scale / np.asarray(self.cv["norm_in"][1], dtype=np.float64)
        g = self.summed_cv_gradient()
        acc = self.engine.input_sensitivity(self.training_normalized[:rows], _dev(g.astype(np.float32), dev), _dev(scale.astype(np.float32), dev))
        acc = self.comm.sum_(acc).cpu().numpy() if self.comm.active else acc.cpu().numpy()
        score = acc / float(n_glob)
        return score / score.sum()

    def sensitivity_analysis(self):
        """sensitivity_analysis.csv as NonLinear.sensitivity_analysis writes it (reference :1893-1921):
        features ascending by sensitivity.  Plots and the per-atom mapping need matplotlib / MDAnalysis."""
        if self.cv is None or self.engine is None or self.training_normalized is None:
            return
        score = self.sensitivity_scores()
        if self.comm.rank != 0:
            return
        order = np.argsort(score)
        Path(self.sensitivity_output_folder).mkdir(parents=True, exist_ok=True)
        pd.DataFrame({"sensitivity": score[order]}, index=list(np.array(self.features_ref_labels)[order])).to_csv(
            os.path.join(self.sensitivity_output_folder, "sensitivity_analysis.csv"))

    # ---- persistence
    def _export_dropout(self, cfg: Dict, drops: List[float]) -> List[Optional[float]]:
        """Dropout entry per Linear of the exported module tree: mlcolvar adds a Dropout module wherever the
        configured value is not None -- also for 0 (the bundled models carry Dropout(p=0))."""
        n = len(drops)
        given = self._fit_list((cfg or {}).get("dropout", [None] * (n - 1)), n - 1, "dropout") + [(cfg or {}).get("last_layer_dropout", None)]
        return [None if g is None else float(d) for g, d in zip(given, drops)]

    def _export_parts(self):
        """What every exported module tree starts from: (norm_in, postprocessing, dropout / batch-norm entry per Linear)."""
        st, n = self.cv, len(self.cv["linears"])
        norm = export.Normalization(self.features_norm_mean, self.features_norm_range) if self.feats_norm_mode is not None else None
        post = export.Normalization(*st["post"]) if st.get("post") is not None else None
        return norm, post, st.get("drops") or [0.0] * n, st.get("bn") or [None] * n

    def to_torch_module(self) -> torch.nn.Module:
        raise NotImplementedError

    def save_weights(self, weights_path: str):
        export.save_torchscript(self.to_torch_module(), self.num_features, weights_path)
        self.weights_path = weights_path

    def save_model(self):
        super().save_model()
        if self.cv is None:
            logger.error("No collective variable model to save.")
            return
        self.save_weights(os.path.join(self.model_output_folder, "cv_weights.pt"))
        model_path = os.path.join(self.output_path, "model.zip")
        zip_files(model_path, str(self.model_output_folder))
        shutil.rmtree(self.model_output_folder)
        logger.info(f"Model saved to {model_path}")

    def _load_from_folder(self, folder_path: str):
        super()._load_from_folder(folder_path)
        weights_path = os.path.join(self.model_output_folder, "cv_weights.pt")
        if not os.path.exists(weights_path):
            raise FileNotFoundError(f"CV model weights not found at {weights_path}")
        parts = export.read_torchscript(weights_path)
        self.weights_path = weights_path
        dims = [parts["linears"][0][0].shape[1]] + [w.shape[0] for w, _ in parts["linears"]]
        self.cv = {"linears": parts["linears"], "acts": parts["acts"], "dims": dims, "tica": parts["tica"],
                   "post": parts["postprocessing"], "norm_in": parts["norm_in"], "latent": len(parts["linears"])}
        # projection only needs the chain up to the CV (the AE file's encoder): a plain Linear chain
        bn = parts.get("bn")
        has_bn = bn is not None and any(b is not None for b in bn)
        self.cv["bn"] = bn if has_bn else None
        self.engine = hip.Mlp("deep_tica", dims, parts["acts"], max_batch=32768, lag=0, device=_device(),
                              batchnorm=[b is not None for b in bn] if has_bn else None)
        self.engine.set_linears(parts["linears"], bn=bn if has_bn else None)

    def get_cv_parameters(self):
        return {"cv_name": self.cv_name, "cv_dimension": self.cv_dimension, "weights_path": self.weights_path}

    def get_cv_type(self) -> str:
        return "non-linear"

    def plumed_cv_lines(self) -> str:
        """The non-linear CV section (assembler.py:408-422): normalisations live inside the TorchScript model."""
        return ("\n# Collective variable\n" + f"{self.cv_name}: PYTORCH_MODEL FILE={os.path.abspath(self.weights_path)} "
                f"ARG={','.join(self.features_ref_labels)}\n")

    def plumed_cv_labels(self) -> List[str]:
        return [f"{self.cv_name}.node-{i}" for i in range(self.cv_dimension)]


class AECalculator(NonLinear):
    """Autoencoder CV (reference :2386-2505): encoder [F]+layers+[d], decoder [d]+layers+[F],
    loss = mean squared reconstruction error in the original feature units."""

    model_kind = "ae"

    def __init__(self, configuration: Optional[Dict] = None, output_path: Optional[str] = None):
        super().__init__(configuration, output_path)
        self.cv_name = "ae"

    def layer_plan(self):
        enc_act, enc_drop, enc_bn = self._layer_options(self.encoder_config, len(self.encoder_hidden_layers))
        dec_act, dec_drop, dec_bn = self._decoder_options()
        enc = [self.num_features] + self.encoder_hidden_layers + [self.cv_dimension]
        dec = [self.cv_dimension] + self.decoder_hidden_layers + [self.num_features]
        return enc + dec[1:], enc_act + dec_act, enc_drop + dec_drop, enc_bn + dec_bn, len(enc) - 1

    def to_torch_module(self):
        st = self.cv
        L = st["latent"]
        norm, post, drops, bn = self._export_parts()
        enc = export.FeedForward(st["linears"][:L], st["acts"][:L], self._export_dropout(self.encoder_config, drops[:L]), bn[:L])
        dec_cfg = self.decoder_config if self.decoder_config is not None else self.encoder_config
        dec = export.FeedForward(st["linears"][L:], st["acts"][L:], self._export_dropout(dec_cfg, drops[L:]), bn[L:])
        return export.AutoEncoderCV(norm, enc, dec, post)


class DeepTICACalculator(NonLinear):
    """Deep-TICA CV (reference :2507-2627): norm_in -> FeedForward -> TICA on time-lagged pairs,
    loss = -sum(eigenvalues^2) of the batch TICA."""

    model_kind = "deep_tica"

    def __init__(self, configuration: Optional[Dict] = None, output_path: Optional[str] = None):
        super().__init__(configuration, output_path)
        self.cv_name = "deep_tica"

    def lag(self) -> int:
        return int(self.configuration.get("lag_time"))

    def layer_plan(self):
        act, drop, bn = self._layer_options(self.encoder_config, len(self.encoder_hidden_layers))
        dims = [self.num_features] + self.encoder_hidden_layers + [self.cv_dimension]
        return dims, act, drop, bn, len(dims) - 1

    def n_samples_local(self) -> int:
        return self.training_data.shape[0] - self.lag()   # pairs (i, i+lag) inside this rank's block

    def n_val_samples_local(self) -> int:
        return self.validation_data.shape[0] - self.lag()  # create_timelagged_dataset(validation_data) (reference :2546-2553)

    def _records_to_metrics(self, rec, need_eig: bool = True):
        d = self.cv_dimension
        w = rec[:, 1]
        loss = float((rec[:, 0] * w).sum() / w.sum())
        if not need_eig:
            return loss, None, None
        reg = float(self.configuration.get("tica_regularization", 1e-6))
        # the d x d TICA of every record in one stacked pass (the same LAPACK routine per record as linalg.tica_eigh)
        ev, evecs = linalg.tica_eigh_stack(rec[:, 2:2 + d * d].reshape(-1, d, d), rec[:, 2 + d * d:2 + 2 * d * d].reshape(-1, d, d), reg=reg)
        buffers = (rec[-1, 2 + 2 * d * d:2 + 2 * d * d + d].astype(np.float32), evecs[-1].astype(np.float32))
        eig = (ev * w[:, None]).sum(axis=0) / w.sum()
        return loss, eig, buffers   # buffers: TICA of the LAST batch (SURVEY.md Appendix A.6 ii)

    def to_torch_module(self):
        st = self.cv
        norm, post, drops, bn = self._export_parts()
        nn_ = export.FeedForward(st["linears"], st["acts"], self._export_dropout(self.encoder_config, drops), bn)
        return export.DeepTICA(norm, nn_, export.TICA(st["tica"][1], st["tica"][0]), post)


def kl_annealing_settings(section: Optional[Dict], max_epochs: int) -> Dict:
    """The VAE's KL-annealing parameters (reference VAECalculator.__init__, cv_calculator.py:2645-2660): the configured
    `training.kl_annealing` section, or the defaults when it is absent.  Checked as KLAAnnealing.__init__ checks them: an
    unknown type, or a cyclical schedule with fewer annealing epochs than cycles, raises ValueError here."""
    if section is not None:
        kl = {"type": section.get("type"), "start_beta": section.get("start_beta"), "max_beta": section.get("max_beta"),
              "start_epoch": section.get("start_epoch", max_epochs // 2), "n_cycles": section.get("n_cycles"),
              "n_epochs_anneal": section.get("n_epochs_anneal", max_epochs // 4)}
    else:
        kl = {"type": "sigmoid", "start_beta": 1e-06, "max_beta": 0.01, "start_epoch": max_epochs // 2, "n_cycles": 1,
              "n_epochs_anneal": max_epochs // 4}
    if kl["type"] not in ("linear", "sigmoid", "cyclical"):
        raise ValueError("Invalid type for KLAAnnealing. Must be 'linear' or 'cyclical'.")
    if kl["type"] == "cyclical" and kl["n_epochs_anneal"] < kl["n_cycles"]:
        raise ValueError("n_epochs_anneal must be greater than or equal to n_cycles for cyclical annealing.")
    return kl


def kl_beta(epoch: int, kl: Dict) -> float:
    """beta of `epoch` as the reference's KLAAnnealing callback sets it at the start of that epoch (modules/ml/ml.py): start_beta
    up to and including start_epoch, then the linear / sigmoid / cyclical schedule of the epochs since start_epoch."""
    kind, b0, b1, start, n_anneal = kl["type"], kl["start_beta"], kl["max_beta"], kl["start_epoch"], kl["n_epochs_anneal"]
    if kind not in ("linear", "sigmoid", "cyclical"):
        raise ValueError("Invalid type for KLAAnnealing. Must be 'linear' or 'cyclical'.")

    def linear(e, n):
        if e >= n:
            return b1
        return b0 + (b1 - b0) * (e / n)

    if epoch <= start:
        return b0
    e = epoch - start
    if kind == "linear":
        return float(linear(e, n_anneal))
    if kind == "cyclical":
        if e >= n_anneal:
            return float(b1)
        cycle_length = n_anneal // kl["n_cycles"]
        return float(linear(e % cycle_length, cycle_length // 2))
    eps = 1e-3
    midpoint = start + n_anneal // 2
    steepness = np.log(eps / (1 - eps)) / (start - midpoint)
    return float(b0 + (b1 - b0) / (1 + np.exp(-steepness * (e + start - midpoint))))


def plateau_manager_start(kl: Dict, max_epochs: int) -> int:
    """First epoch of the reference's LROnPlateauManager for a VAE (cv_calculator.py VAECalculator.get_callbacks): the end of
    the annealing plus a quarter of the epochs left after it."""
    end = kl["start_epoch"] + kl["n_epochs_anneal"]
    return end + (max_epochs - kl["start_epoch"] - kl["n_epochs_anneal"]) // 4


class VAECalculator(NonLinear):
    """Variational autoencoder CV (reference :2629-2900, mlcolvar VariationalAutoEncoderCV): encoder [F] + layers (every Linear
    with its activation and dropout), two heads mean_nn / log_var_nn (h -> d, no activation), decoder [d] + layers + [F];
    loss = reconstruction (the AE's) + beta * KL, z = mu + exp(lv / 2) * eps, beta annealed per epoch.  The CV is the mean
    head.  In the engine the heads are ONE Linear of 2d outputs (mean rows, then log-variance rows: dcv.h DCV_MODEL_VAE).
    eps is drawn on the host from torch's global generator, one randn(batch, d) per batch in loader order (training batches,
    then validation batches), and uploaded once per epoch.  Lightning runs its sanity validation before epoch 0 inside
    isolate_rng() (trainer._run_stage), so it leaves the generator where it was and draws nothing here.  Dropout masks come
    from the engine's own generator, as for the AE."""

    model_kind = "vae"

    def __init__(self, configuration: Optional[Dict] = None, output_path: Optional[str] = None):
        super().__init__(configuration, output_path)
        self.cv_name = "vae"
        self.kl = kl_annealing_settings(self.training_config.get("kl_annealing"), self.max_epochs)
        self._post_best: Optional[Tuple[float, Dict]] = None

    def _encoder_options(self):
        n = len(self.encoder_hidden_layers)
        act, drop, bn = self._layer_options(self.encoder_config, n)
        return act[:n], drop[:n], bn[:n]   # the heads take the place of the last-layer entries (set_up_encoder_last_layer)

    def layer_plan(self):
        if self.comm.world > 1:
            raise ValueError("the VAE is not supported in a frame-sharded (multi-GPU) fit: run this CV on one GPU")
        enc_act, enc_drop, enc_bn = self._encoder_options()
        dec_act, dec_drop, dec_bn = self._decoder_options()
        enc = [self.num_features] + self.encoder_hidden_layers + [2 * self.cv_dimension]
        dec = [self.cv_dimension] + self.decoder_hidden_layers + [self.num_features]
        return enc + dec[1:], enc_act + [None] + dec_act, enc_drop + [0.0] + dec_drop, enc_bn + [False] + dec_bn, len(enc) - 1

    def _init_linears(self, dims):
        """Construction order of VariationalAutoEncoderCV: encoder Linears, mean_nn, log_var_nn, decoder Linears (global RNG);
        the heads are concatenated into the engine's one 2d-output Linear."""
        L = len(self.encoder_hidden_layers) + 1   # the first decoder Linear
        d = self.cv_dimension
        lins = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(L - 1)]
        mean, log_var = torch.nn.Linear(dims[L - 1], d), torch.nn.Linear(dims[L - 1], d)
        dec = [torch.nn.Linear(d if i == L else dims[i], dims[i + 1]) for i in range(L, len(dims) - 1)]
        out = [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in lins]
        out.append((torch.cat([mean.weight, log_var.weight]).detach().numpy().copy(), torch.cat([mean.bias, log_var.bias]).detach().numpy().copy()))
        return out + [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in dec]

    # ---- the epoch loop's hooks
    def _noise_for(self, batches) -> List[torch.Tensor]:
        return [torch.randn(batches.size(i), self.cv_dimension) for i in range(len(batches))]

    def _fit_begin(self, sched, n_val: int, bs: int):
        self.engine.set_feature_range(self.features_norm_range)
        self._post_best = None
        if sched is not None and sched.plateau:
            sched.plateau_from = plateau_manager_start(self.kl, self.max_epochs)

    def _epoch_begin(self, epoch: int, tb, make_val_batches):
        self._beta = kl_beta(epoch, self.kl)
        self.engine.set_kl_beta(self._beta)
        eps = self._noise_for(tb)
        vb = make_val_batches()
        if len(vb):
            eps += self._noise_for(vb)
        dev = self.training_normalized.device
        self.engine.set_noise(torch.cat(eps).to(dev) if eps else torch.zeros(0, self.cv_dimension, device=dev))   # one copy per epoch
        return vb

    def _on_validation(self, epoch, rec_train, rec_val, metrics, snapshot):
        valid_loss = metrics["valid_loss"][-1]
        for tag, rec in (("train", rec_train), ("valid", rec_val)):
            w = rec[:, 1]
            metrics.setdefault(f"{tag}_reconstruction_loss", []).append(float((rec[:, 2] * w).sum() / w.sum()))
            metrics.setdefault(f"{tag}_kl_loss", []).append(float((rec[:, 3] * w).sum() / w.sum()))
        metrics.setdefault("beta", []).append(self._beta)
        # PostAnnealingCheckpoint: the lowest valid_loss from the end of the annealing on (only with an annealing stage)
        if self.kl["n_epochs_anneal"] > 0 and epoch >= self.kl["start_epoch"] + self.kl["n_epochs_anneal"]:
            if self._post_best is None or valid_loss < self._post_best[0]:
                self._post_best = (valid_loss, snapshot())

    def _choose_model(self, best_state, best_score, last_state, metrics):
        """model_to_save 'best' of a VAE = the best post-annealing checkpoint; without one, the last (reference :1575-1600)."""
        if self.model_to_save == "best":
            if self._post_best is not None:
                return self._post_best[1], self._post_best[0]
            logger.warning("Best post-annealing model not found, falling back to last model.")
        if last_state is not None:
            return last_state, metrics["valid_loss"][-1]
        return None

    metric_files = NonLinear.metric_files + ("train_kl_loss", "valid_kl_loss", "train_reconstruction_loss", "valid_reconstruction_loss", "beta", "lr")

    # ---- projection / sensitivity / export
    def summed_cv_gradient(self) -> np.ndarray:
        """The CV is the mean half of the heads' output: gradient [1 / post range | 0 for the log-variance half]."""
        d = self.cv_dimension
        g = np.zeros(2 * d, dtype=np.float64)
        g[:d] = 1.0 / np.asarray(self.cv["post"][1], dtype=np.float64) if self.cv.get("post") is not None else 1.0
        return g

    def to_torch_module(self):
        st = self.cv
        L = st["latent"]   # the first decoder Linear; L - 1 = the heads
        d = self.cv_dimension
        n_enc = L - 1
        norm, post, drops, bn = self._export_parts()
        given = self._fit_list(self.encoder_config.get("dropout", [None] * n_enc), n_enc, "dropout") if n_enc else []
        enc = export.FeedForward(st["linears"][:n_enc], st["acts"][:n_enc], [None if g is None else float(p) for g, p in zip(given, drops[:n_enc])],
                                 bn[:n_enc])
        hw, hb = st["linears"][n_enc]
        dec_cfg = self.decoder_config if self.decoder_config is not None else self.encoder_config
        dec = export.FeedForward(st["linears"][L:], st["acts"][L:], self._export_dropout(dec_cfg, drops[L:]), bn[L:])
        return export.VariationalAutoEncoderCV(norm, enc, (hw[:d], hb[:d]), (hw[d:], hb[d:]), dec, post)


cv_calculators_map = {
    "pca": PCACalculator,
    "ae": AECalculator,
    "tica": TICACalculator,
    "htica": HTICACalculator,
    "deep_tica": DeepTICACalculator,
}
# CVs added after the first five; every lookup by name goes through calculator_class
more_cv_calculators_map = {
    "vae": VAECalculator,
}


def calculator_class(name: str):
    """The calculator class of CV `name` (reference cv_calculators_map, cv_calculator.py:2952-2960), or None when this engine
    does not implement it (umap)."""
    return cv_calculators_map.get(name) or more_cv_calculators_map.get(name)
cv_names_map = {"pca": "PCA", "ae": "AE", "tica": "TICA", "htica": "HTICA", "deep_tica": "DeepTICA", "vae": "VAE", "umap": "UMAP"}
cv_components_map = {"pca": "PC", "ae": "AE", "tica": "TIC", "htica": "HTIC", "deep_tica": "DeepTIC", "vae": "VAE", "umap": "UMAP"}
