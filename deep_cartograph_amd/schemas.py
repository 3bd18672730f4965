"""Configuration contract of the CV-fit path: pydantic models with the field names, defaults
and `extra` policy of the reference's deep_cartograph/yaml_schemas/{filter_features,train_colvars,
traj_cluster,traj_projection}.py.  tests/test_host_cpu.py checks model_dump() of the defaults against the
reference's own dump (tests/golden/schema_defaults.json)."""
from __future__ import annotations

from typing import Dict, List, Literal, Optional, Union

from pydantic import BaseModel, ConfigDict

Activation = Literal["relu", "elu", "tanh", "softplus", "shifted_softplus", "custom_sigmoid", "leaky_relu", "linear"]


class Optimizer(BaseModel):
    name: str = "Adam"
    kwargs: dict = {"lr": 1.0e-04, "weight_decay": 0.0}


class RLScheduler(BaseModel):
    name: str = "OneCycleLR"
    kwargs: dict = {}


class NeuralNetwork(BaseModel):
    layers: List[int] = [64, 32, 16]
    activation: List[Optional[Activation]] = ["leaky_relu", "leaky_relu", "leaky_relu"]
    batchnorm: List[bool] = [False, False, False]
    dropout: List[Optional[float]] = [None, None, None]
    last_layer_activation: Optional[Activation] = None
    last_layer_batchnorm: bool = False
    last_layer_dropout: Optional[float] = None


class Architecture(BaseModel):
    encoder: NeuralNetwork = NeuralNetwork()
    decoder: NeuralNetwork = NeuralNetwork()


class GeneralSettings(BaseModel):
    num_tries: int = 10
    seed: int = 42
    lengths: List[float] = [0.8, 0.2]
    batch_size: int = 32
    max_epochs: int = 1000
    shuffle: bool = False
    random_split: bool = True
    check_val_every_n_epoch: int = 10
    save_check_every_n_epoch: int = 10


class InputColvars(BaseModel):
    start: int = 0
    stop: Union[int, None] = None
    stride: int = 1


class EarlyStopping(BaseModel):
    patience: int = 20
    min_delta: float = 1.0e-05


class KLAnnealing(BaseModel):
    type: Literal["linear", "sigmoid", "cyclical"] = "linear"
    start_beta: float = 1e-06
    max_beta: float = 0.01
    start_epoch: int = 1000
    n_cycles: int = 4
    n_epochs_anneal: int = 5000


class Trainings(BaseModel):
    general: GeneralSettings = GeneralSettings()
    early_stopping: EarlyStopping = EarlyStopping()
    optimizer: Optimizer = Optimizer()
    lr_scheduler: Optional[RLScheduler] = None
    lr_scheduler_config: Optional[dict] = {"interval": "epoch", "monitor": "valid_loss", "frequency": 1}
    kl_annealing: Optional[KLAnnealing] = None
    save_loss: bool = True
    plot_loss: bool = True
    model_to_save: Literal["best", "last"] = "best"


class BiasArgs(BaseModel):
    temperature: float = 300.0
    sigma: float = 0.05
    pace: int = 500
    grid_min: float = -1.0
    grid_max: float = 1.0
    grid_bin: int = 300
    height: float = 1.0
    bias_factor: float = 10.0
    barrier: float = 50.0
    observation_steps: int = 100
    compression_threshold: float = 0.1


class Bias(BaseModel):
    method: Literal["wt_metadynamics", "opes_metad", "opes_metad_explore", "opes_expanded"] = "opes_metad"
    args: BiasArgs = BiasArgs()
    add_rmsd_restraint: bool = False
    align_waypoint_structures: bool = True
    rmsd_restraint_k: float = 5000.0
    rmsd_restraint_eq: float = 0.4


class CommonCollectiveVariable(BaseModel):
    dimension: int = 2
    lag_time: int = 1
    tica_regularization: float = 1.0e-06
    features_normalization: Optional[Literal["mean_std", "min_max_range1", "min_max_range2"]] = None
    input_colvars: InputColvars = InputColvars()
    architecture: Architecture = Architecture()
    training: Trainings = Trainings()
    num_subspaces: int = 10
    subspaces_dimension: int = 5
    n_neighbors: int = 15
    min_dist: float = 0.1
    metric: str = "euclidean"
    bias: Bias = Bias()


class FesFigure(BaseModel):
    compute: bool = True
    save: bool = True
    temperature: int = 300
    bandwidth: float = 0.05
    num_fes_levels: int = 10
    num_bins: int = 150
    max_fes: float = 30


class TrajProjection(BaseModel):
    plot: bool = True
    num_bins: int = 100
    bandwidth: float = 0.25
    alpha: float = 0.8
    cmap: str = "turbo"
    marker_size: int = 5


class Figures(BaseModel):
    fes: FesFigure = FesFigure()
    traj_projection: TrajProjection = TrajProjection()


class TrainColvarsSchema(BaseModel):
    # per-CV override sections (e.g. `deep_tica: {...}`) are extra fields, as in the reference
    model_config = ConfigDict(extra="allow")
    cvs: List[Literal["pca", "ae", "tica", "htica", "deep_tica", "vae", "umap"]] = ["pca", "ae", "tica", "htica", "deep_tica", "vae", "umap"]
    common: CommonCollectiveVariable = CommonCollectiveVariable()
    figures: Figures = Figures()


class ClusterFigures(BaseModel):
    plot: bool = True
    num_bins: int = 100
    bandwidth: float = 0.25
    alpha: float = 0.8
    cmap: str = "turbo"
    marker_size: int = 5


class TrajClusterSchema(BaseModel):
    run: bool = True
    output_structures: Optional[Literal["centroids", "all"]] = "centroids"
    algorithm: Literal["kmeans", "hdbscan", "hierarchical"] = "hierarchical"
    opt_num_clusters: bool = True
    search_interval: List[int] = [3, 10]
    num_clusters: int = 10
    linkage: str = "complete"
    n_init: int = 20
    min_cluster_size: int = 5
    max_cluster_size: Union[int, None] = None
    min_samples: int = 3
    cluster_selection_epsilon: float = 0
    cluster_selection_method: Literal["eom", "leaf"] = "eom"
    figures: ClusterFigures = ClusterFigures()


class TrajProjectionSchema(BaseModel):
    figures: Figures = Figures()


class FilterSettings(BaseModel):
    # distance threshold to distinguish local contacts, in Angstroms (None skips the filter)
    local_distance_threshold: Optional[float] = None
    # significance level of Hartigan's dip test (None skips the filter)
    diptest_significance_level: Optional[float] = 0.05
    # entropy quantile below which features are dropped (None skips the filter)
    entropy_quantile: Optional[float] = None
    # standard deviation quantile below which features are dropped (None skips the filter)
    std_quantile: Optional[float] = None


class SamplingSettings(BaseModel):
    # accepted and unused, as in the reference's Filter
    num_samples: Union[int, None] = None
    total_num_samples: Union[int, None] = None
    relaxation_time: int = 1


class FilterFeaturesSchema(BaseModel):
    filter_settings: FilterSettings = FilterSettings()
    sampling_settings: SamplingSettings = SamplingSettings()


# ---------------------------------------------------------------- compute_features (yaml_schemas/compute_features.py)
class CoordinateGroup(BaseModel):
    selection: str = "not name H*"
    stride: int = 1


class DistanceGroup(BaseModel):
    first_selection: str = "not name H*"
    second_selection: str = "not name H*"
    # keep every first_stride-th / second_stride-th atom of the selections
    first_stride: int = 1
    second_stride: int = 5
    # skip pairs of atoms in the same or in neighbouring residues
    skip_neigh_residues: bool = False
    # skip pairs of bonded atoms
    skip_bonded_atoms: bool = True


class DihedralGroup(BaseModel):
    selection: str = "not name H*"
    # sin and cos of the angle instead of the angle
    periodic_encoding: bool = True
    # only "virtual" is computed here; the other two are refused by trajectory.feature_definitions
    search_mode: Literal["virtual", "protein_backbone", "real"] = "real"


class DistanceToCenterGroup(BaseModel):
    selection: str = "not name H*"
    center_selection: str = "not name H*"


class Features(BaseModel):
    coordinate_groups: Dict[str, CoordinateGroup] = {}
    distance_groups: Dict[str, DistanceGroup] = {}
    dihedral_groups: Dict[str, DihedralGroup] = {}
    distance_to_center_groups: Dict[str, DistanceToCenterGroup] = {}


class PlumedSettings(BaseModel):
    # accepted and ignored: there is no PLUMED subprocess to time out
    timeout: int = 172800
    # keep one frame in every traj_stride
    traj_stride: int = 1
    features: Features = Features()


class PlumedEnvironment(BaseModel):
    # accepted and ignored: the features are computed by libdcv.so
    bin_path: str = "plumed"
    kernel_path: Union[str, None] = None
    env_commands: List[str] = []


class ComputeFeaturesSchema(BaseModel):
    plumed_settings: PlumedSettings = PlumedSettings()
    plumed_environment: PlumedEnvironment = PlumedEnvironment()
    # this project's extension: "npy" writes the binary fast path colvars.npy + colvars.names.txt, "dat" a COLVAR text file
    colvars_format: Literal["npy", "dat"] = "npy"


# ---------------------------------------------------------------- analyze_geometry (yaml_schemas/analyze_geometry.py)
# The reference's default selections are "protein and name CA"; the selection grammar here has no `protein` keyword
# (trajectory.select_atoms), so the defaults are "name CA".
class RMSSettings(BaseModel):
    title: str
    # atoms the RMS is computed for
    selection: str = "name CA"
    # atoms every frame is fitted on before the RMS is computed
    fit_selection: str = "name CA"


class RMSDSettings(RMSSettings):
    title: str = "Protein Backbone RMSD"


class RMSFSettings(RMSSettings):
    title: str = "Protein Backbone RMSF"


class dRMSDSettings(BaseModel):
    title: str = "Protein Backbone dRMSD"
    selection: str = "name CA"
    # keep every selection_stride-th atom of the selection
    selection_stride: int = 5


class AnalysisList(BaseModel):
    RMSD: Dict[str, RMSDSettings] = {}
    RMSF: Dict[str, RMSFSettings] = {}
    dRMSD: Dict[str, dRMSDSettings] = {}


class AnalyzeGeometrySchema(BaseModel):
    analysis: AnalysisList = AnalysisList()
    # time between frames in ps
    dt_per_frame: float = 1.0
    run: bool = True


# ---------------------------------------------------------------- traj_augmentation (yaml_schemas/traj_augmentation.py)
class TrajAugmentationSchema(BaseModel):
    # frames of the interpolated trajectory (ignored with interpolation_method: null)
    num_frames: int = 1000
    # keep the original frames among the interpolated ones
    keep_original_frames: bool = False
    # akima (modified Akima, smoother) or pchip (monotone between frames); null emits the original frames
    interpolation_method: Optional[Literal["akima", "pchip"]] = "pchip"
    # standard deviation of the Gaussian noise added to every coordinate (null: none)
    noise_std: Optional[float] = None
    random_seed: int = 42
    # atoms written to the new trajectory and topology (trajectory.select_atoms)
    atom_selection: str = "all"
    # "dcd" or "npy" are written; the reference's default "xtc" and its "nc" / "pdb" are accepted here and refused by
    # augmentation.interpolate_trajectory with an error that names the option (no compressed or NetCDF writer)
    traj_format: Literal["dcd", "npy", "xtc", "nc", "pdb"] = "dcd"
    # unwrapping and centring need the box: true is refused by augmentation.interpolate_trajectory
    prepare_trajectory: bool = False
