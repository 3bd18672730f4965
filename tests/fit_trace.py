"""NonLinear.train() on the CPU, with hip.Mlp replaced by a recording stand-in: everything the host driver decides -- seeds,
RNG order of split / initialisation / shuffles / noise, engine construction, batch plans, learning rates, checkpoint cadence,
early stopping, model choice -- shows up as an ordered list of engine calls, which tests/test_fit_trace_cpu.py compares with
tests/golden/fit_trace.json (written by tests/golden/make_golden_fit_trace.py).  A helper module, not a conftest.

The stand-in answers read_log() with records whose loss column follows the case's list of epoch losses (try t lies
0.125 * (t - 1) lower, so the second try wins), and get_linears() with a tag {"engine": try, "reads": read_log calls so far}:
the chosen cv["linears"] tells which checkpoint of which try won."""
import copy
import hashlib
import json
import math

import numpy as np
import torch

N_FRAMES, N_FEATURES, N_VAL_FRAMES, DIM = 103, 5, 41, 2
LOSSES = [3.0, 2.0, 1.0, 1.5, 1.6, 1.7]
NAN_LOSSES = [3.0, math.nan, 1.0, 1.5, 1.6, 1.7]
# Deep-TICA records: C0 and Ct of every batch.  Diagonal, so that Cholesky, inverse and eigh are exact in IEEE arithmetic and the
# eigenvalue metrics do not depend on the BLAS build behind numpy.
C0_BLOCK = np.diag([2.0, 1.0])
CT_BLOCK = np.diag([0.5, 0.75])


def digest(a) -> str:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()[:16]


def jsonable(v):
    """Plain JSON data: arrays and tensors as digests, everything else by value."""
    if isinstance(v, (torch.Tensor, np.ndarray)):
        return {"sha256": digest(v)}
    if isinstance(v, dict):
        return {str(k): jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [jsonable(x) for x in v]
    if isinstance(v, (np.floating, np.integer, np.bool_)):
        return v.item()
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return str(v)


class OneRankOfTwo:
    """Stand-in for parallel.Comm: rank 0 of 2, every collective returns the one-rank answer."""
    active, world, rank, group, _dist = True, 2, 0, None, "dist"

    def min_(self, t):
        return t

    sum_ = max_ = min_

    def barrier(self):
        pass

    def sum_scalar(self, v, device="cpu"):
        return float(v)


def recording_engine(ctx):
    """The class that takes hip.Mlp's place during one case.  ctx: trace (list), losses, calc, engines (count)."""
    trace = ctx["trace"]

    class RecordingMlp:
        def __init__(self, model, dims, acts, **kw):
            ctx["engines"] += 1
            self.no, self.model, self.reads, self.pending, self.closed = ctx["engines"], model, 0, [], False
            d = DIM
            self.log_width = {"deep_tica": 2 + 2 * d * d + d, "ae": 2, "vae": 4}[model]
            trace.append(["Mlp", jsonable(dict(kw, model=model, dims=list(dims), acts=list(acts)))])

        def _matrix(self, Xn):
            calc = ctx["calc"]
            return "train" if Xn is calc.training_normalized else "val" if Xn is calc.validation_normalized else "other"

        def _rows(self, idx, row0, batch):
            if idx is not None:
                return {"idx": digest(idx), "n": int(idx.numel())}
            return {"row0": int(row0), "batch": int(batch)}

        # ---- state
        def set_linears(self, linears, bn=None):
            if isinstance(linears, dict):
                trace.append(["set_linears", {"tag": linears, "bn": jsonable(bn)}])
            else:
                trace.append(["set_linears", {"linears": [[digest(w), digest(b)] for w, b in linears], "bn": jsonable(bn)}])

        def set_rank(self, rank):
            trace.append(["set_rank", int(rank)])

        def set_feature_range(self, rng):
            trace.append(["set_feature_range", digest(np.asarray(rng, dtype=np.float64))])

        def set_lr(self, lr):
            trace.append(["set_lr", float(lr)])

        def set_momentum(self, value):
            trace.append(["set_momentum", float(value)])

        def set_kl_beta(self, beta):
            trace.append(["set_kl_beta", float(beta)])

        def set_noise(self, eps):
            trace.append(["set_noise", {"shape": list(eps.shape), "sha256": digest(eps)}])

        def close(self):
            if not self.closed:
                trace.append(["close", self.no])
            self.closed = True

        # ---- work
        def _one(self, name, Xn, idx, row0, batch, **more):
            rows = self._rows(idx, row0, batch)
            self.pending.append(rows.get("n", rows.get("batch")))
            trace.append([name, dict(rows, X=self._matrix(Xn), **more)])

        def train_step(self, Xn, idx=None, row0=0, batch=None):
            self._one("train_step", Xn, idx, row0, batch)

        def eval_step(self, Xn, idx=None, row0=0, batch=None):
            self._one("eval_step", Xn, idx, row0, batch)

        def data_parallel_step(self, Xn, dist, global_batch, idx=None, row0=0, batch=None, train=True, group=None):
            self._one("data_parallel_step", Xn, idx, row0, batch, global_batch=int(global_batch), train=bool(train), dist=str(dist), group=str(group))

        def _many(self, name, Xn, batch, count, idx, row0):
            self.pending += [int(batch)] * int(count)
            rows = {"idx": digest(idx), "n": int(idx.numel())} if idx is not None else {"row0": int(row0)}
            trace.append([name, dict(rows, X=self._matrix(Xn), batch=int(batch), count=int(count))])

        def train_steps(self, Xn, batch, nsteps, idx=None, row0=0):
            self._many("train_steps", Xn, batch, nsteps, idx, row0)

        def eval_steps(self, Xn, batch, nbatches, idx=None, row0=0):
            self._many("eval_steps", Xn, batch, nbatches, idx, row0)

        # ---- log
        def reset_log(self, capacity):
            self.pending = []
            trace.append(["reset_log", int(capacity)])

        def read_log(self):
            trace.append(["read_log", len(self.pending)])
            loss = ctx["losses"][self.reads] - 0.125 * (self.no - 1)
            self.reads += 1
            rec = np.zeros((len(self.pending), self.log_width), dtype=np.float64)
            rec[:, 0] = loss
            rec[:, 1] = self.pending
            if self.model == "deep_tica":
                d = DIM
                rec[:, 2:2 + d * d] = C0_BLOCK.reshape(-1)
                rec[:, 2 + d * d:2 + 2 * d * d] = CT_BLOCK.reshape(-1)
                rec[:, 2 + 2 * d * d:] = [0.25, -0.5]
            elif self.model == "vae":
                rec[:, 2], rec[:, 3] = 0.75 * loss, 0.25 * loss
            return rec

        # ---- read-only getters: answered, not part of the ordered trace
        def get_linears(self):
            return {"engine": self.no, "reads": self.reads}

        def get_bn(self):
            return {"bn_of_engine": self.no, "reads": self.reads}

        def stats_view(self):
            return None

        def grads_view(self):
            return None

    return RecordingMlp


def _base_config():
    return {"dimension": DIM, "features_normalization": "mean_std", "lag_time": 1,
            "architecture": {"encoder": {"layers": [4, 3]}},
            "training": {"general": {"num_tries": 2, "seed": 42, "batch_size": 16, "max_epochs": 6, "shuffle": True, "random_split": True,
                                     "check_val_every_n_epoch": 1, "save_check_every_n_epoch": 1},
                         "early_stopping": {"patience": 2, "min_delta": 1e-5}}}


def _with(cfg, general=None, training=None, encoder=None):
    cfg = copy.deepcopy(cfg)
    cfg["training"]["general"].update(general or {})
    cfg["training"].update(training or {})
    cfg["architecture"]["encoder"].update(encoder or {})
    return cfg


_PLATEAU = {"lr_scheduler": {"name": "ReduceLROnPlateau", "kwargs": {"factor": 0.5}}}
# name -> (CV, configuration, options: val = separate validation matrix, losses, comm = data-parallel stand-in)
CASES = {
    "deep_tica": ("deep_tica", _base_config(), {}),
    "ae": ("ae", _base_config(), {}),
    "vae": ("vae", _with(_base_config(), training={"kl_annealing": {
        "type": "sigmoid", "start_beta": 1e-6, "max_beta": 0.01, "start_epoch": 2, "n_cycles": 1, "n_epochs_anneal": 2}}), {}),
    "ae_ordered": ("ae", _with(_base_config(), general={"shuffle": False, "random_split": False}), {}),
    "deep_tica_one_batch": ("deep_tica", _with(_base_config(), general={"batch_size": 0}), {}),
    "ae_one_cycle": ("ae", _with(_base_config(), training={"lr_scheduler": {"name": "OneCycleLR", "kwargs": {"max_lr": 0.01}}}), {}),
    "deep_tica_plateau": ("deep_tica", _with(_base_config(), training=_PLATEAU), {}),
    "ae_last": ("ae", _with(_base_config(), general={"save_check_every_n_epoch": 2}, training={"model_to_save": "last"}), {}),
    "vae_anneal_plateau": ("vae", _with(_base_config(), training=dict(_PLATEAU, kl_annealing={
        "type": "linear", "start_beta": 0.0, "max_beta": 0.01, "start_epoch": 1, "n_cycles": 1, "n_epochs_anneal": 2})), {}),
    "deep_tica_separate_val": ("deep_tica", _base_config(), {"val": True}),
    "ae_nan": ("ae", _base_config(), {"losses": NAN_LOSSES}),
    "ae_two_ranks": ("ae", _base_config(), {"comm": True}),
    "ae_two_ranks_batchnorm": ("ae", _with(_base_config(), encoder={"batchnorm": [True, False]}), {"comm": True}),
}
NO_RNG_DIGEST = ("ae_nan",)   # the one intended change of behaviour: the generator after a non-finite loss


def make_calculator(cv_name, configuration, val=False, comm=False):
    """A calculator with CPU tensors in the places load_training_data() fills on the GPU."""
    from deep_cartograph_amd.cv_calculator import calculator_class

    calc = calculator_class(cv_name)(configuration=configuration, output_path=None)
    g = torch.Generator().manual_seed(7)
    X = torch.randn(N_FRAMES, N_FEATURES, generator=g)
    mean, std = X.numpy().astype(np.float64).mean(axis=0), X.numpy().astype(np.float64).std(axis=0)
    norm = lambda M: ((M - torch.from_numpy(mean).float()) / torch.from_numpy(std).float()).contiguous()
    calc.training_data, calc.training_normalized = X, norm(X)
    calc.num_features, calc.num_frames_global = N_FEATURES, N_FRAMES
    calc.features_norm_mean, calc.features_norm_range = mean, std
    if val:
        V = torch.randn(N_VAL_FRAMES, N_FEATURES, generator=g)
        calc.validation_data, calc.validation_normalized = V, norm(V)
    if comm:
        calc.comm = OneRankOfTwo()
    return calc


def run_case(name, general=None):
    """Everything train() did in case `name`, as JSON data.  `general`: overrides of training.general."""
    from deep_cartograph_amd import hip

    cv_name, configuration, opt = CASES[name]
    configuration = _with(configuration, general=general)
    ctx = {"trace": [], "losses": opt.get("losses", LOSSES), "calc": None, "engines": 0}
    real = hip.Mlp
    hip.Mlp = recording_engine(ctx)
    try:
        torch.manual_seed(0)
        calc = ctx["calc"] = make_calculator(cv_name, configuration, val=opt.get("val", False), comm=opt.get("comm", False))
        ret = calc.train()
        rng = digest(torch.get_rng_state())
    finally:
        hip.Mlp = real
    cv = dict(calc.cv) if calc.cv is not None else None
    out = {"trace": ctx["trace"], "return": ret, "cv_score": calc.cv_score, "metrics": calc.metrics,
           "chosen": cv.pop("linears") if cv is not None else None, "cv": cv, "tries": calc.tries, "rng": rng}
    return json.loads(json.dumps(jsonable(out)))   # what a reader of the golden file sees (tuples are lists)


def first_difference(got, want, path="result"):
    """None when equal, else a line naming the first entry that differs."""
    if type(got) is not type(want):
        return f"{path}: {got!r} != {want!r}"
    if isinstance(got, dict):
        for k in sorted(set(got) | set(want)):
            if k not in got or k not in want:
                return f"{path}[{k!r}]: {'missing' if k not in got else got[k]!r} != {'missing' if k not in want else want[k]!r}"
            d = first_difference(got[k], want[k], f"{path}[{k!r}]")
            if d:
                return d
        return None
    if isinstance(got, list):
        for i, (a, b) in enumerate(zip(got, want)):
            d = first_difference(a, b, f"{path}[{i}]")
            if d:
                return d
        return None if len(got) == len(want) else f"{path}: {len(got)} entries != {len(want)} (first extra: {max(got, want, key=len)[min(len(got), len(want))]!r})"
    return None if got == want else f"{path}: {got!r} != {want!r}"
