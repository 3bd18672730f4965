"""Training driver of the neural CVs (reference NonLinear.train, cv_calculator.py:1456-1642): what one try does on the host,
whichever calculator it serves -- seed and split, build and load the HIP engine, the epoch loop with its batch plans,
learning-rate scheduler, checkpoint cadence and early stopping.  NonLinear.train() (cv_calculator.py) builds one FitPlan and
runs a Try per try; the model-specific parts stay on the calculator (layer_plan, _init_linears, _records_to_metrics and the four
hooks _fit_begin / _epoch_begin / _on_validation / _choose_model)."""
from __future__ import annotations

import functools
import logging
import random
from collections import namedtuple
from typing import Dict, Optional

import numpy as np
import torch

from . import hip

logger = logging.getLogger(__name__)


class _torch_threads:
    """with _torch_threads(k): torch's intra-op thread count capped at k for the block (restored afterwards)."""

    def __init__(self, k: int):
        self.k = k

    def __enter__(self):
        self.prev = torch.get_num_threads()
        if self.prev > self.k:
            torch.set_num_threads(self.k)
        return self

    def __exit__(self, *exc):
        if torch.get_num_threads() != self.prev:
            torch.set_num_threads(self.prev)
        return False


class _Batches:
    """The batches of one pass over a DictLoader, without the per-batch objects: kind 'idx' (base = the device index list of
    the pass, batch i = base[i * bs:(i + 1) * bs]) or 'range' (base = first row, batch i = rows base + i * bs ...)."""

    def __init__(self, kind: str, base, n: int, bs: int):
        self.kind, self.base, self.n, self.bs = kind, base, int(n), int(bs)
        self.count = (self.n + self.bs - 1) // self.bs if self.n > 0 else 0

    def __len__(self):
        return self.count

    def size(self, i: int) -> int:
        return min(self.bs, self.n - i * self.bs)

    def full(self) -> int:
        """Number of leading batches of the full size bs."""
        return self.n // self.bs

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self.count))]
        if i < 0:
            i += self.count
        if not 0 <= i < self.count:
            raise IndexError(i)
        if self.kind == "idx":
            return ("idx", self.base[i * self.bs:i * self.bs + self.size(i)], self.base)
        return ("range", self.base + i * self.bs, self.size(i))

    def __iter__(self):
        return (self[i] for i in range(self.count))


class _HostLRScheduler:
    """torch.optim.lr_scheduler.<name> (reference :1382-1394, adjusted by :1228-1273) evaluated on the host: the very
    torch class runs over a one-parameter optimiser of the configured type, and after each of its steps the
    learning rate -- and beta1 / momentum, which OneCycleLR and CyclicLR cycle too -- are handed to the HIP engine.
    Stepping follows lightning's lr_scheduler_config: interval 'step' (after every optimiser step) or 'epoch'
    (at the end of every epoch), every `frequency`-th time; ReduceLROnPlateau receives the monitored valid_loss."""

    def __init__(self, name: str, kwargs: Dict, config: Dict, opt_name: str, opt_kwargs: Dict, engine):
        cls = getattr(torch.optim.lr_scheduler, name, None)
        if cls is None:
            logger.error(f"Learning rate scheduler {name} not recognized. Exiting...")
            raise ValueError(f"Learning rate scheduler {name} not recognized.")
        self.opt = getattr(torch.optim, opt_name)([torch.nn.Parameter(torch.zeros(1))], **opt_kwargs)
        self.sched = cls(self.opt, **kwargs)
        self.plateau = isinstance(self.sched, torch.optim.lr_scheduler.ReduceLROnPlateau)
        self.interval = config.get("interval", "epoch")
        self.frequency = max(1, int(config.get("frequency", 1)))
        self.monitor = config.get("monitor", "valid_loss")
        self.engine = engine
        self.count = 0
        self.plateau_from: Optional[int] = None   # VAE: LROnPlateauManager's extra step from this epoch on (set by the calculator)
        self.push()

    def push(self):
        g = self.opt.param_groups[0]
        self.engine.set_lr(float(g["lr"]))
        if "betas" in g:
            self.engine.set_momentum(float(g["betas"][0]))
        elif "momentum" in g:
            self.engine.set_momentum(float(g["momentum"]))

    def lr(self) -> float:
        return float(self.opt.param_groups[0]["lr"])

    def _advance(self, metric=None):
        self.count += 1
        if self.count % self.frequency:
            return
        self.opt.step()   # no gradients: a no-op that keeps torch's call-order check quiet
        if self.plateau:
            if metric is None:   # lightning raises MisconfigurationException here
                raise ValueError(f"ReduceLROnPlateau conditioned on metric {self.monitor} which is not available yet "
                                 "(set check_val_every_n_epoch to 1)")
            self.sched.step(metric)
        else:
            self.sched.step()
        self.push()

    def after_step(self):
        if self.interval == "step":
            self._advance()

    def after_epoch(self, last_valid_loss):
        if self.interval == "epoch":
            self._advance(last_valid_loss)

    def on_validation_end(self, epoch: int, valid_loss: float):
        """The reference's LROnPlateauManager (VAE, modules/ml/ml.py): at the end of every validation from epoch `plateau_from`
        on, ReduceLROnPlateau is stepped once more with the validation loss, outside lightning's interval / frequency."""
        if self.plateau and self.plateau_from is not None and epoch >= self.plateau_from:
            self.sched.step(valid_loss)
            self.push()


def split(n: int, lengths, random_split: bool, generator):
    """DictModule split: fractional lengths = floor + round-robin remainder; random_split uses
    ONE randperm of the given generator, else consecutive blocks."""
    sizes = [int(np.floor(n * f)) for f in lengths]
    for i in range(n - sum(sizes)):
        sizes[i % len(sizes)] += 1
    perm = torch.randperm(n, generator=generator) if random_split else None
    out, off = [], 0
    for s in sizes:
        out.append((perm[off:off + s].clone() if perm is not None else (off, s)))
        off += s
    return out


def batches(part, batch_size: int, shuffle: bool, dev) -> _Batches:
    """DictLoader: consecutive slices of batch_size, last partial batch kept, fresh randperm per
    epoch when shuffling.  A sequence of ('idx', tensor, whole list) or ('range', row0, count) entries, materialised on
    access (an epoch of 10 000 batches issued by ONE dcv_mlp_train_steps call never builds 10 000 views)."""
    if isinstance(part, tuple):
        off, n = part
        if shuffle:
            part = torch.arange(off, off + n)
        else:
            return _Batches("range", off, n, batch_size if batch_size > 0 else n)
    idx = part
    if shuffle:
        idx = idx[torch.randperm(len(idx))]   # the reference's permutation (global CPU generator)
    bs = batch_size if batch_size > 0 else len(idx)
    idx_d = idx.to(dev).contiguous()   # one copy per epoch; the batches are consecutive views of it (third field: the whole list)
    return _Batches("idx", idx_d, len(idx), bs)


def part_len(part) -> int:
    return part[1] if isinstance(part, tuple) else len(part)


# What every try of one train() call shares (immutable): the model description (layer_plan: dims, activation / dropout / batch-norm
# flag per Linear, latent index), the optimiser (torch.optim name, keyword arguments with torch's defaults) and this rank's sample
# counts and batch size (0 = one batch per pass).
FitPlan = namedtuple("FitPlan", "dims acts drops bn latent opt_name opt_kw n_local n_val_local local_bs")


class Try:
    """One training try of calculator `calc`: run() = seed_and_split, build_engine, epochs."""

    def __init__(self, calc, plan: FitPlan, try_num: int):
        self.calc, self.plan, self.try_num = calc, plan, try_num
        self.seed = calc.seed + try_num
        self.dev = calc.training_data.device
        self.separate_val = calc.validation_data is not None
        self.sched: Optional[_HostLRScheduler] = None
        self.metrics: Dict[str, list] = {"train_loss": [], "valid_loss": [], "epoch": []}
        # ModelCheckpoint(save_top_k=1, save_last=True) and EarlyStopping(monitor=valid_loss, mode=min)
        self.best_score, self.best_state, self.last_state = float("inf"), None, None
        self.es_best, self.wait, self.last_valid = float("inf"), 0, None

    def run(self) -> Optional[Dict]:
        """{"state", "score", "metrics"} of the try's chosen model, or None when it has none."""
        self.build_engine(self.seed_and_split())
        self.epochs()
        c, metrics = self.calc, self.metrics
        if metrics["valid_loss"] and min(metrics["valid_loss"]) > metrics["valid_loss"][0]:
            logger.warning(f"Try {self.try_num}: validation loss did not decrease during training.")
        chosen = c._choose_model(self.best_state, self.best_score, self.last_state, metrics)
        if chosen is None:
            logger.error("Training finished, but no valid model checkpoint was found.")
            return None
        state, score = chosen
        if c.cv_name == "deep_tica" and score < -float(c.cv_dimension):
            logger.warning(f"Deep TICA validation loss ({score:.5f}) is below the theoretical minimum "
                           f"({-float(c.cv_dimension):.5f}). Try reducing the learning rate or increasing 'tica_regularization'.")
            return None
        return {"state": state, "score": score, "metrics": metrics}

    def seed_and_split(self):
        """Seeds, then split and model initialisation in the reference's RNG order; returns the initial Linears."""
        c, p = self.calc, self.plan
        random.seed(self.seed)
        np.random.seed(self.seed % (2 ** 32))
        gen = torch.manual_seed(self.seed)           # seed_everything + DictModule(generator=manual_seed(seed))
        # RNG order (SURVEY.md Appendix A.6 i): create_model() first, the split inside trainer.fit second --
        # unless a scheduler is configured, whose _adjust_lr_scheduler_from_datamodule splits before the model exists
        split_first = c.lr_scheduler is not None and not self.separate_val
        parts = split(p.n_local, c.training_validation_lengths, c.random_split, gen) if split_first else None
        linears = c._init_linears(p.dims)
        if self.separate_val:       # DictLoader over the whole training set and over the validation set (:1485-1492)
            self.train_part, self.val_part = (0, p.n_local), (0, p.n_val_local)
        else:
            if parts is None:
                parts = split(p.n_local, c.training_validation_lengths, c.random_split, gen)
            # index plans live on the GPU
            self.train_part, self.val_part = [q if isinstance(q, tuple) or c.shuffle else q.to(self.dev) for q in parts[:2]]
        self.Xn_train = c.training_normalized
        self.Xn_val = c.validation_normalized if self.separate_val else c.training_normalized
        self.n_tr, self.n_va = part_len(self.train_part), part_len(self.val_part)
        self.bs = p.local_bs if p.local_bs > 0 else max(self.n_tr, self.n_va, 1)
        return linears

    def build_engine(self, linears):
        """The calculator's engine for this try, loaded with the initial parameters, and the scheduler that drives it."""
        c, p = self.calc, self.plan
        if c.engine is not None:
            c.engine.close()
        nmax = max(1, min(self.bs, max(self.n_tr, self.n_va)))
        c.engine = hip.Mlp(c.model_kind, p.dims, p.acts, max_batch=nmax, lag=c.lag(), latent_layer=p.latent,
                           tica_reg=float(c.configuration.get("tica_regularization", 1e-6)), dropout=p.drops, seed=self.seed, device=self.dev,
                           batchnorm=p.bn, **c._engine_optimizer_kwargs(p.opt_name, p.opt_kw))
        c.engine.set_linears(linears)
        c.engine.set_rank(c.comm.rank)   # data-parallel ranks hold the same seed: independent dropout masks per rank
        if c.comm.world > 1 and any(p.bn):
            # each rank would normalise with its local rows and keep its own running statistics: no longer the reference's
            # single-process fit (dcv_mlp_dp_step refuses it too) -- say so before the first step
            raise ValueError("batchnorm / last_layer_batchnorm are not supported in a frame-sharded (multi-GPU) fit: run this CV on one GPU "
                             "or drop the option")
        if c.model_kind == "ae":
            c.engine.set_feature_range(c.features_norm_range)
        so = c._scheduler_options((self.n_tr + self.bs - 1) // self.bs)   # len(train_loader)
        if so is not None:
            self.sched = _HostLRScheduler(*so, p.opt_name, dict(p.opt_kw), c.engine)
            self.metrics["lr"] = []
        c._fit_begin(self.sched, self.n_va, self.bs)

    def batches(self, part) -> _Batches:
        return batches(part, self.bs, self.calc.shuffle, self.dev)

    def step(self, Xn, batch, train: bool):
        c = self.calc
        kw = dict(idx=batch[1]) if batch[0] == "idx" else dict(row0=batch[1], batch=batch[2])
        n = int(batch[1].numel()) if batch[0] == "idx" else int(batch[2])
        if not c.comm.active:
            (c.engine.train_step if train else c.engine.eval_step)(Xn, **kw)
            return
        # equal shards: every rank runs the same batch sizes
        c.engine.data_parallel_step(Xn, c.comm._dist, n * c.comm.world, train=train, group=c.comm.group, **kw)

    def run_batches(self, Xn, plan, train: bool, per_step=None):
        """One pass over the loader's batches: a training step (train) or an evaluation step per batch.  On one GPU and with
        nothing to do between steps (`per_step` None: no learning-rate scheduler) the full-sized batches go down in ONE call --
        dcv_mlp_train_steps / dcv_mlp_eval_steps: the epoch loop runs behind the C-ABI, and small networks are evaluated many
        batches per launch -- and the ragged last batch follows; launches, parameters and loss records are those of the
        step-by-step loop, bit for bit."""
        engine, k = self.calc.engine, 0
        if not self.calc.comm.active and per_step is None and len(plan) > 1:
            k = plan.full()
            if k > 0:
                many = engine.train_steps if train else engine.eval_steps
                if plan.kind == "idx":
                    many(Xn, plan.bs, k, idx=plan.base)
                else:
                    many(Xn, plan.bs, k, row0=plan.base)
        for b in plan[k:]:
            self.step(Xn, b, train)
            if per_step is not None:
                per_step()

    def epochs(self):
        """The epoch loop.  While the device works through the epoch just enqueued, the host draws the NEXT epoch's permutation
        and uploads its indices (a CPU randperm of 10 M indices is ~0.1 s -- as long as the epoch itself).  The draws keep the
        reference's order (train loader, validation loader, next train loader ...); whenever the loop ends with such a plan
        unused -- early stop, non-finite loss, any exception -- the generator is put back where the reference's would be."""
        c, sched = self.calc, self.sched
        # (a scheduler stepped per EPOCH -- lightning's default interval -- has nothing to do between the steps of an epoch)
        per_step = sched.after_step if sched is not None and sched.interval == "step" else None
        next_tb, rng_before_prefetch = None, None
        try:
            for epoch in range(c.max_epochs):
                tb = next_tb if next_tb is not None else self.batches(self.train_part)
                next_tb, rng_before_prefetch = None, None
                do_val = (epoch + 1) % c.check_val_every_n_epoch == 0
                vb = c._epoch_begin(epoch, tb, lambda: self.batches(self.val_part) if do_val else [])
                c.engine.reset_log(len(tb) + len(vb))
                self.run_batches(self.Xn_train, tb, True, per_step)
                self.run_batches(self.Xn_val, vb, False)
                if c.shuffle and epoch + 1 < c.max_epochs:
                    rng_before_prefetch = torch.get_rng_state()
                    next_tb = self.batches(self.train_part)
                rec = c.engine.read_log()   # waits for the epoch; the hooks and checkpoints below may read the device again
                if not np.all(np.isfinite(rec[:, 0])):
                    raise FloatingPointError("non-finite loss (ill-conditioned batch covariance?)")
                stop = do_val and self.validated(epoch, rec[:len(tb)], rec[len(tb):])
                if sched is not None:
                    sched.after_epoch(self.last_valid)
                if stop:
                    break
        finally:
            if next_tb is not None:
                torch.set_rng_state(rng_before_prefetch)

    def snapshot(self, buffers) -> Dict:
        """The model state a checkpoint keeps (one device read of the parameters)."""
        engine, p = self.calc.engine, self.plan
        return {"linears": engine.get_linears(), "tica": buffers, "dims": p.dims, "acts": p.acts, "drops": p.drops, "latent": p.latent,
                "bn": engine.get_bn() if any(p.bn) else None}

    def validated(self, epoch: int, rec_train: np.ndarray, rec_val: np.ndarray) -> bool:
        """Metrics, hooks, checkpoint and early-stopping bookkeeping after a validation pass; True = stop."""
        c, metrics = self.calc, self.metrics
        train_loss, _, _ = c._records_to_metrics(rec_train, need_eig=False)   # (only validation logs eigenvalues)
        valid_loss, eig, buffers = c._records_to_metrics(rec_val)
        self.last_valid = valid_loss
        metrics["train_loss"].append(train_loss)
        metrics["valid_loss"].append(valid_loss)
        metrics["epoch"].append(epoch)
        if self.sched is not None:
            metrics["lr"].append(self.sched.lr())
        snapshot = functools.cache(lambda: self.snapshot(buffers))   # at most one per validation, shared by the hook and the checkpoint
        c._on_validation(epoch, rec_train, rec_val, metrics, snapshot)
        if self.sched is not None:
            self.sched.on_validation_end(epoch, valid_loss)
        if eig is not None:
            for i, v in enumerate(eig):
                metrics.setdefault(f"valid_eigval_{i + 1}", []).append(float(v))
        if (epoch + 1) % c.save_check_every_n_epoch == 0:
            self.last_state = snapshot()
            if valid_loss < self.best_score:
                self.best_score, self.best_state = valid_loss, self.last_state
        if valid_loss < self.es_best - c.early_stop_delta:
            self.es_best, self.wait = valid_loss, 0
            return False
        self.wait += 1
        return self.wait >= c.early_stop_patience
