"""Given-gradient oracle of the engine's optimiser updates (csrc/reduce_quad.h: opt_update_p, csrc/mlp_opt.hip: next_opt_args):
torch.optim itself, single-tensor form, over ONE flat CPU parameter tensor whose gradient of every step is handed in -- no model,
no autograd.  Run in float64 it is the reference; run in float32 on the same start and gradients it measures how far a correct
float32 implementation strays from that reference, which is where the tolerance of every comparison comes from (FACTOR times that
deviation, per tensor) -- never from what the engine computes.

CASES are the optimiser configurations the tests run, NEUTRAL the value at which each hyper-parameter does nothing.  A case is
only worth running when each of its hyper-parameters is visible at the tolerance (sensitivity): with the hyper-parameter at its
neutral value the float64 oracle must move at least MIN_FRACTION of the elements by more than VISIBLE x tol."""
import inspect
import math

import numpy as np
import torch

STEPS = 12          # RAdam's rho_t crosses 5 at step 6: both of its branches run
FACTOR = 4.0        # the engine contracts to fmaf and rounds in another order than torch's op-by-op kernels: both are float32 walks of the same length
VISIBLE = 10.0      # a neutralised hyper-parameter must move an element by more than VISIBLE x tol ...
MIN_FRACTION = 0.1  # ... on at least this fraction of the elements

# (torch.optim class, keyword arguments).  The first 19 are the cases of tests/test_training_options_gpu.py, two of them changed
# because a hyper-parameter was invisible at any float32 tolerance (NAdam's momentum_decay at torch's default 4e-3; the weight
# decay of the maximising SGD at lr 1e-4), ASGD without its explicit alpha = 0.75 (torch's default, and with lambd 1e-3 the
# exponent of a factor 1 + 2e-5 t: the second ASGD case below carries an alpha that acts), Rprop with step bounds that bind
# within 12 steps (1e-3 x 1.2^11 stays below 1e-2).  The rest are flag combinations those 19 leave out.
CASES = [
    ("Adam", dict(lr=2e-3, weight_decay=1e-3)),
    ("Adam", dict(lr=1e-3, amsgrad=True, betas=(0.8, 0.99))),
    ("AdamW", dict(lr=2e-3, weight_decay=0.05)),
    ("SGD", dict(lr=0.05)),
    ("SGD", dict(lr=0.02, momentum=0.9, nesterov=True, weight_decay=1e-4)),
    ("SGD", dict(lr=0.02, momentum=0.8, dampening=0.1)),
    ("RMSprop", dict(lr=1e-3, momentum=0.5, centered=True)),
    ("RMSprop", dict(lr=2e-3, alpha=0.9, weight_decay=1e-3)),
    ("Adagrad", dict(lr=0.02, lr_decay=0.01, initial_accumulator_value=0.1)),
    ("Adamax", dict(lr=2e-3, weight_decay=1e-3)),
    ("NAdam", dict(lr=2e-3, momentum_decay=1.0)),
    ("NAdam", dict(lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True)),
    ("RAdam", dict(lr=2e-3)),
    ("RAdam", dict(lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True, betas=(0.9, 0.9))),
    ("Adadelta", dict(lr=1.0, rho=0.9, weight_decay=1e-4)),
    ("ASGD", dict(lr=0.02, lambd=1e-3)),
    ("Rprop", dict(lr=1e-3, etas=(0.5, 1.2), step_sizes=(4e-4, 2e-3))),
    ("Adam", dict(lr=1e-3, maximize=True)),
    ("SGD", dict(lr=0.01, weight_decay=0.02, maximize=True)),
    # flag combinations no case above has
    ("AdamW", dict(lr=2e-3, weight_decay=0.05, amsgrad=True, betas=(0.8, 0.9))),
    ("Adagrad", dict(lr=0.02, weight_decay=0.01)),
    ("RMSprop", dict(lr=1e-3, centered=True)),
    ("Adamax", dict(lr=2e-3, betas=(0.8, 0.99))),
    ("NAdam", dict(lr=2e-3, weight_decay=0.01)),
    ("RAdam", dict(lr=1e-3, weight_decay=0.01, betas=(0.9, 0.9))),
    ("Rprop", dict(lr=1e-3, etas=(0.4, 1.3), step_sizes=(4e-4, 2e-3), maximize=True)),
    ("Adadelta", dict(lr=1.0, rho=0.8, maximize=True)),
    ("ASGD", dict(lr=0.02, lambd=0.5, alpha=0.5, weight_decay=0.01)),
]
N_PRESENT = 19   # the leading cases that tests/test_training_options_gpu.py also runs (end to end, at its own tolerance)


def case_id(case):
    name, kw = case
    return name + "-" + "-".join(k if v is True else f"{k}={v}" for k, v in kw.items() if k != "lr").replace(" ", "")


# The value at which a hyper-parameter does nothing: no decay, no averaging, no momentum, no flag, step sizes that never change
# (torch.optim.Rprop refuses etas of exactly 1) and are never clipped.  (`maximize` has no such value: the sensitivity check flips it.)
NEUTRAL = {
    "weight_decay": 0.0, "dampening": 0.0, "lr_decay": 0.0, "momentum_decay": 0.0, "lambd": 0.0, "momentum": 0.0,
    "initial_accumulator_value": 0.0, "alpha": 0.0, "rho": 0.0, "betas": (0.0, 0.0), "etas": (1.0 - 1e-12, 1.0 + 1e-12), "step_sizes": (0.0, math.inf),
    "amsgrad": False, "nesterov": False, "centered": False, "decoupled_weight_decay": False,
}

# engine state tensor 0 / 1 / 2 (dcv_mlp_opt_state) -> torch's name in optimizer.state[p] (csrc/reduce_quad.h); a name the
# torch run does not hold (no momentum, no amsgrad, not centered) is a tensor the engine does not use
STATE_MAP = {
    "Adam": ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"),
    "AdamW": ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"),
    "SGD": ("momentum_buffer", None, None),
    "RMSprop": ("momentum_buffer", "square_avg", "grad_avg"),
    "Adagrad": (None, "sum", None),
    "Adamax": ("exp_avg", "exp_inf", None),
    "NAdam": ("exp_avg", "exp_avg_sq", None),
    "RAdam": ("exp_avg", "exp_avg_sq", None),
    "Adadelta": ("square_avg", "acc_delta", None),
    "ASGD": (None, None, None),   # eta lives on the host, the averaged copy ax is not kept
    "Rprop": ("prev", "step_size", None),
}


def run_torch(name, kwargs, p0, grads, dtype, lrs=None, momenta=None):
    """len(grads) steps of torch.optim.<name>(**kwargs) over one flat parameter tensor starting at p0, step t on grads[t];
    lrs[t] / momenta[t] (optional) are written into the parameter group before step t, as a scheduler does (momenta: betas[0]
    of the Adam family, momentum of SGD / RMSprop).  Returns (parameters, {torch's state name: tensor}) in `dtype`."""
    cls = getattr(torch.optim, name)
    kw = dict(kwargs)
    if "foreach" in inspect.signature(cls.__init__).parameters:
        kw["foreach"] = False
    p = torch.nn.Parameter(torch.as_tensor(p0).detach().to(dtype).clone())
    opt = cls([p], **kw)
    group = opt.param_groups[0]
    for t in range(len(grads)):
        if lrs is not None:
            group["lr"] = float(lrs[t])
        if momenta is not None:
            if "betas" in group:
                group["betas"] = (float(momenta[t]), group["betas"][1])
            else:
                group["momentum"] = float(momenta[t])
        p.grad = torch.as_tensor(grads[t]).detach().to(dtype).clone()
        opt.step()
    state = {k: v.detach().clone() for k, v in opt.state[p].items() if torch.is_tensor(v) and v.shape == p.shape}
    return p.detach().clone(), state


class Reference:
    """The float64 run of a case on given gradients, and per tensor ("params" and torch's state names) the deviation of the
    float32 run from it (dev32) and the tolerance FACTOR x dev32."""

    def __init__(self, name, kwargs, p0, grads, lrs=None, momenta=None):
        self.name, self.kwargs, self.p0, self.grads, self.lrs, self.momenta = name, kwargs, p0, grads, lrs, momenta
        p64, s64 = run_torch(name, kwargs, p0, grads, torch.float64, lrs, momenta)
        p32, s32 = run_torch(name, kwargs, p0, grads, torch.float32, lrs, momenta)
        assert set(s64) == set(s32)
        self.ref = {"params": p64, **s64}
        self.dev32 = {k: float((dict(params=p32, **s32)[k].double() - v).abs().max()) for k, v in self.ref.items()}
        self.tol = {k: FACTOR * d for k, d in self.dev32.items()}
        for k, v in self.ref.items():
            assert bool(torch.isfinite(v).all()), (name, kwargs, k)

    def deviation(self, key, got):
        """max |got - float64 reference| of tensor `key` and its ratio to the float32 run's deviation."""
        dev = float((torch.as_tensor(got).double() - self.ref[key]).abs().max())
        d32 = self.dev32[key]
        return dev, (dev / d32 if d32 > 0 else (0.0 if dev == 0 else math.inf))

    def sensitivity(self):
        """{hyper-parameter: fraction of the parameters that the float64 oracle moves by more than VISIBLE x tol when the
        hyper-parameter takes its neutral value (`maximize`: is flipped)}, over every keyword of the case but lr."""
        out = {}
        for k in self.kwargs:
            if k == "lr":
                continue
            kw = dict(self.kwargs)
            kw[k] = (not kw[k]) if k == "maximize" else NEUTRAL[k]
            if k == "momentum":   # flags that torch refuses without momentum go with it
                kw.pop("nesterov", None)
                kw.pop("dampening", None)
            p, _ = run_torch(self.name, kw, self.p0, self.grads, torch.float64, self.lrs, None if k in ("momentum", "betas") else self.momenta)
            moved = (p - self.ref["params"]).abs() > VISIBLE * self.tol["params"]
            out[k] = float(moved.double().mean())
        return out


def synthetic_problem(n=4001, steps=STEPS, seed=5):
    """Start uniform in +-0.3; gradients N(0, 1e-2) 0.9^t + N(0, 3e-3) (a direction per element that decays, fresh noise each
    step); every 97th element has an exactly zero gradient throughout.  Float32 values: what an engine would hand over."""
    g = torch.Generator().manual_seed(seed)
    p0 = (torch.rand(n, generator=g, dtype=torch.float64) * 0.6 - 0.3).float()
    direction = torch.randn(n, generator=g, dtype=torch.float64) * 1e-2
    grads = []
    for t in range(steps):
        gt = direction * 0.9 ** t + torch.randn(n, generator=g, dtype=torch.float64) * 3e-3
        gt[::97] = 0.0
        grads.append(gt.float())
    return p0, grads


def np_flat(t):
    return np.ascontiguousarray(torch.as_tensor(t).detach().cpu().numpy())
