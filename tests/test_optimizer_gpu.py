"""The optimiser updates and the gradient reductions they are fused into (csrc/reduce_quad.h, csrc/mlp_opt.hip, csrc/ride.hip)
against torch.optim in float64 GIVEN THE GRADIENT: the engine runs its steps, the gradient buffer is copied after each (the
reductions store the gradient before the fused update), and those float32 gradients drive torch's optimiser over the same start
(tests/optimizer_oracle.py).  Parameters and every optimiser state tensor must agree within 4 x the deviation of torch's own
float32 run from its float64 run on the same gradients, a tolerance about fifty times below the end-to-end comparison of
tests/test_training_options_gpu.py, and every hyper-parameter of a case must be visible at it.  Each test asserts from
last_path / last_ride / last_reduce that the step took the kernels it is about.
Run on the GPU box: python -m pytest tests -m gpu"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import optimizer_oracle as oo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = oo.STEPS
BLOCK_DIMS, BLOCK_BATCH, BLOCK_LAG = [40, 264, 36, 3], 300, 5   # a width above 256: the block engine, whatever the process's environment
STRIDE_DIMS = [512, 520, 40, 3]                                   # 287 923 parameters: optimizer_kernel's grid is capped (1024 blocks of 256), its loop strides
WAVE16_DIMS, WAVE16_BATCH, WAVE16_LAG = [64, 128, 128, 3], 16500, 10
CASE_INDEX = {oo.case_id(c): i for i, c in enumerate(oo.CASES)}
ADAM_AMSGRAD, RPROP, RMSPROP_CENTERED, ASGD = (CASE_INDEX[k] for k in (
    "Adam-amsgrad-betas=(0.8,0.99)", "Rprop-etas=(0.5,1.2)-step_sizes=(0.0004,0.002)", "RMSprop-momentum=0.5-centered", "ASGD-lambd=0.001"))
ADAM_WD, ADADELTA, NADAM, SGD_NESTEROV = (CASE_INDEX[k] for k in (
    "Adam-weight_decay=0.001", "Adadelta-rho=0.9-weight_decay=0.0001", "NAdam-momentum_decay=1.0", "SGD-momentum=0.9-nesterov-weight_decay=0.0001"))


# ----------------------------------------------------------------------------- running the engine
def real_mask(eng):
    """True at the elements of the flat parameter buffer that belong to a weight, a bias or a normalisation's weight / bias."""
    mask = np.zeros(eng.n_params, dtype=bool)
    for l in range(eng.L):
        wo, bo = eng.offsets[l]
        mask[wo:wo + eng.dims[l + 1] * eng.in_dims[l]] = True
        mask[bo:bo + eng.dims[l + 1]] = True
        if eng.batchnorm[l]:
            for o in eng.bn_offsets[l]:
                mask[o:o + eng.dims[l + 1]] = True
    return mask


def make_engine(model, dims, acts, case, **extra):
    """The engine for torch.optim.<name>(**kwargs), its keyword arguments through the calculators' own mapping."""
    from deep_cartograph_amd import hip
    from deep_cartograph_amd.cv_calculator import NonLinear, _OPTIMIZERS

    name, kw = case
    ek = NonLinear._engine_optimizer_kwargs(name, {**_OPTIMIZERS[name], **kw})
    return hip.Mlp(model, dims, acts, optimizer=ek.pop("optimizer"), **ek, **extra)


def start_linears(dims, seed):
    torch.manual_seed(seed)
    return [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]


@functools.lru_cache(maxsize=None)
def features(n, F, seed):
    from tests.test_mlp_gpu import ar_features_fast, normalized

    return torch.from_numpy(normalized(ar_features_fast(n, F, seed))[0]).cuda()


def record(eng, X, batch, steps, fused=True, lrs=None, momenta=None, stride=97):
    """`steps` training steps on rows that move by `stride` per step; fused: dcv_mlp_train_step, else forward + backward +
    apply.  Returns the start, the gradient of every step, the end and the optimiser's state as float32 arrays over the flat
    buffer, and what the engine says about the path of every step."""
    mask = real_mask(eng)
    out = {"mask": mask, "p0": eng.params_view().cpu().numpy().copy(), "grads": [], "path": [], "ride": [], "reduce": []}
    span = X.shape[0] - batch - 64   # (64: more than any lag here)
    assert span >= 1
    for i in range(steps):
        r0 = (i * stride) % span
        if lrs is not None:
            eng.set_lr(lrs[i])
        if momenta is not None:
            eng.set_momentum(momenta[i])
        if fused:
            eng.train_step(X, row0=r0, batch=batch)
        else:
            eng.forward(X, row0=r0, batch=batch, train=True)
            eng.backward(X, row0=r0, batch=batch)
        out["grads"].append(eng.grads_view().cpu().numpy().copy())
        out["path"].append(eng.last_path())
        out["ride"].append(eng.last_ride())
        out["reduce"].append(eng.last_reduce())
        if not fused:
            eng.apply()
    out["grads"] = np.stack(out["grads"])
    out["params"] = eng.params_view().cpu().numpy().copy()
    for k in range(3):
        v = eng.opt_state_view(k)
        if v is not None:
            out[f"state{k}"] = v.cpu().numpy().copy()
    assert np.isfinite(out["grads"]).all() and np.isfinite(out["params"]).all()
    return out


def block_record(i, fused=True, dims=None, batchnorm=None, steps=T, lrs=None, momenta=None, case=None):
    dims = dims or BLOCK_DIMS
    eng = make_engine("deep_tica", dims, ["tanh"] * (len(dims) - 2) + [None], case or oo.CASES[i], max_batch=BLOCK_BATCH, lag=BLOCK_LAG, tica_reg=1e-6,
                      batchnorm=batchnorm)
    lins = [(l.weight.detach().numpy(), l.bias.detach().numpy()) for l in start_linears(dims, 3)]
    bn = None
    if batchnorm is not None:   # not the trivial weight 1 / bias 0
        g = torch.Generator().manual_seed(9)
        bn = [dict(weight=(torch.rand(dims[l + 1], generator=g) + 0.5).numpy(), bias=(torch.rand(dims[l + 1], generator=g) * 0.6 - 0.3).numpy()) if b else None
              for l, b in enumerate(batchnorm)]
    eng.set_linears(lins, bn=bn)
    eng.reset_log(steps + 1)
    out = record(eng, features(2048, dims[0], 23), BLOCK_BATCH, steps, fused=fused, lrs=lrs, momenta=momenta)
    eng.close()
    return out


@functools.lru_cache(maxsize=None)
def fused_block_record(i):
    return block_record(i)


def small_record(i):
    """The autoencoder of test_optimizers_follow_torch: the fused small-network launch, whose reduction is the flat-grid kernel."""
    from tests.test_mlp_gpu import ar_features, normalized

    F, batch = 24, 512
    dims, acts = [F, 12, 2, 12, F], ["tanh", None, "tanh", None]
    Xn, _, r = normalized(ar_features(1600, F, 23))
    eng = make_engine("ae", dims, acts, oo.CASES[i], max_batch=batch, latent_layer=2)
    eng.set_linears([(l.weight.detach().numpy(), l.bias.detach().numpy()) for l in start_linears(dims, 31)])
    eng.set_feature_range(r)
    eng.reset_log(T + 1)
    out = record(eng, torch.from_numpy(Xn).cuda(), batch, T)
    eng.close()
    return out


# ----------------------------------------------------------------------------- comparing with the oracle
def check(case, rec, label, lrs=None, momenta=None):
    """Parameters and state of the record against the float64 oracle on the record's own gradients; the padding of the
    parameter buffer; the visibility of the case's hyper-parameters on these gradients.  Prints every figure before it asserts."""
    name, kw = case
    idx = torch.from_numpy(np.flatnonzero(rec["mask"]))
    pick = lambda a: torch.from_numpy(np.asarray(a))[idx]
    ref = oo.Reference(name, kw, pick(rec["p0"]), [pick(g) for g in rec["grads"]], lrs, momenta)
    failures = []
    for k, key in enumerate(("params",) + oo.STATE_MAP[name]):
        if key is None or key not in ref.ref:
            continue
        got = rec["params"] if k == 0 else rec.get(f"state{k - 1}")
        assert got is not None, f"{label}: the engine holds no state tensor {k - 1} for torch's {key}"
        dev, ratio = ref.deviation(key, pick(got))
        print(f"RATIO {label} | {oo.case_id(case)} | {key} | engine {dev:.3e} float32-torch {ref.dev32[key]:.3e} ratio {ratio:.2f} tol {ref.tol[key]:.3e}")
        if not dev <= ref.tol[key]:
            failures.append(f"{key}: {dev:.3e} > {ref.tol[key]:.3e} (ratio {ratio:.2f})")
    pad = rec["params"][~rec["mask"]]
    seen = ref.sensitivity()
    print(f"VISIBLE {label} | {oo.case_id(case)} | {seen}")
    assert not failures, f"{label} {oo.case_id(case)}: " + "; ".join(failures)
    assert pad.size == 0 or not pad.any(), f"{label}: alignment padding of the parameters was written"
    for k, frac in seen.items():
        assert frac >= oo.MIN_FRACTION, f"{label} {oo.case_id(case)}: {k} moves only {frac:.1%} of the elements by more than {oo.VISIBLE} x tol"


def assert_same_bits(a, b, what):
    """Gradients, parameters and state of two records, bit for bit over the weights, biases and normalisation parameters.  (Not
    over the alignment padding between them: optimizer_kernel walks the whole buffer and leaves the state of a zero parameter
    with a zero gradient there -- Adamax's exp_inf = eps, Rprop's prev = -0 under maximize -- where the reductions touch nothing;
    check() holds the padding of the parameters themselves to zero.)"""
    assert np.array_equal(a["mask"], b["mask"])
    m = a["mask"]
    for key in ("grads", "params", "state0", "state1", "state2"):
        assert (key in a) == (key in b), (what, key)
        if key in a:
            x, y = np.ascontiguousarray(a[key][..., m]), np.ascontiguousarray(b[key][..., m])
            assert x.tobytes() == y.tobytes(), f"{what}: {key} differs in {int(np.sum(x.view(np.uint32) != y.view(np.uint32)))} elements"


# ----------------------------------------------------------------------------- the paths
@pytest.mark.parametrize("i", range(len(oo.CASES)), ids=[oo.case_id(c) for c in oo.CASES])
def test_block_engine_fused_and_riding(i):
    """Every gradient but layer 0's weights is reduced and updated by blocks riding in the layer-0 weight-gradient launch
    (ride.hip), those weights by the flat-grid reduction behind it."""
    rec = fused_block_record(i)
    assert rec["path"] == [0] * T and all(r > 0 for r in rec["ride"]) and rec["reduce"] == [1] * T, (rec["path"], rec["ride"], rec["reduce"])
    check(oo.CASES[i], rec, "block-fused")


@pytest.mark.parametrize("i", range(len(oo.CASES)), ids=[oo.case_id(c) for c in oo.CASES])
def test_small_network_fused(i):
    rec = small_record(i)
    assert rec["path"] == [1] * T and rec["ride"] == [0] * T and rec["reduce"] == [1] * T, (rec["path"], rec["ride"], rec["reduce"])
    check(oo.CASES[i], rec, "small-network")


@pytest.mark.parametrize("i", range(len(oo.CASES)), ids=[oo.case_id(c) for c in oo.CASES])
def test_unfused_apply_equals_the_fused_step(i):
    """forward + backward + apply(): the reduction without the update, then optimizer_kernel -- the bits of the fused step."""
    rec = block_record(i, fused=False)
    assert rec["path"] == [0] * T and rec["ride"] == [0] * T and rec["reduce"] == [1] * T, (rec["path"], rec["ride"], rec["reduce"])
    check(oo.CASES[i], rec, "block-unfused")
    assert_same_bits(rec, fused_block_record(i), oo.case_id(oo.CASES[i]))


@pytest.mark.parametrize("i", [ADAM_AMSGRAD, RPROP, RMSPROP_CENTERED], ids=lambda i: oo.case_id(oo.CASES[i]))
def test_grid_stride_optimizer_kernel(i):
    """More than 262 144 parameters: optimizer_kernel's thread loop runs more than once.  Three uses of the state tensors."""
    unfused = block_record(i, fused=False, dims=STRIDE_DIMS)
    assert unfused["mask"].size > 1024 * 256 and unfused["path"] == [0] * T and unfused["ride"] == [0] * T, (unfused["mask"].size, unfused["path"], unfused["ride"])
    check(oo.CASES[i], unfused, "grid-stride-unfused")
    fused = block_record(i, dims=STRIDE_DIMS)
    assert fused["path"] == [0] * T and all(r > 0 for r in fused["ride"]) and fused["reduce"] == [1] * T, (fused["path"], fused["ride"], fused["reduce"])
    check(oo.CASES[i], fused, "grid-stride-fused")
    assert_same_bits(unfused, fused, oo.case_id(oo.CASES[i]))


@pytest.mark.parametrize("i", [ADAM_WD, ADADELTA, NADAM], ids=lambda i: oo.case_id(oo.CASES[i]))
def test_batchnorm_parameters(i):
    """Weight and bias of a batch normalisation are parameters like any other: their reduction items ride too."""
    rec = block_record(i, batchnorm=[True, False, False])
    assert int(rec["mask"].sum()) == sum(a * b + b for a, b in zip(BLOCK_DIMS[:-1], BLOCK_DIMS[1:])) + 2 * BLOCK_DIMS[1]
    assert rec["path"] == [0] * T and all(r > 0 for r in rec["ride"]) and rec["reduce"] == [1] * T, (rec["path"], rec["ride"], rec["reduce"])
    check(oo.CASES[i], rec, "batchnorm")


@pytest.mark.parametrize("case", [("Adam", dict(lr=1e-3, betas=(0.9, 0.99))), ("SGD", dict(lr=0.02, momentum=0.9))], ids=oo.case_id)
def test_scheduler_sets_lr_and_momentum_before_every_step(case):
    """OneCycleLR(cycle_momentum=True) over torch's own optimiser gives lr and beta1 / momentum of every step; the engine takes
    them through set_lr / set_momentum, the oracle through its parameter group."""
    name, kw = case
    dummy = getattr(torch.optim, name)([torch.nn.Parameter(torch.zeros(1))], **kw)
    sched = torch.optim.lr_scheduler.OneCycleLR(dummy, max_lr=5 * kw["lr"], total_steps=T, cycle_momentum=True, base_momentum=0.8, max_momentum=0.95)
    lrs, momenta = [], []
    for t in range(T):
        g = dummy.param_groups[0]
        lrs.append(float(g["lr"]))
        momenta.append(float(g["betas"][0] if "betas" in g else g["momentum"]))
        dummy.step()
        if t + 1 < T:
            sched.step()
    assert max(lrs) > 3 * min(lrs) and max(momenta) - min(momenta) > 0.1
    rec = block_record(None, case=case, lrs=lrs, momenta=momenta)
    assert rec["path"] == [0] * T and all(r > 0 for r in rec["ride"]) and rec["reduce"] == [1] * T, (rec["path"], rec["ride"], rec["reduce"])
    check(case, rec, "scheduler", lrs=lrs, momenta=momenta)
    # the schedule itself is visible: the oracle at the constant lr / momentum of creation lands elsewhere
    idx = np.flatnonzero(rec["mask"])
    flat, _ = oo.run_torch(name, kw, torch.from_numpy(rec["p0"][idx]), [torch.from_numpy(g[idx]) for g in rec["grads"]], torch.float64)
    ref = oo.Reference(name, kw, torch.from_numpy(rec["p0"][idx]), [torch.from_numpy(g[idx]) for g in rec["grads"]], lrs, momenta)
    assert float(((flat - ref.ref["params"]).abs() > oo.VISIBLE * ref.tol["params"]).double().mean()) >= oo.MIN_FRACTION


# ----------------------------------------------------------------------------- the 16-wave reduction
@functools.lru_cache(maxsize=None)
def wave16_record(i):
    dims = WAVE16_DIMS
    eng = make_engine("deep_tica", dims, ["tanh", "tanh", None], oo.CASES[i], max_batch=WAVE16_BATCH, lag=WAVE16_LAG, tica_reg=1e-6)
    eng.set_linears([(l.weight.detach().numpy(), l.bias.detach().numpy()) for l in start_linears(dims, 3)])
    eng.reset_log(4)
    out = record(eng, features(WAVE16_BATCH + WAVE16_LAG + 64 + 3 * 7, dims[0], 29), WAVE16_BATCH, 3, stride=7)
    eng.close()
    return out


def _assert_wave16(rec):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # head_plan (csrc/mlp_heads.hip): the fused backward of the narrow last layer leaves ceil(R / 32) partials, R = batch + lag
    # shared rows, up to 4 per CU: 516 here from 129 CUs up -- more than the 512 the flat-grid and 4-wave kernels take
    assert rec["path"] == [0] * 3 and rec["reduce"] == [3] * 3 and rec["ride"] == [0] * 3, \
        f"the 16-wave reduction did not run on {cus} CUs: path {rec['path']} reduce {rec['reduce']} ride {rec['ride']}"


def test_wave16_reduction_gradients_match_float64_autograd():
    """The first step's gradients, summed by reduce_grads_kernel from 516 partials, against a float64 run of the autograd
    oracle on the same rows, at the bound of test_deeptica_step_matches_autograd (2e-5 of the largest entry per tensor)."""
    import copy

    from oracle import nn as onn
    from tests.test_mlp_gpu import linears_of, rel_err

    rec = wave16_record(ADAM_WD)
    _assert_wave16(rec)
    dims, B, lag = WAVE16_DIMS, WAVE16_BATCH, WAVE16_LAG
    ref = onn.DeepTICAModel(dims, ["tanh", "tanh", None], None, None, None, 1e-6).double()
    lins = linears_of(ref.nn)
    with torch.no_grad():
        for lin, src in zip(lins, start_linears(dims, 3)):
            lin.weight.copy_(src.weight.double())
            lin.bias.copy_(src.bias.double())
    X = features(B + lag + 64 + 3 * 7, dims[0], 29).cpu().double()
    loss, _ = ref.step(X[:B], X[lag:lag + B])
    loss.backward()
    g, off = rec["grads"][0], 0
    for l, lin in enumerate(lins):   # the flat layout: weight, bias of every layer, each aligned to 4 floats
        gw, gb = lin.weight.grad.numpy(), lin.bias.grad.numpy()
        ew = rel_err(g[off:off + gw.size].reshape(gw.shape), gw)
        off += -(-gw.size // 4) * 4
        got_b = g[off:off + gb.size]
        off += -(-gb.size // 4) * 4
        print(f"wave16 layer {l}: weight gradient {ew:.2e} of the largest entry")
        assert ew < 2e-5, f"layer {l} weight: {ew:.2e}"
        if l < len(lins) - 1:
            eb = rel_err(got_b, gb)
            assert eb < 2e-5, f"layer {l} bias: {eb:.2e}"
        else:   # exactly zero by the mean removal: rounding noise only
            assert np.max(np.abs(got_b)) < 2e-5 * max(1.0, np.max(np.abs(gw))), f"layer {l} bias"
    assert off == g.size


@pytest.mark.parametrize("i", [ADAM_WD, SGD_NESTEROV], ids=lambda i: oo.case_id(oo.CASES[i]))
def test_wave16_reduction_fused_update(i):
    rec = wave16_record(i)
    _assert_wave16(rec)
    check(oo.CASES[i], rec, "wave16")


# ----------------------------------------------------------------------------- the 4-wave reduction
_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, {root!r})
from tests import test_optimizer_gpu as t
out = {{}}
for i in t.WAVE4_CASES:
    rec = t.block_record(i)
    for k, v in rec.items():
        out[f"{{i}}_{{k}}"] = np.asarray(v)
np.savez(sys.argv[1], **out)
"""
WAVE4_CASES = [ADAM_AMSGRAD, RPROP, ASGD]


def test_wave4_reduction_fused_update(tmp_path):
    """DCV_REDUCE_QUAD=0 (read once per process: a fresh child) sends every reduction to reduce_grads_small_kernel."""
    script, npz = tmp_path / "wave4_run.py", tmp_path / "wave4.npz"
    script.write_text(_CHILD.format(root=ROOT))
    env = dict(os.environ)
    env["DCV_REDUCE_QUAD"] = "0"
    p = subprocess.Popen([sys.executable, str(script), str(npz)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        _, err = p.communicate(timeout=180)
        assert p.returncode == 0, err[-2000:]
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
    data = np.load(npz)
    for i in WAVE4_CASES:
        rec = {k[len(f"{i}_"):]: data[k] for k in data.files if k.startswith(f"{i}_")}
        assert rec["path"].tolist() == [0] * T and rec["reduce"].tolist() == [2] * T and rec["ride"].tolist() == [0] * T, (rec["path"], rec["reduce"], rec["ride"])
        check(oo.CASES[i], rec, "wave4")
