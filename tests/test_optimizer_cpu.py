"""The given-gradient optimiser oracle (tests/optimizer_oracle.py) by itself, on the CPU: every case it holds must make each of
its hyper-parameters visible at the tolerance the GPU tests compare at, otherwise an engine that ignored the hyper-parameter
would pass them (tests/test_optimizer_gpu.py asserts the same again on the engine's own gradients)."""
import inspect

import pytest
import torch

from tests import optimizer_oracle as oo


@pytest.fixture(scope="module")
def problem():
    return oo.synthetic_problem()


def test_cases_are_complete_and_constructible():
    """All eleven optimisers of the engine, the 19 cases of test_optimizers_follow_torch first, ids unique, every keyword one
    that torch.optim accepts and NEUTRAL knows, every state name of the map one that torch holds."""
    from deep_cartograph_amd.cv_calculator import _OPTIMIZERS

    assert {n for n, _ in oo.CASES} == set(_OPTIMIZERS) == set(oo.STATE_MAP)
    assert len({oo.case_id(c) for c in oo.CASES}) == len(oo.CASES) and len(oo.CASES) >= oo.N_PRESENT + 9
    p0, grads = oo.synthetic_problem(n=64, steps=2)
    for name, kw in oo.CASES:
        accepted = inspect.signature(getattr(torch.optim, name).__init__).parameters
        for k in kw:
            assert k in accepted and k in _OPTIMIZERS[name] or k == "maximize", (name, k)
            assert k in oo.NEUTRAL or k in ("lr", "maximize"), (name, k)
        full = {**kw, "amsgrad": True} if name in ("Adam", "AdamW") else {**kw, "momentum": 0.5, "centered": True} if name == "RMSprop" else \
            {**kw, "momentum": 0.5} if name == "SGD" else kw
        _, state = oo.run_torch(name, full, p0, grads, torch.float64)
        assert {s for s in oo.STATE_MAP[name] if s} <= set(state), (name, sorted(state))


def test_run_torch_takes_per_step_lr_and_momentum():
    p0, grads = oo.synthetic_problem(n=64, steps=3)
    a, _ = oo.run_torch("SGD", dict(lr=0.5, momentum=0.9), p0, grads, torch.float64, lrs=[0.1, 0.2, 0.3], momenta=[0.9, 0.5, 0.25])
    g = [x.double() for x in grads]
    b1 = g[0]
    b2 = 0.5 * b1 + g[1]
    b3 = 0.25 * b2 + g[2]
    torch.testing.assert_close(a, p0.double() - 0.1 * b1 - 0.2 * b2 - 0.3 * b3, rtol=0, atol=1e-15)
    c, st = oo.run_torch("Adam", dict(lr=1e-3), p0, grads[:1], torch.float64, momenta=[0.5])
    torch.testing.assert_close(st["exp_avg"], 0.5 * g[0], rtol=0, atol=1e-18)


@pytest.mark.parametrize("case", oo.CASES, ids=oo.case_id)
def test_every_hyperparameter_is_visible_at_the_tolerance(case, problem):
    name, kw = case
    p0, grads = problem
    ref = oo.Reference(name, kw, p0, grads)
    assert 0 < ref.tol["params"] < 1e-5, ref.tol   # a float32 walk of 12 steps: 1e-7 .. 1e-6
    seen = ref.sensitivity()
    print(oo.case_id(case), "tol", {k: f"{v:.2e}" for k, v in ref.tol.items()}, "moved", seen)
    assert set(seen) == set(kw) - {"lr"}
    for k, frac in seen.items():
        assert frac >= oo.MIN_FRACTION, f"{oo.case_id(case)}: {k} moves only {frac:.1%} of the elements by more than {oo.VISIBLE} x tol = {oo.VISIBLE * ref.tol['params']:.2e}"
