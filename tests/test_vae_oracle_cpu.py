"""tests/vae_oracle.py (NumPy float64, backward by hand) against torch float64 autograd of the same expression, and the case
tables of tests/test_vae_step_gpu.py: every case well conditioned, every claim of coverage counted."""
import numpy as np
import pytest
import torch

from tests import test_vae_step_gpu as gpu_cases
from tests import vae_oracle as vo

_TORCH_ACT = {None: lambda a: a, "none": lambda a: a, "tanh": torch.tanh, "elu": torch.nn.functional.elu,
              "leaky_relu": torch.nn.functional.leaky_relu}


def _autograd(lins, acts, latent, xn, eps, rng, beta):
    """The ELBO step in torch float64: (loss, recon, kl), the gradients in layer order, (dmu, dlv)."""
    p = [(torch.tensor(w, dtype=torch.float64, requires_grad=True), torch.tensor(b, dtype=torch.float64, requires_grad=True)) for w, b in lins]
    x, e, r = (torch.tensor(np.asarray(v), dtype=torch.float64) for v in (xn, eps, rng))
    h = x
    for l, (w, b) in enumerate(p):
        if l == latent:
            heads, d = h, h.shape[1] // 2
            heads.retain_grad()
            mu, lv = h[:, :d], h[:, d:]
            h = e * torch.exp(lv / 2) + mu
        h = _TORCH_ACT[acts[l]](h @ w.T + b)
    rec = ((h - x) * r).square().mean()
    kl = (-0.5 * (lv - lv.exp() - mu ** 2 + 1).sum(dim=1)).mean()
    loss = rec + beta * kl
    loss.backward()
    return (loss.item(), rec.item(), kl.item()), [(w.grad.numpy(), b.grad.numpy()) for w, b in p], heads.grad.numpy()


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / (np.max(np.abs(b)) + 1e-300))


@pytest.mark.parametrize("act", [None, "tanh", "elu", "leaky_relu"])
@pytest.mark.parametrize("beta", [0.0, 0.3])
@pytest.mark.parametrize("d", [1, 3, 8])
def test_hand_written_backward_matches_float64_autograd(d, beta, act):
    """A ragged batch of 37 rows through 20-12-2d-7-20 with the activation behind every Linear but the heads (the output
    Linear included): the three scalars, every gradient tensor and [dmu | dlv] to 1e-12 relative."""
    dims, acts, latent = [20, 12, 2 * d, 7, 20], [act, None, act, act], 2
    c = vo.case(dims, acts, latent, 50, 100 * d + (0 if act is None else len(act)))
    rows = np.random.Generator(np.random.PCG64(d)).permutation(50)[:37]
    xn, eps = c["Xn"][rows], c["eps"][5:42]
    o = vo.step(c["lins"], acts, latent, xn, eps, c["range"], beta)
    scalars, grads, dheads = _autograd(c["lins"], acts, latent, xn, eps, c["range"], beta)
    worst = 0.0
    for got, want in zip((o["loss"], o["recon"], o["kl"]), scalars):
        worst = max(worst, abs(got - want) / abs(want))
    assert o["loss"] == o["recon"] + beta * o["kl"]
    assert abs(o["SSE"] / (37 * 20) - o["recon"]) <= 1e-15 * o["recon"] and abs(o["KL"] / 37 - o["kl"]) <= 1e-15 * abs(o["kl"])
    for (gw, gb), (tw, tb) in zip(o["grads"], grads):
        assert gw.shape == tw.shape and gb.shape == tb.shape
        worst = max(worst, _rel(gw, tw), _rel(gb, tb))
    worst = max(worst, _rel(np.concatenate([o["dmu"], o["dlv"]], axis=1), dheads))
    print(f"d={d} beta={beta} {act}: worst deviation from float64 autograd {worst:.2e}")
    assert worst < 1e-12


def test_forward_is_the_forward_of_step():
    c = vo.case([33, 12, 6, 7, 33], ["elu", None, "leaky_relu", None], 2, 40, 5)
    f = vo.forward(c["lins"], c["acts"], 2, c["Xn"], c["eps"], c["range"], 0.3)
    s = vo.step(c["lins"], c["acts"], 2, c["Xn"], c["eps"], c["range"], 0.3)
    assert all(f[k] == s[k] for k in ("loss", "recon", "kl", "SSE", "KL")) and np.array_equal(f["z"], s["z"])


def test_builder_refuses_an_ill_conditioned_case():
    with pytest.raises(AssertionError, match="KL per row"):   # torch.nn.Linear's own scale on a narrow head input: KL ~ 0.01
        vo.case([20, 4, 2, 12, 20], ["tanh", None, "tanh", None], 2, 64, 1, head_gain=0.25)
    with pytest.raises(AssertionError, match="lv"):
        vo.case([20, 12, 6, 12, 20], ["tanh", None, "tanh", None], 2, 64, 1, lv_shift=13.0)


def _well_conditioned(o, what):
    """The builder's conditions on the rows the GPU test really runs."""
    assert o["kl"] >= 0.05, f"{what}: KL per row {o['kl']:.3g}"
    assert np.max(np.abs(o["lv"])) <= 12.0, f"{what}: max |lv| {np.max(np.abs(o['lv'])):.3g}"
    assert all(np.isfinite(v) for v in (o["loss"], o["recon"], o["kl"]))


@pytest.mark.parametrize("table", ["fused", "layer", "large_lv", "eval"])
def test_gpu_cases_are_well_conditioned(table):
    """vae_oracle.case asserts mean KL per row >= 0.05 and max |lv| <= 12 on the whole matrix while it builds each case;
    here the same on the batch each GPU test runs, and every oracle gradient tensor has an entry to be relative to."""
    lo_kl, hi_lv = np.inf, 0.0
    if table == "eval":
        for key, d, batch, form, path, tr in gpu_cases.EVAL_CASES:
            c = gpu_cases.prepare_eval(key, d, batch, form)
            for j, o in enumerate(c["o"]):
                _well_conditioned(o, f"{key} d={d} batch {j}")
                lo_kl, hi_lv = min(lo_kl, o["kl"]), max(hi_lv, float(np.max(np.abs(o["lv"]))))
    else:
        if table == "fused":
            cases = [gpu_cases.prepare_step(k, d, b, f, beta, cur) for k, d, b, f, beta, cur, tr in gpu_cases.FUSED_CASES]
        elif table == "layer":
            cases = [gpu_cases.prepare_step(k, d, b, f, beta) for k, d, b, f, beta in gpu_cases.LAYER_CASES]
        else:
            cases = [gpu_cases.prepare_step(k, 3, b, "idx", 1.0, lv_shift=s) for k, path, b, s in gpu_cases.LARGE_LV_CASES]
        for c in cases:
            what = f"{c['dims']} batch {c['batch']}"
            _well_conditioned(c["o"], what)
            for l, (gw, gb) in enumerate(c["o"]["grads"]):
                assert np.max(np.abs(gw)) > 1e-8 and np.max(np.abs(gb)) > 1e-8, f"{what}: layer {l} has no gradient to compare with"
            lo_kl, hi_lv = min(lo_kl, c["o"]["kl"]), max(hi_lv, float(np.max(np.abs(c["o"]["lv"]))))
    print(f"{table}: smallest KL per row {lo_kl:.3g}, largest |lv| {hi_lv:.3g}")


def test_gpu_case_tables_cover_what_they_claim():
    fused = [c for c in gpu_cases.FUSED_CASES if c[6] != 0]
    t16, t32 = [c for c in fused if c[6] == 16], [c for c in fused if c[6] == 32]
    assert {c[1] for c in t16} == set(range(1, 9)) and {c[1] for c in t32} == {1, 3, 5, 8}
    assert {c[2] for c in t16} == {1, 5, 16, 17, 77, 2048} and {c[2] for c in t32} == {2049, 4100, 16384}
    for c in fused:   # the tile rows snet_ae_pick_tr gives: 16 rows up to 128 tiles
        assert c[6] == (16 if -(-c[2] // 16) <= 128 else 32)
    for d in range(1, 9):
        mine = [c for c in t16 if c[1] == d]
        assert any(c[2] < 16 for c in mine) and any(c[2] % 16 != 0 and c[2] > 16 for c in mine) and any(c[2] % 16 == 0 for c in mine), d
        assert {c[3] for c in fused if c[1] == d} == {"idx", "row0"}, d
    for batch in {c[2] for c in fused}:
        assert {c[1] % 2 for c in fused if c[2] == batch} == {0, 1}, batch
    assert {c[4] for c in fused} == {0.0, 0.3, 4.0}
    assert 3 * sum(c[5] for c in fused) >= len(fused) - 2 and 28 <= len(gpu_cases.FUSED_CASES) <= 34
    assert [c for c in gpu_cases.FUSED_CASES if c[6] == 0] == [("C", 2, 16385, "idx", 0.3, False, 0)]
    layer = gpu_cases.LAYER_CASES
    for keys in ("ABC", "W"):
        mine = [c for c in layer if c[0] in keys]
        assert {c[1] for c in mine} == set(range(1, 9)), keys
        assert {c[2] for c in mine} >= {1, 255, 256, 257, 1000}, keys
        assert {c[3] for c in mine if c[2] == 1000} == {"idx", "row0"}, keys
    ev = gpu_cases.EVAL_CASES
    for batch, path in ((77, 1), (2100, 1), (None, 0)):
        mine = [c for c in ev if c[4] == path and (batch is None or c[2] == batch)]
        assert {c[1] for c in mine} == {1, 3, 4, 7} and {c[3] for c in mine} == {"idx", "row0"}, (batch, path)
    assert {(c[1], c[3]) for c in gpu_cases.LARGE_LV_CASES} == {(1, 8.0), (1, -8.0), (0, 8.0), (0, -8.0)}
