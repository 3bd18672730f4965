"""The variational autoencoder CV on the host: KL annealing schedule (reference modules/ml/ml.py KLAAnnealing), the
LROnPlateauManager start epoch, the registry lookup of train_colvars, and the TorchScript tree of the exporter.  No GPU."""
import logging

import numpy as np
import pytest
import torch

from tests.conftest import load_golden


def _anneal(type_, b0, b1, start, n, cycles, epoch):
    """ml.py's formulas, written out once more for the test."""
    if not epoch > start:
        return b0
    e = epoch - start

    def lin(x, m):
        return b1 if x >= m else b0 + (b1 - b0) * (x / m)

    if type_ == "linear":
        return lin(e, n)
    if type_ == "cyclical":
        if e >= n:
            return b1
        cl = n // cycles
        return lin(e % cl, cl // 2)
    mid = start + n // 2
    k = np.log(1e-3 / (1 - 1e-3)) / (start - mid)
    return b0 + (b1 - b0) / (1 + np.exp(-k * (e + start - mid)))


@pytest.mark.parametrize("type_,b0,b1,start,n,cycles", [
    ("linear", 0.0, 1e-3, 10, 40, 4),
    ("sigmoid", 1e-6, 1e-2, 20, 30, 1),
    ("cyclical", 0.0, 0.5, 5, 40, 4),
    ("cyclical", 1e-4, 2e-2, 0, 21, 3),
])
def test_kl_annealing_schedule(type_, b0, b1, start, n, cycles):
    from deep_cartograph_amd.cv_calculator import kl_annealing_settings, kl_beta

    kl = kl_annealing_settings({"type": type_, "start_beta": b0, "max_beta": b1, "start_epoch": start, "n_cycles": cycles,
                                "n_epochs_anneal": n}, 100)
    got = [kl_beta(e, kl) for e in range(start + n + 10)]
    exp = [_anneal(type_, b0, b1, start, n, cycles, e) for e in range(start + n + 10)]
    np.testing.assert_allclose(got, exp, rtol=1e-12, atol=0)
    assert got[start] == b0                      # strictly after start_epoch
    assert got[start + 1] != b0
    assert got[-1] == pytest.approx(b1, rel=2e-3)


def test_kl_annealing_defaults_and_fallbacks():
    from deep_cartograph_amd.cv_calculator import VAECalculator, kl_annealing_settings, kl_beta

    kl = kl_annealing_settings(None, 200)
    assert kl == {"type": "sigmoid", "start_beta": 1e-6, "max_beta": 0.01, "start_epoch": 100, "n_cycles": 1, "n_epochs_anneal": 50}
    assert kl_beta(100, kl) == 1e-6
    assert kl_beta(101, kl) == pytest.approx(_anneal("sigmoid", 1e-6, 0.01, 100, 50, 1, 101), rel=1e-12)
    # the sigmoid passes eps = 1e-3 of the way at start_epoch and its midpoint at start + n // 2
    assert kl_beta(125, kl) == pytest.approx(1e-6 + (0.01 - 1e-6) / 2, rel=1e-12)
    part = kl_annealing_settings({"type": "linear", "start_beta": 0, "max_beta": 1e-3}, 40)
    assert part["start_epoch"] == 20 and part["n_epochs_anneal"] == 10
    calc = VAECalculator({"dimension": 2, "training": {"general": {"max_epochs": 80}}})
    assert calc.kl["start_epoch"] == 40 and calc.kl["n_epochs_anneal"] == 20 and calc.kl["type"] == "sigmoid"
    with pytest.raises(ValueError):
        kl_beta(5, dict(kl, type="step", start_epoch=0))
    # KLAAnnealing.__init__'s checks, at construction rather than as a ZeroDivisionError in the middle of a fit
    with pytest.raises(ValueError, match="n_cycles"):
        kl_annealing_settings({"type": "cyclical", "start_beta": 0, "max_beta": 1e-3, "start_epoch": 1, "n_cycles": 4, "n_epochs_anneal": 3}, 40)
    with pytest.raises(ValueError, match="Invalid type"):
        VAECalculator({"dimension": 2, "training": {"kl_annealing": {"type": "step", "start_beta": 0, "max_beta": 1e-3}}})


def test_plateau_manager_start_epoch_and_extra_step():
    from deep_cartograph_amd.cv_calculator import _HostLRScheduler, kl_annealing_settings, plateau_manager_start

    kl = kl_annealing_settings({"type": "linear", "start_beta": 0, "max_beta": 1e-3, "start_epoch": 10, "n_epochs_anneal": 20}, 100)
    assert plateau_manager_start(kl, 100) == 10 + 20 + (100 - 30) // 4
    assert plateau_manager_start(kl_annealing_settings(None, 1000), 1000) == 500 + 250 + 250 // 4

    class _Eng:
        def __init__(self):
            self.lr = []

        def set_lr(self, v):
            self.lr.append(v)

        def set_momentum(self, v):
            pass

    eng = _Eng()
    s = _HostLRScheduler("ReduceLROnPlateau", {"patience": 0, "factor": 0.5}, {"interval": "epoch"}, "Adam", {"lr": 1e-3}, eng)
    s.plateau_from = 3
    for epoch in range(3):   # before the manager's epoch: nothing
        s.on_validation_end(epoch, 1.0)
    assert s.lr() == 1e-3
    s.on_validation_end(3, 1.0)   # first extra step: the best so far, no reduction
    s.on_validation_end(4, 1.0)   # no improvement, patience 0: halved
    assert s.lr() == pytest.approx(5e-4) and eng.lr[-1] == pytest.approx(5e-4)
    t = _HostLRScheduler("StepLR", {"step_size": 1}, {"interval": "epoch"}, "Adam", {"lr": 1e-3}, eng)
    t.plateau_from = 0
    t.on_validation_end(5, 1.0)   # only ReduceLROnPlateau is managed
    assert t.lr() == 1e-3


def test_train_colvars_keeps_vae_skips_umap(monkeypatch, tmp_path, caplog):
    from deep_cartograph_amd import tools
    from deep_cartograph_amd.cv_calculator import VAECalculator, calculator_class, cv_calculators_map

    assert calculator_class("vae") is VAECalculator and calculator_class("umap") is None
    assert calculator_class("ae") is cv_calculators_map["ae"]
    built = []

    class _Stop(Exception):
        pass

    def fake_load(self, *a, **k):
        built.append(self.cv_name)
        raise _Stop()

    monkeypatch.setattr(VAECalculator, "load_training_data", fake_load)
    caplog.set_level(logging.WARNING)
    with pytest.raises(_Stop):
        tools.train_colvars({"cvs": ["umap", "vae"]}, [str(tmp_path / "x.dat")], output_folder=str(tmp_path / "out"))
    assert built == ["vae"]
    skipped = [r.getMessage() for r in caplog.records if "skipped" in r.getMessage()]
    assert any("'umap'" in m for m in skipped) and not any("'vae'" in m for m in skipped)


def _vae_module_from_fixture():
    from deep_cartograph_amd import export

    g = load_golden("vae_model.npz")
    p = lambda n: g[f"param.{n}"]
    enc = export.FeedForward([(p("encoder.nn.0.weight"), p("encoder.nn.0.bias")), (p("encoder.nn.3.weight"), p("encoder.nn.3.bias"))],
                             ["leaky_relu", "leaky_relu"], [0.0, 0.0])
    dec = export.FeedForward([(p(f"decoder.nn.{i}.weight"), p(f"decoder.nn.{i}.bias")) for i in (0, 3, 6)], ["leaky_relu", "leaky_relu", None],
                             [0.0, 0.0, None])
    model = export.VariationalAutoEncoderCV(export.Normalization(g["buffer.norm_in.mean"], g["buffer.norm_in.range"]), enc,
                                            (p("mean_nn.weight"), p("mean_nn.bias")), (p("log_var_nn.weight"), p("log_var_nn.bias")), dec,
                                            export.Normalization(g["buffer.postprocessing.mean"], g["buffer.postprocessing.range"]))
    return g, model


def test_vae_torchscript_tree_and_reader(tmp_path):
    from deep_cartograph_amd import export

    g, model = _vae_module_from_fixture()
    path = str(tmp_path / "cv_weights.pt")
    export.save_torchscript(model, 54, path)
    ts = torch.jit.load(path)
    names = [n for n, _ in ts.named_modules()]
    assert [n for n in names if n and "." not in n] == ["loss_fn", "norm_in", "encoder", "mean_nn", "log_var_nn", "decoder", "postprocessing"]
    assert [n for n, _ in ts.named_parameters()] == [k[len("param."):] for k in g.files if k.startswith("param.")]
    assert sorted(n for n, _ in ts.named_buffers()) == sorted(k[len("buffer."):] for k in g.files if k.startswith("buffer."))
    X = load_golden("features_164x54.npz")["X"]
    with torch.no_grad():
        np.testing.assert_allclose(ts(torch.from_numpy(X)).numpy(), g["output"], atol=1e-6)
    parts = export.read_torchscript(path)
    assert parts["kind"] == "vae" and len(parts["linears"]) == 3 and parts["acts"] == ["leaky_relu", "leaky_relu", None]
    np.testing.assert_array_equal(parts["linears"][2][0], g["param.mean_nn.weight"])
    np.testing.assert_array_equal(parts["postprocessing"][1], g["buffer.postprocessing.range"])
