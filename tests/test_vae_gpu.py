"""The variational autoencoder on the MI355X: forward parity with the reference's vae_model.zip (tests/golden/vae_model.npz),
the ELBO training step against a float64 torch restatement of mlcolvar's VariationalAutoEncoderCV step (written out below,
fed the same initial parameters and the same eps), the epoch entry points and the noise cursor, the calculator on the
reference's test configuration, and the refusal of a frame-sharded fit."""
import io
import json
import os
import zipfile

import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests.test_calculators_gpu import TEST_COMMON, match_fraction
from tests.test_mlp_gpu import ar_features, normalized

pytestmark = pytest.mark.gpu

_ACT = {"leaky_relu": torch.nn.functional.leaky_relu, "tanh": torch.tanh, "elu": torch.nn.functional.elu, None: lambda x: x}


def _init(dims, latent, seed):
    """torch.nn.Linear initialisation in VariationalAutoEncoderCV's order (encoder, mean_nn, log_var_nn, decoder); the heads
    concatenated as the engine holds them."""
    torch.manual_seed(seed)
    d = dims[latent] // 2
    lins = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(latent - 1)]
    mean, lv = torch.nn.Linear(dims[latent - 1], d), torch.nn.Linear(dims[latent - 1], d)
    dec = [torch.nn.Linear(d if i == latent else dims[i], dims[i + 1]) for i in range(latent, len(dims) - 1)]
    out = [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in lins]
    out.append((torch.cat([mean.weight, lv.weight]).detach().numpy().copy(), torch.cat([mean.bias, lv.bias]).detach().numpy().copy()))
    return out + [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in dec]


class VaeRef:
    """The training step of mlcolvar's VariationalAutoEncoderCV with elbo_gaussians_loss, in float64:
    h = encoder(xn); mu, lv = heads(h); z = eps * exp(lv / 2) + mu; x_hat = decoder(z) * range + mean;
    loss = mean((x_hat - x)^2) + beta * mean_batch(-0.5 * sum(lv - exp(lv) - mu^2 + 1))."""

    def __init__(self, linears, acts, latent, rng, lr):
        self.p = [(torch.tensor(w, dtype=torch.float64, requires_grad=True), torch.tensor(b, dtype=torch.float64, requires_grad=True))
                  for w, b in linears]
        self.acts, self.latent = acts, latent
        self.rng = torch.as_tensor(np.asarray(rng), dtype=torch.float64)
        self.opt = torch.optim.Adam([t for wb in self.p for t in wb], lr=lr)

    def loss(self, xn, eps, beta, masks=None):
        h = xn
        masks = masks or {}
        for l, (w, b) in enumerate(self.p):
            if l == self.latent:
                d = h.shape[1] // 2
                mu, lv = h[:, :d], h[:, d:]
                h = eps * torch.exp(lv / 2) + mu
            h = _ACT[self.acts[l]](h @ w.T + b)
            if l in masks:
                h = h * masks[l]
        rec = ((h - xn) * self.rng).square().mean()
        kl = (-0.5 * (lv - lv.exp() - mu ** 2 + 1).sum(dim=1)).mean()
        return rec + beta * kl, rec, kl

    def step(self, xn, eps, beta, masks=None):
        self.opt.zero_grad()
        loss, rec, kl = self.loss(xn, eps, beta, masks)
        loss.backward()
        self.opt.step()
        return float(loss), float(rec), float(kl)


def _engine(dims, acts, latent, max_batch, rng, lr=1e-3, **kw):
    from deep_cartograph_amd import hip

    eng = hip.Mlp("vae", dims, acts, max_batch=max_batch, latent_layer=latent, lr=lr, **kw)
    eng.set_feature_range(rng)
    return eng


REF_DIMS = [54, 16, 8, 4, 4, 8, 54]          # [54, 16, 8] -> heads 2 x 2 -> z (2) -> [4, 8, 54]: dims[3] = 2d, Linear 3 reads d
REF_ACTS = ["leaky_relu", "leaky_relu", None, "leaky_relu", "leaky_relu", None]


@pytest.mark.parametrize("dims,acts,latent,n,batch,beta,path", [
    (REF_DIMS, REF_ACTS, 3, 164, 128, 0.0, 1),        # the reference's test network and its clamped batch (+ a 36-row ragged batch)
    (REF_DIMS, REF_ACTS, 3, 164, 128, 1e-2, 1),
    (REF_DIMS, REF_ACTS, 3, 164, 128, 1.0, 1),
    ([128, 64, 32, 8, 32, 64, 128], ["tanh", "tanh", None, "leaky_relu", "tanh", None], 3, 1500, 512, 1e-2, 1),   # d = 4
    (REF_DIMS, REF_ACTS, 3, 9000, 4096, 1e-2, 1),     # 4096 rows: 128 workgroups of 32 rows (+ a ragged 808-row batch)
    (REF_DIMS, REF_ACTS, 3, 40000, 20000, 1e-2, 0),   # 625 tiles: too many for the fused step, the layer-by-layer path
    ([20, 6, 12, 3, 20], ["elu", None, "leaky_relu", None], 2, 250, 100, 0.5, 1),   # one hidden encoder layer, d = 6, ragged 50
])
def test_vae_steps_match_float64_restatement(dims, acts, latent, n, batch, beta, path):
    X = ar_features(n, dims[0], 23)
    Xn, m, r = normalized(X)
    lins = _init(dims, latent, 7)
    eng = _engine(dims, acts, latent, batch, r)
    eng.set_linears(lins)
    eng.set_kl_beta(beta)
    ref = VaeRef(lins, acts, latent, r, 1e-3)
    d = dims[latent] // 2
    Xd, Xt = torch.from_numpy(Xn).cuda(), torch.from_numpy(Xn).double()
    g = torch.Generator().manual_seed(11)
    steps, got_ref = [], []
    while len(steps) < 24:
        perm = torch.randperm(n, generator=g)
        steps += [perm[i:i + batch] for i in range(0, n, batch)]
    steps = steps[:24]
    eps = [torch.randn(len(b), d, generator=g) for b in steps]
    eng.set_noise(torch.cat(eps).cuda())
    eng.reset_log(len(steps))
    from tests.test_snet_dt_gpu import tile_rows

    for b, e in zip(steps, eps):
        eng.train_step(Xd, idx=b.cuda())
        assert eng.last_path() == path
        # snet_ae_kernel<16, true> up to 2048 rows, <32, true> beyond (the 4096-row case runs both)
        assert tile_rows(eng) == (0 if path == 0 else (16 if len(b) <= 2048 else 32))
        got_ref.append(ref.step(Xt[b], e.double(), beta))
    assert eng.noise_position() == sum(len(b) for b in steps)
    rec, exp = eng.read_log(), np.array(got_ref)
    assert rec.shape == (24, 4)
    np.testing.assert_allclose(rec[:, 1], [len(b) for b in steps])
    np.testing.assert_allclose(rec[:, 0], exp[:, 0], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(rec[:, 2], exp[:, 1], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(rec[:, 3], exp[:, 2], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(rec[:, 0], rec[:, 2] + beta * rec[:, 3], rtol=1e-12)
    worst = 0.0
    for (w, b), (wr, br) in zip(eng.get_linears(), ref.p):   # the fused autoencoder tests' tolerance (test_snet_dt_gpu.py)
        np.testing.assert_allclose(w, wr.detach().numpy(), atol=3e-6 * max(1.0, float(wr.abs().max())))
        np.testing.assert_allclose(b, br.detach().numpy(), atol=3e-6)
        worst = max(worst, np.max(np.abs(w - wr.detach().numpy())))
    print(f"{dims} batch {batch} beta {beta} path {path}: max |d weight| after 24 Adam steps = {worst:.2e}")
    eng.close()


def test_vae_first_step_gradients_and_latent_sample():
    X = ar_features(300, 54, 5)
    Xn, m, r = normalized(X)
    lins = _init(REF_DIMS, 3, 3)
    eng = _engine(REF_DIMS, REF_ACTS, 3, 256, r)
    eng.set_linears(lins)
    eng.set_kl_beta(0.3)
    ref = VaeRef(lins, REF_ACTS, 3, r, 1e-3)
    eps = torch.randn(256, 2, generator=torch.Generator().manual_seed(2))
    eng.set_noise(eps.cuda())
    eng.reset_log(4)
    Xd = torch.from_numpy(Xn).cuda()
    eng.forward(Xd, row0=10, batch=256)
    eng.backward(Xd, row0=10, batch=256)
    loss, rec, kl = ref.loss(torch.from_numpy(Xn[10:266]).double(), eps.double(), 0.3)
    loss.backward()
    with torch.no_grad():
        h = torch.from_numpy(Xn[10:266]).double()
        for l in range(3):
            h = _ACT[REF_ACTS[l]](h @ ref.p[l][0].T + ref.p[l][1])
        z = eps.double() * torch.exp(h[:, 2:] / 2) + h[:, :2]
    np.testing.assert_allclose(eng.latent_sample(256).cpu().numpy(), z.numpy(), rtol=1e-5, atol=1e-6)
    g = eng.grads_view().cpu().numpy()
    for l, (w, b) in enumerate(ref.p):
        wo, bo = eng.offsets[l]
        gw, gb = w.grad.numpy(), b.grad.numpy()
        assert np.max(np.abs(g[wo:wo + gw.size].reshape(gw.shape) - gw)) < 1e-4 * max(1.0, np.abs(gw).max()), f"weight {l}"
        assert np.max(np.abs(g[bo:bo + gb.size] - gb)) < 1e-4 * max(1.0, np.abs(gb).max()), f"bias {l}"
    np.testing.assert_allclose(eng.read_log()[0], [float(loss), 256, float(rec), float(kl)], rtol=1e-5)
    eng.close()


def test_vae_dropout_and_batchnorm_on_the_layer_path():
    """Dropout behind the encoder's hidden layers (the engine's masks handed to the restatement through the test hook), and a
    batch normalisation behind a decoder layer checked against torch.nn.BatchNorm1d in training mode."""
    X = ar_features(400, 54, 9)
    Xn, m, r = normalized(X)
    lins = _init(REF_DIMS, 3, 4)
    drops = [0.2, 0.1, 0.0, 0.0, 0.0, 0.0]
    eng = _engine(REF_DIMS, REF_ACTS, 3, 128, r, dropout=drops, seed=99)
    eng.set_linears(lins)
    eng.set_kl_beta(1e-2)
    ref = VaeRef(lins, REF_ACTS, 3, r, 1e-3)
    Xd, Xt = torch.from_numpy(Xn).cuda(), torch.from_numpy(Xn).double()
    g = torch.Generator().manual_seed(1)
    eps = torch.randn(20 * 128, 2, generator=g)
    eng.set_noise(eps.cuda())
    eng.reset_log(20)
    exp = []
    for s in range(20):
        b = torch.randperm(400, generator=g)[:128]
        step = eng.dropout_step()
        eng.train_step(Xd, idx=b.cuda())
        assert eng.last_path() == 0
        masks = {l: eng.dropout_mask(l, step, 128).cpu().double() for l in (0, 1)}
        exp.append(ref.step(Xt[b], eps[s * 128:(s + 1) * 128].double(), 1e-2, masks))
    rec = eng.read_log()
    np.testing.assert_allclose(rec[:, 0], np.array(exp)[:, 0], rtol=1e-4)
    for (w, b), (wr, br) in zip(eng.get_linears(), ref.p):
        np.testing.assert_allclose(w, wr.detach().numpy(), atol=1e-4)
    eng.close()
    # batch normalisation behind decoder Linear 4 (one training step: the gradient of every parameter)
    bn = [False, False, False, False, True, False]
    eng = _engine(REF_DIMS, REF_ACTS, 3, 128, r, batchnorm=bn)
    eng.set_linears(lins)
    eng.set_kl_beta(0.5)
    e = torch.randn(128, 2, generator=g)
    eng.set_noise(e.cuda())
    eng.reset_log(2)
    eng.forward(Xd, row0=0, batch=128)
    eng.backward(Xd, row0=0, batch=128)
    p = [(torch.tensor(w, dtype=torch.float64, requires_grad=True), torch.tensor(b_, dtype=torch.float64, requires_grad=True)) for w, b_ in lins]
    norm = torch.nn.BatchNorm1d(8).double().train()
    h = Xt[:128]
    for l, (w, b_) in enumerate(p):
        if l == 3:
            mu, lv = h[:, :2], h[:, 2:]
            h = e.double() * torch.exp(lv / 2) + mu
        h = _ACT[REF_ACTS[l]](h @ w.T + b_)
        if bn[l]:
            h = norm(h)
    loss = ((h - Xt[:128]) * torch.as_tensor(r, dtype=torch.float64)).square().mean() + 0.5 * (-0.5 * (lv - lv.exp() - mu ** 2 + 1).sum(1)).mean()
    loss.backward()
    assert abs(eng.read_log()[0, 0] - float(loss)) < 1e-5 * max(1.0, abs(float(loss)))
    gr = eng.grads_view().cpu().numpy()
    for l, (w, b_) in enumerate(p):
        wo, _ = eng.offsets[l]
        assert np.max(np.abs(gr[wo:wo + w.numel()].reshape(w.shape) - w.grad.numpy())) < 1e-4 * max(1.0, float(w.grad.abs().max())), l
    go, beo = eng.bn_offsets[4]
    np.testing.assert_allclose(gr[go:go + 8], norm.weight.grad.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(gr[beo:beo + 8], norm.bias.grad.numpy(), rtol=1e-4, atol=1e-6)
    eng.close()


@pytest.mark.parametrize("path", [1, 0])
def test_vae_epoch_entry_points_bit_for_bit_and_noise_cursor(path):
    """train_steps / eval_steps against the step-by-step loop, records and parameters bit for bit, noise cursor included:
    path 1 = the fused step (the validation pass as ONE launch of five batches, each taking its own eps rows), path 0 = the
    layer-by-layer engine (a batch normalisation keeps the fused form off)."""
    from deep_cartograph_amd import hip

    X = ar_features(1000, 54, 13)
    Xn, m, r = normalized(X)
    lins = _init(REF_DIMS, 3, 8)
    Xd = torch.from_numpy(Xn).cuda()
    idx = torch.randperm(1000, generator=torch.Generator().manual_seed(3)).cuda()
    eps = torch.randn(7 * 128 + 5 * 128, 2, generator=torch.Generator().manual_seed(4)).cuda()
    bn = None if path == 1 else [False, False, False, False, True, False]
    out = []
    for one_call in (False, True):
        eng = _engine(REF_DIMS, REF_ACTS, 3, 128, r, batchnorm=bn)
        eng.set_linears(lins)
        eng.set_kl_beta(0.05)
        eng.set_noise(eps)
        eng.reset_log(12)
        if one_call:
            eng.train_steps(Xd, 128, 7, idx=idx)
            assert eng.noise_position() == 7 * 128 and eng.last_path() == path
            eng.eval_steps(Xd, 128, 5, row0=100)
        else:
            for j in range(7):
                eng.train_step(Xd, idx=idx[j * 128:(j + 1) * 128])
            for j in range(5):
                eng.eval_step(Xd, row0=100 + j * 128, batch=128)
        assert eng.last_path() == path
        assert eng.noise_position() == 12 * 128
        out.append((eng.read_log(), eng.get_linears()))
        with pytest.raises(hip.DcvError, match="noise"):   # the buffer is used up: refused before any launch
            eng.eval_step(Xd, row0=0, batch=1)
        assert eng.noise_position() == 12 * 128 and len(eng.read_log()) == 12
        eng.close()
    (ra, la), (rb, lb) = out
    np.testing.assert_array_equal(ra, rb)
    for (wa, ba), (wb, bb) in zip(la, lb):
        np.testing.assert_array_equal(wa, wb)
        np.testing.assert_array_equal(ba, bb)
    # a validation pass the noise buffer covers only in part: the covered batches go, the first uncovered one is refused
    eng = _engine(REF_DIMS, REF_ACTS, 3, 128, r, batchnorm=bn)
    eng.set_linears(lins)
    eng.set_noise(eps[:3 * 128])
    eng.reset_log(8)
    with pytest.raises(hip.DcvError, match="noise"):
        eng.eval_steps(Xd, 128, 5, row0=0)
    assert eng.noise_position() == 3 * 128 and len(eng.read_log()) == 3
    eng.close()
    eng = _engine(REF_DIMS, REF_ACTS, 3, 128, r)
    eng.reset_log(1)
    with pytest.raises(hip.DcvError, match="noise"):   # no noise set at all
        eng.train_step(Xd, row0=0, batch=16)
    eng.close()


def _fixture_engine():
    g = load_golden("vae_model.npz")
    p = lambda n: g[f"param.{n}"]
    heads = (np.concatenate([p("mean_nn.weight"), p("log_var_nn.weight")]), np.concatenate([p("mean_nn.bias"), p("log_var_nn.bias")]))
    lins = [(p("encoder.nn.0.weight"), p("encoder.nn.0.bias")), (p("encoder.nn.3.weight"), p("encoder.nn.3.bias")), heads] + \
           [(p(f"decoder.nn.{i}.weight"), p(f"decoder.nn.{i}.bias")) for i in (0, 3, 6)]
    return g, lins


def test_vae_forward_matches_reference_model(features, tmp_path):
    from deep_cartograph_amd import export, hip
    from deep_cartograph_amd.cv_calculator import CVCalculator, VAECalculator

    X, names = features
    g, lins = _fixture_engine()
    eng = _engine(REF_DIMS, REF_ACTS, 3, 256, g["buffer.norm_in.range"])
    eng.set_linears(lins)
    Xn = hip.normalize(torch.from_numpy(X).cuda(), torch.from_numpy(g["buffer.norm_in.mean"]).cuda(), torch.from_numpy(g["buffer.norm_in.range"]).cuda())
    out, _ = eng.infer(Xn, pmean=torch.from_numpy(g["buffer.postprocessing.mean"]).cuda(), prange=torch.from_numpy(g["buffer.postprocessing.range"]).cuda())
    np.testing.assert_allclose(out.cpu().numpy(), g["output"], atol=2e-5)
    eng.close()
    # model.zip in the reference's format, written by our exporter, loads through CVCalculator.load
    from tests.test_vae_cpu import _vae_module_from_fixture

    _, model = _vae_module_from_fixture()
    pt = tmp_path / "cv_weights.pt"
    export.save_torchscript(model, 54, str(pt))
    zpath = tmp_path / "vae_model.zip"
    with zipfile.ZipFile(zpath, "w") as z:
        z.writestr("model/metadata.json", json.dumps({"cv_name": "vae", "cv_dimension": 2}))
        z.writestr("model/features_labels.txt", "\n".join(names) + "\n")
        z.write(pt, "model/cv_weights.pt")
    calc = CVCalculator.load(str(zpath), str(tmp_path / "load"))
    assert isinstance(calc, VAECalculator)
    np.testing.assert_allclose(calc.project_data(torch.from_numpy(X.copy())).numpy(), g["output"], atol=2e-5)


def _restated_fit(X, m, r, training, dims, acts, latent):
    """The calculator's fit restated in float32 torch on the host: seed, model construction order, split, per-epoch beta, the
    loaders' permutations (shuffle) and one randn(batch, d) per batch in loader order (training loader, then validation
    loader; lightning's sanity validation runs inside isolate_rng and draws nothing), Adam, early stopping."""
    from deep_cartograph_amd.cv_calculator import kl_annealing_settings, kl_beta

    gcfg, es = training["general"], training["early_stopping"]
    max_epochs, seed, shuffle = gcfg["max_epochs"], gcfg["seed"] + 1, gcfg["shuffle"]
    kl = kl_annealing_settings(training.get("kl_annealing"), max_epochs)
    gen = torch.manual_seed(seed)
    lins = _init_no_seed(dims, latent)
    n = X.shape[0]
    sizes = [int(np.floor(n * f)) for f in gcfg["lengths"]]
    for i in range(n - sum(sizes)):
        sizes[i % 2] += 1
    perm = torch.randperm(n, generator=gen)
    tr, va = perm[:sizes[0]], perm[sizes[0]:]
    bs = 128   # closest power of two below the training samples (reference :1297-1309)
    d = dims[latent] // 2
    p = [(torch.tensor(w, requires_grad=True), torch.tensor(b, requires_grad=True)) for w, b in lins]
    opt = torch.optim.Adam([t for wb in p for t in wb], lr=1e-3)
    xn = torch.from_numpy(((X - m) / r).astype(np.float32))
    rng = torch.from_numpy(r.astype(np.float32))

    def loss_of(x, e, beta):
        h = x
        for l, (w, b) in enumerate(p):
            if l == latent:
                mu, lv = h[:, :d], h[:, d:]
                h = e * torch.exp(0.5 * lv) + mu
            h = _ACT[acts[l]](h @ w.T + b)
        rec = ((h - x) * rng).square().mean()
        kld = (-0.5 * (lv - lv.exp() - mu ** 2 + 1).sum(dim=1)).mean()
        return rec + beta * kld, rec, kld

    def wmean(vals):
        w = np.array([v[-1] for v in vals], dtype=np.float64)
        return [float(np.dot([v[i] for v in vals], w) / w.sum()) for i in range(len(vals[0]) - 1)]

    keys = ("valid_loss", "valid_reconstruction_loss", "valid_kl_loss", "train_loss", "train_reconstruction_loss", "train_kl_loss", "beta")
    met = {k: [] for k in keys}
    best, wait = float("inf"), 0
    for epoch in range(max_epochs):
        beta = kl_beta(epoch, kl)
        tri = tr[torch.randperm(len(tr))] if shuffle else tr
        tv = []
        for i in range(0, len(tri), bs):
            b = tri[i:i + bs]
            e = torch.randn(len(b), d)
            opt.zero_grad()
            loss, rec, kld = loss_of(xn[b], e, beta)
            loss.backward()
            opt.step()
            tv.append((float(loss), float(rec), float(kld), len(b)))
        vai = va[torch.randperm(len(va))] if shuffle else va
        vl = []
        with torch.no_grad():
            for i in range(0, len(vai), bs):
                b = vai[i:i + bs]
                loss, rec, kld = loss_of(xn[b], torch.randn(len(b), d), beta)
                vl.append((float(loss), float(rec), float(kld), len(b)))
        for k, v in zip(keys, wmean(vl) + wmean(tv) + [beta]):
            met[k].append(v)
        valid = met["valid_loss"][-1]
        if valid < best - es["min_delta"]:
            best, wait = valid, 0
        else:
            wait += 1
            if wait >= es["patience"]:
                break
    return met


def _init_no_seed(dims, latent):
    d = dims[latent] // 2
    lins = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(latent - 1)]
    mean, lv = torch.nn.Linear(dims[latent - 1], d), torch.nn.Linear(dims[latent - 1], d)
    dec = [torch.nn.Linear(d if i == latent else dims[i], dims[i + 1]) for i in range(latent, len(dims) - 1)]
    out = [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in lins]
    out.append((torch.cat([mean.weight, lv.weight]).detach().numpy().copy(), torch.cat([mean.bias, lv.bias]).detach().numpy().copy()))
    return out + [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in dec]


REF_KL = {"type": "linear", "start_beta": 0, "max_beta": 0.001, "start_epoch": 1000, "n_epochs_anneal": 5000}


def _vae_calc(tmp_path, max_epochs, kl_section, **general):
    from deep_cartograph_amd.cv_calculator import VAECalculator

    cfg = json.loads(json.dumps(TEST_COMMON))
    cfg["training"]["general"]["max_epochs"] = max_epochs
    cfg["training"]["general"].update(general)
    if kl_section is not None:
        cfg["training"]["kl_annealing"] = dict(kl_section)
    return cfg, VAECalculator(cfg, str(tmp_path))


@pytest.mark.parametrize("kl_section,max_epochs,shuffle", [(REF_KL, 1000, False), (None, 60, False), (None, 60, True)])
def test_vae_calculator_against_restatement(features, golden_proj, tmp_path, kl_section, max_epochs, shuffle):
    X, names = features
    cfg, calc = _vae_calc(tmp_path, max_epochs, kl_section, shuffle=shuffle)
    calc.set_training_matrix(X.copy(), names)
    df = calc.run(2)
    assert df is not None and list(df.columns) == ["VAE 1", "VAE 2"]
    assert calc.engine.last_path() == 1   # the reference's sizes take the fused step
    m, r = calc.features_norm_mean.astype(np.float32), calc.features_norm_range.astype(np.float32)
    dims, acts = [54, 16, 8, 4, 4, 8, 54], ["leaky_relu", "leaky_relu", None, "leaky_relu", "leaky_relu", None]
    exp = _restated_fit(X, m, r, cfg["training"], dims, acts, 3)
    n_exp, n_got = len(exp["valid_loss"]), len(calc.metrics["valid_loss"])
    print(f"vae epochs ({'reference config' if kl_section else 'annealing defaults'}, shuffle {shuffle}): engine {n_got}, restatement {n_exp}")
    assert n_got == n_exp
    worst = {}
    for key in ("valid_loss", "train_loss", "valid_reconstruction_loss", "train_reconstruction_loss", "valid_kl_loss", "train_kl_loss"):
        worst[key] = float(np.max(np.abs(np.array(calc.metrics[key]) / np.array(exp[key]) - 1)))
    print("  worst relative deviation:", {k: f"{v:.1e}" for k, v in worst.items()})
    for key in worst:
        np.testing.assert_allclose(calc.metrics[key], exp[key], rtol=2e-4, err_msg=key)
    np.testing.assert_array_equal(calc.metrics["beta"], exp["beta"])
    frac = match_fraction(df.to_numpy(), golden_proj["vae"])
    print(f"vae vs the reference's projected_trajectory.csv: identical '%.4f' entries {frac:.3f} (not pinned: see the issue)")
    with zipfile.ZipFile(tmp_path / "vae" / "model.zip") as z:
        ts = torch.jit.load(io.BytesIO(z.read("model/cv_weights.pt")))
    assert [n for n, _ in ts.named_children()] == ["loss_fn", "norm_in", "encoder", "mean_nn", "log_var_nn", "decoder", "postprocessing"]
    with torch.no_grad():
        np.testing.assert_allclose(ts(torch.from_numpy(X)).numpy(), df.to_numpy(), atol=5e-5)
    with zipfile.ZipFile(tmp_path / "vae" / "training" / "training_metrics.zip") as z:
        got = {os.path.basename(n) for n in z.namelist()}
    assert {"train_loss.npy", "valid_loss.npy", "epoch.npy", "train_kl_loss.npy", "valid_kl_loss.npy", "train_reconstruction_loss.npy",
            "valid_reconstruction_loss.npy", "beta.npy"} <= got
    from tests.test_calculators_gpu import _check_sensitivity

    _check_sensitivity(tmp_path / "vae", ts, X, names)


def test_vae_best_is_the_best_post_annealing_checkpoint(features, tmp_path):
    """model_to_save 'best': the lowest valid_loss from the end of the annealing (start_epoch + n_epochs_anneal) on, that
    model exported; no epoch past the annealing -> the last checkpoint, scored with the final validation loss."""
    X, names = features
    kl = {"type": "linear", "start_beta": 0, "max_beta": 0.01, "start_epoch": 5, "n_epochs_anneal": 10}
    cfg, calc = _vae_calc(tmp_path / "a", 40, kl)
    calc.model_to_save = "best"
    calc.set_training_matrix(X.copy(), names)
    calc.run(2)
    vl = calc.metrics["valid_loss"]
    assert len(vl) > 16 and calc.cv_score == min(vl[15:])
    best_epoch = 15 + int(np.argmin(vl[15:]))
    cfg2, calc2 = _vae_calc(tmp_path / "b", best_epoch + 1, kl)   # the same fit stopped at the chosen epoch: its last state
    calc2.set_training_matrix(X.copy(), names)
    calc2.run(2)
    for (w, b), (w2, b2) in zip(calc.cv["linears"], calc2.cv["linears"]):
        np.testing.assert_array_equal(w, w2)
        np.testing.assert_array_equal(b, b2)
    kl_long = dict(kl, n_epochs_anneal=100)
    cfg3, calc3 = _vae_calc(tmp_path / "c", 30, kl_long)
    calc3.model_to_save = "best"
    calc3.set_training_matrix(X.copy(), names)
    calc3.run(2)
    assert calc3.cv_score == calc3.metrics["valid_loss"][-1]


def _dp_rank(rank, world, port, tmpdir):
    import torch.distributed as dist

    from deep_cartograph_amd import hip

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    Xn, _, r = normalized(ar_features(256, 54, 3))
    eng = _engine(REF_DIMS, REF_ACTS, 3, 64, r)
    eng.set_linears(_init(REF_DIMS, 3, 1))
    eng.set_noise(torch.zeros(64, 2).cuda())
    eng.reset_log(2)
    try:
        eng.data_parallel_step(torch.from_numpy(Xn).cuda(), dist, 64 * world, row0=rank * 64, batch=64)
        msg = "accepted"
    except hip.DcvError as e:
        msg = str(e)
    with open(os.path.join(tmpdir, f"rank{rank}.txt"), "w") as f:
        f.write(msg)
    eng.close()
    dist.destroy_process_group()


def test_frame_sharded_vae_is_refused(tmp_path):
    """dcv_mlp_dp_step refuses a VAE step whose global batch spans more than this rank (two gloo ranks on one GPU); the
    calculator refuses the fit before it starts."""
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_dp_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for rank in (0, 1):
        msg = (tmp_path / f"rank{rank}.txt").read_text()
        assert "variational autoencoder is not implemented for data-parallel" in msg, msg
