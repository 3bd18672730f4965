"""One ELBO step of the variational autoencoder in NumPy float64, the backward pass written out by hand (no torch, no
autograd: tests/test_vae_oracle_cpu.py pins it against float64 autograd of the same expression).

    h = act(h W^T + b) through the encoder;  [mu | lv] = heads(h);  z = eps * exp(lv / 2) + mu;  x_hat = decoder(z)
    recon = mean(((x_hat - xn) * range)^2);  kl = mean_rows(-0.5 * sum_j(lv - exp(lv) - mu^2 + 1));  loss = recon + beta * kl

Layers are in the engine's order: the encoder's Linears, the two heads concatenated as one Linear [mean | log-variance]
(index latent - 1, no activation), then the decoder, whose first Linear (index latent) reads z."""
import numpy as np

LEAKY_SLOPE = 0.01   # torch.nn.functional.leaky_relu's default, the engine's


def _act(name, a):
    """(act(a), act'(a)) for the pre-activation a."""
    if name is None or name == "none":
        return a, np.ones_like(a)
    if name == "tanh":
        h = np.tanh(a)
        return h, 1.0 - h * h
    if name == "elu":
        e = np.exp(np.minimum(a, 0.0))
        return np.where(a > 0, a, e - 1.0), np.where(a > 0, 1.0, e)
    if name == "leaky_relu":
        return np.where(a > 0, a, LEAKY_SLOPE * a), np.where(a > 0, 1.0, LEAKY_SLOPE)
    raise ValueError(f"vae_oracle: activation {name!r} is not restated here")


def forward(linears, acts, latent, xn, eps, rng, beta):
    """The forward pass on the rows xn with the noise rows eps.  Returns a dict: loss, recon, kl, the sums SSE and KL (the
    engine's stats_view() holds [SSE | KL sum]), z, mu, lv, x_hat, and the per-layer inputs / activation slopes the backward
    pass reads."""
    xn = np.asarray(xn, dtype=np.float64)
    eps = np.asarray(eps, dtype=np.float64)
    rng = np.asarray(rng, dtype=np.float64)
    B, F = xn.shape
    h, inputs, slopes = xn, [], []
    mu = lv = z = None
    for l, (w, b) in enumerate(linears):
        if l == latent:
            d = h.shape[1] // 2
            mu, lv = h[:, :d], h[:, d:]
            z = eps * np.exp(lv / 2) + mu
            h = z
        inputs.append(h)
        h, s = _act(acts[l], h @ np.asarray(w, dtype=np.float64).T + np.asarray(b, dtype=np.float64))
        slopes.append(s)
    sse = float(np.sum(((h - xn) * rng) ** 2))
    kl_sum = float(np.sum(-0.5 * (lv - np.exp(lv) - mu ** 2 + 1.0)))
    recon, kl = sse / (B * F), kl_sum / B
    return dict(loss=recon + beta * kl, recon=recon, kl=kl, SSE=sse, KL=kl_sum, z=z, mu=mu, lv=lv, x_hat=h, inputs=inputs,
                slopes=slopes)


def step(linears, acts, latent, xn, eps, rng, beta):
    """forward() plus the gradient of loss with respect to every weight and bias: `grads` = [(dW, db)] in layer order, and
    the gradient at the heads' output, dmu = dz + beta * mu / B and dlv = dz * eps * 0.5 * exp(lv / 2) + beta * 0.5 *
    (exp(lv) - 1) / B."""
    out = forward(linears, acts, latent, xn, eps, rng, beta)
    xn = np.asarray(xn, dtype=np.float64)
    eps = np.asarray(eps, dtype=np.float64)
    rng = np.asarray(rng, dtype=np.float64)
    B, F = xn.shape
    dh = 2.0 * (out["x_hat"] - xn) * rng * rng / (B * F)
    grads = [None] * len(linears)
    for l in range(len(linears) - 1, -1, -1):
        da = dh * out["slopes"][l]
        grads[l] = (da.T @ out["inputs"][l], da.sum(axis=0))
        dh = da @ np.asarray(linears[l][0], dtype=np.float64)
        if l == latent:
            mu, lv = out["mu"], out["lv"]
            out["dz"] = dh
            out["dmu"] = dh + beta * mu / B
            out["dlv"] = dh * eps * 0.5 * np.exp(lv / 2) + beta * 0.5 * (np.exp(lv) - 1.0) / B
            dh = np.concatenate([out["dmu"], out["dlv"]], axis=1)
    out["grads"] = grads
    return out


def _linear(g, fan_in, fan_out):
    """torch.nn.Linear's default draw restated: weight and bias uniform in (-1 / sqrt(fan_in), 1 / sqrt(fan_in))."""
    k = 1.0 / np.sqrt(fan_in)
    return g.uniform(-k, k, (fan_out, fan_in)).astype(np.float32), g.uniform(-k, k, fan_out).astype(np.float32)


def case(dims, acts, latent, n, seed, head_gain=4.0, lv_shift=0.0, noise_rows=None):
    """Inputs, float32 parameters and range of one test case: n rows of standardised features with three slow modes mixed in,
    `noise_rows` (default n) rows of standard-normal eps, the Linears in the engine's order (dims[latent] = 2d; the heads'
    weights times `head_gain`, the log-variance head's bias moved by `lv_shift`), range uniform in (0.5, 2).

    With torch.nn.Linear's initialisation |mu| and |lv| are about 0.1 and the KL term is a difference of nearly equal numbers;
    head_gain = 4 puts the KL per row between 1 and 10.  The builder asserts on the oracle's own output that the case is well
    conditioned: mean KL per row >= 0.05 and max |lv| <= 12."""
    g = np.random.Generator(np.random.PCG64(seed))
    F, d = dims[0], dims[latent] // 2
    assert dims[latent] == 2 * d and dims[-1] == F and len(acts) == len(dims) - 1
    slow = np.cumsum(g.standard_normal((n, 3)), axis=0) / np.sqrt(np.arange(1, n + 1))[:, None]
    X = slow @ g.standard_normal((3, F)) + 0.5 * g.standard_normal((n, F))
    Xn = ((X - X.mean(0)) / (X.std(0) + 1e-12) if n > 1 else X).astype(np.float32)
    rng = g.uniform(0.5, 2.0, F).astype(np.float32)
    eps = g.standard_normal((n if noise_rows is None else noise_rows, d)).astype(np.float32)
    lins = []
    for l in range(len(dims) - 1):
        if l == latent - 1:
            (wm, bm), (wl, bl) = _linear(g, dims[l], d), _linear(g, dims[l], d)
            lins.append((np.concatenate([wm, wl]) * np.float32(head_gain), np.concatenate([bm, bl + np.float32(lv_shift)])))
        else:
            lins.append(_linear(g, d if l == latent else dims[l], dims[l + 1]))
    m = min(n, eps.shape[0])
    chk = forward(lins, acts, latent, Xn[:m], eps[:m], rng, 1.0)
    assert chk["kl"] >= 0.05, f"ill-conditioned case: mean KL per row {chk['kl']:.3g} < 0.05"
    assert np.max(np.abs(chk["lv"])) <= 12.0, f"ill-conditioned case: max |lv| = {np.max(np.abs(chk['lv'])):.3g} > 12"
    return dict(dims=list(dims), acts=list(acts), latent=latent, d=d, Xn=Xn, eps=eps, lins=lins, range=rng)
