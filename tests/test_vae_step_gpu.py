"""The variational autoencoder's per-step arithmetic against tests/vae_oracle.py (NumPy float64, hand-written backward): ONE
training step or ONE validation pass per case, at latent widths 1 to 8, on the fused kernel (snet_ae_kernel<16 | 32, true>,
csrc/snet.hip) and on the layer-by-layer path (vae_sample_kernel, vae_sample_backward_kernel, latent_backward_layer,
csrc/mlp.hip).

Bounds (tests/test_snet_dt_gpu.py's): every gradient tensor within 2e-5 of the oracle tensor's largest entry; the loss,
reconstruction and KL records within 1e-5 relative; the record's weight equal to the batch; loss == recon + beta * kl to
1e-12; z (latent_sample) at rtol 1e-5 / atol 1e-6.

The case tables are plain data and the prepare_* functions need no GPU: tests/test_vae_oracle_cpu.py imports them and checks
that every case is well conditioned and that the tables cover what they claim to."""
import numpy as np
import pytest
import torch

from tests import vae_oracle as vo
from tests.test_mlp_gpu import rel_err
from tests.test_snet_dt_gpu import tile_rows

pytestmark = pytest.mark.gpu

GRAD_TOL, REC_TOL = 2e-5, 1e-5
Z_ATOL = 1e-6
# z behind the 300-wide heads of network W: mu and lv are 300-term float32 sums of size ~3, and at 1000 rows x 4 columns one
# z = eps * exp(lv / 2) + mu lands close enough to 0 for rtol to give nothing.  The same step in float32 torch on the host
# leaves |dz| - 1e-5 |z| = 1.23e-6 (W, 1000 rows, d = 4; 1.21e-6 at d = 7; the layer cases of A / B / C stay below 6e-7), so
# a correct kernel cannot hold atol = 1e-6 on W: 4 x 1.23e-6, for the summation order.  Measured on the MI355X: 1.33e-6.
Z_ATOL_W = 4.9e-6
CURSOR_ROWS = 7   # rows of the evaluation step that moves the noise cursor ahead of the training step


def net(key, d):
    """(dims, acts, latent) of the networks of this module at latent width d."""
    if key == "A":   # symmetric, two activations
        return [20, 12, 2 * d, 12, 20], ["tanh", None, "tanh", None], 2
    if key == "B":   # F % 4 != 0: the scalar input loader; an asymmetric decoder
        return [33, 12, 2 * d, 7, 33], ["elu", None, "leaky_relu", None], 2
    if key == "C":   # the reference's depth; tanh on every Linear that takes an activation (the heads take none)
        return [54, 16, 8, 2 * d, 4, 8, 54], ["tanh", "tanh", None, "tanh", "tanh", "tanh"], 3
    if key == "W":   # too wide for LDS: the layer-by-layer path whatever the batch
        return [64, 300, 2 * d, 300, 64], ["tanh", None, "tanh", None], 2
    raise KeyError(key)


# ---- a. fused training step: (network, d, batch, rows form, beta, noise cursor moved first, tile rows)
FUSED_CASES = [
    ("A", 1, 1, "row0", 0.3, True, 16),
    ("B", 1, 17, "idx", 4.0, False, 16),
    ("C", 1, 2048, "idx", 0.0, False, 16),
    ("B", 2, 5, "idx", 0.3, True, 16),
    ("A", 2, 77, "row0", 0.0, False, 16),
    ("C", 2, 16, "idx", 4.0, False, 16),
    ("C", 3, 5, "row0", 4.0, True, 16),
    ("A", 3, 77, "idx", 0.3, False, 16),
    ("B", 3, 2048, "row0", 0.3, False, 16),
    ("A", 4, 1, "idx", 4.0, False, 16),
    ("C", 4, 17, "row0", 0.3, True, 16),
    ("B", 4, 2048, "idx", 0.0, False, 16),
    ("B", 5, 1, "row0", 0.0, False, 16),
    ("C", 5, 77, "idx", 4.0, True, 16),
    ("A", 5, 16, "row0", 0.3, False, 16),
    ("C", 6, 5, "idx", 0.3, False, 16),
    ("B", 6, 17, "row0", 0.0, False, 16),
    ("A", 6, 16, "idx", 4.0, True, 16),
    ("A", 7, 5, "row0", 4.0, False, 16),
    ("B", 7, 77, "idx", 0.3, False, 16),
    ("C", 7, 16, "row0", 0.0, True, 16),
    ("B", 8, 5, "idx", 0.3, True, 16),
    ("A", 8, 17, "row0", 4.0, False, 16),
    ("C", 8, 2048, "row0", 0.0, False, 16),    # 128 tiles: the last batch on 16 rows; no padding column in the head tile
    ("A", 1, 2049, "idx", 0.3, True, 32),      # 65 tiles of 32 rows, a last tile of one row
    ("C", 8, 2049, "row0", 4.0, False, 32),
    ("B", 3, 4100, "row0", 0.0, False, 32),
    ("A", 8, 4100, "idx", 0.3, True, 32),
    ("C", 5, 16384, "idx", 0.3, False, 32),    # 512 tiles: the largest fused batch
    ("B", 8, 16384, "row0", 4.0, False, 32),
    ("C", 2, 16385, "idx", 0.3, False, 0),     # 513 tiles: off the fused path, the same oracle
]

# ---- b. layer-by-layer training step: (network, d, batch, rows form, beta); A / B / C through forward + backward, W through
#      train_step.  1, 255, 256, 257: the block edges of the 256-row sampling kernels
LAYER_CASES = [
    ("A", 1, 1, "row0", 0.3),
    ("B", 2, 255, "idx", 4.0),
    ("C", 3, 256, "row0", 0.0),
    ("A", 4, 257, "idx", 0.3),
    ("B", 5, 1000, "idx", 0.3),
    ("C", 6, 1000, "row0", 4.0),
    ("A", 7, 255, "row0", 0.0),
    ("B", 8, 257, "idx", 0.3),
    ("C", 1, 257, "idx", 4.0),
    ("A", 8, 256, "row0", 4.0),
    ("B", 3, 1, "idx", 0.3),
    ("C", 5, 255, "row0", 0.3),
    ("W", 1, 1000, "idx", 0.3),
    ("W", 2, 256, "row0", 4.0),
    ("W", 3, 257, "row0", 0.3),
    ("W", 4, 1000, "row0", 0.0),
    ("W", 5, 1, "idx", 0.3),
    ("W", 6, 255, "idx", 0.3),
    ("W", 7, 1000, "idx", 4.0),
    ("W", 8, 255, "row0", 0.3),
]

# ---- c. large log-variances: (network, path, batch, shift of the log-variance head's bias); d = 3, beta = 1
LARGE_LV_CASES = [("A", 1, 77, 8.0), ("A", 1, 77, -8.0), ("A", 0, 257, 8.0), ("A", 0, 257, -8.0)]

# ---- d. evaluation records: (network, d, batch, rows form, path, tile rows): one eval_step, then eval_steps with 5 batches
EVAL_BATCHES = 5
EVAL_CASES = [
    ("A", 1, 77, "idx", 1, 16),
    ("B", 3, 77, "row0", 1, 16),
    ("C", 4, 77, "idx", 1, 16),
    ("A", 7, 77, "row0", 1, 16),
    ("C", 1, 2100, "row0", 1, 32),
    ("A", 3, 2100, "idx", 1, 32),
    ("B", 4, 2100, "row0", 1, 32),
    ("C", 7, 2100, "idx", 1, 32),
    ("W", 1, 200, "row0", 0, 0),
    ("W", 3, 77, "idx", 0, 0),
    ("W", 4, 257, "idx", 0, 0),
    ("W", 7, 200, "row0", 0, 0),
]


def _seed(*parts):
    return sum((i + 1) * 7919 * int(p * 10 if isinstance(p, float) else p) for i, p in enumerate(parts)) % (2 ** 31)


def _rows(form, n, count, g, row0):
    """The logical rows of `count` samples: a random permutation (gathered) or the contiguous rows from row0 != 0."""
    return g.permutation(n)[:count].astype(np.int64) if form == "idx" else np.arange(row0, row0 + count, dtype=np.int64)


def prepare_step(key, d, batch, form, beta, cursor=False, lv_shift=0.0):
    """Inputs of one training step and the oracle's result on its rows (no GPU).  The step's eps rows are [e0, e0 + batch) of
    the noise buffer, e0 = CURSOR_ROWS when an evaluation step goes first."""
    dims, acts, latent = net(key, d)
    row0, e0 = 3, CURSOR_ROWS if cursor else 0
    n = max(batch, CURSOR_ROWS) + 13
    c = vo.case(dims, acts, latent, n, _seed(ord(key), d, batch, beta), lv_shift=lv_shift)
    rows = _rows(form, n, batch, np.random.Generator(np.random.PCG64(d * 1000 + batch)), row0)
    c.update(rows=rows, form=form, row0=row0, batch=batch, beta=beta, e0=e0,
             o=vo.step(c["lins"], acts, latent, c["Xn"][rows], c["eps"][e0:e0 + batch], c["range"], beta))
    return c


def prepare_eval(key, d, batch, form):
    """Inputs of 1 + EVAL_BATCHES evaluation batches and the oracle's forward pass of each, batch j on its own rows and on
    the eps rows [j * batch, (j + 1) * batch)."""
    dims, acts, latent = net(key, d)
    nb, row0, beta = 1 + EVAL_BATCHES, 5, 0.3
    n = nb * batch + 11
    c = vo.case(dims, acts, latent, n, _seed(ord(key), d, batch, 99))
    rows = _rows(form, n, nb * batch, np.random.Generator(np.random.PCG64(d * 1000 + batch + 1)), row0)
    c.update(rows=rows, form=form, row0=row0, batch=batch, beta=beta, nb=nb,
             o=[vo.forward(c["lins"], acts, latent, c["Xn"][rows[j * batch:(j + 1) * batch]], c["eps"][j * batch:(j + 1) * batch],
                           c["range"], beta) for j in range(nb)])
    return c


def _engine(c, max_batch):
    from deep_cartograph_amd import hip

    eng = hip.Mlp("vae", c["dims"], c["acts"], max_batch=max_batch, latent_layer=c["latent"], lr=1e-3)
    eng.set_feature_range(c["range"])
    eng.set_linears(c["lins"])
    eng.set_kl_beta(c["beta"])
    eng.set_noise(torch.from_numpy(c["eps"]).cuda())
    eng.reset_log(8)
    return eng


def _kw(c, lo=0, count=None):
    """The engine's row arguments for samples [lo, lo + count) of the case's rows."""
    count = c["batch"] if count is None else count
    if c["form"] == "idx":
        return dict(idx=torch.from_numpy(c["rows"][lo:lo + count]).cuda())
    return dict(row0=c["row0"] + lo, batch=count)


def _check_record(rec, o, batch, beta, what):
    """[loss | weight | recon | kl] against the oracle; returns the worst relative deviation."""
    assert rec[1] == batch, f"{what}: weight {rec[1]} != {batch}"
    assert abs(rec[0] - (rec[2] + beta * rec[3])) <= 1e-12 * abs(rec[0]), f"{what}: loss != recon + beta * kl"
    worst = 0.0
    for got, name in ((rec[0], "loss"), (rec[2], "recon"), (rec[3], "kl")):
        dev = abs(got - o[name]) / abs(o[name])
        worst = max(worst, dev)
        assert dev < REC_TOL, f"{what}: {name} record {got!r} vs {o[name]!r} ({dev:.2e})"
    return worst


def _check_grads(eng, o, what):
    g = eng.grads_view().cpu().numpy()
    worst = 0.0
    for l, (gw, gb) in enumerate(o["grads"]):
        wo, bo = eng.offsets[l]
        ew, eb = rel_err(g[wo:wo + gw.size].reshape(gw.shape), gw), rel_err(g[bo:bo + gb.size], gb)
        worst = max(worst, ew, eb)
        assert ew < GRAD_TOL, f"{what}: layer {l} weight gradient {ew:.2e}"
        assert eb < GRAD_TOL, f"{what}: layer {l} bias gradient {eb:.2e}"
    return worst


def _fused_step(c, cursor, tr, what):
    """train_step (an evaluation step of CURSOR_ROWS rows first when `cursor`): path, tile rows, record, every gradient."""
    eng = _engine(c, max(c["batch"], CURSOR_ROWS))
    if cursor:   # changes no parameter; the training step's eps rows then start at row 7: an odd element offset for odd d
        eng.eval_step(torch.from_numpy(c["Xn"]).cuda(), row0=0, batch=CURSOR_ROWS)
        assert eng.noise_position() == CURSOR_ROWS
    Xd = torch.from_numpy(c["Xn"]).cuda()
    eng.train_step(Xd, **_kw(c))
    assert eng.last_path() == (1 if tr else 0), "the fused kernel did not take this step" if tr else "fused past 512 tiles"
    assert tile_rows(eng) == tr
    assert eng.noise_position() == c["e0"] + c["batch"]
    wr = _check_record(eng.read_log()[-1], c["o"], c["batch"], c["beta"], what)
    wg = _check_grads(eng, c["o"], what)
    eng.close()
    print(f"{what}: worst record deviation {wr:.2e}, worst gradient deviation from float64 {wg:.2e}")


def _layer_step(c, whole_step, what, z_atol=Z_ATOL):
    """forward + backward (or train_step on a network too wide for LDS) on the layer-by-layer path: z, [SSE | KL sum], the
    record and every gradient."""
    eng = _engine(c, c["batch"])
    Xd = torch.from_numpy(c["Xn"]).cuda()
    if whole_step:
        eng.train_step(Xd, **_kw(c))
    else:
        eng.forward(Xd, **_kw(c))
        eng.backward(Xd, **_kw(c))
    assert eng.last_path() == 0 and tile_rows(eng) == 0
    assert eng.noise_position() == c["batch"]
    o = c["o"]
    z = eng.latent_sample(c["batch"]).cpu().numpy()
    stats = eng.stats_view().cpu().numpy()
    wz = float(np.max(np.abs(z - o["z"]) - 1e-5 * np.abs(o["z"])))   # what rtol = 1e-5 leaves for atol
    ws = max(abs(stats[0] - o["SSE"]) / abs(o["SSE"]), abs(stats[1] - o["KL"]) / abs(o["KL"]))
    print(f"{what}: z beyond rtol 1e-5 by {wz:.2e}, [SSE | KL sum] deviation {ws:.2e}")
    np.testing.assert_allclose(z, o["z"], rtol=1e-5, atol=z_atol, err_msg=f"{what}: z")
    assert ws < REC_TOL, f"{what}: [SSE | KL sum] {stats} vs {o['SSE']!r}, {o['KL']!r}"
    wr = _check_record(eng.read_log()[0], o, c["batch"], c["beta"], what)
    wg = _check_grads(eng, o, what)
    eng.close()
    print(f"{what}: worst z deviation {np.max(np.abs(z - o['z'])):.2e}, sums {ws:.2e}, record {wr:.2e}, gradient vs float64 {wg:.2e}")


@pytest.mark.parametrize("key,d,batch,form,beta,cursor,tr", FUSED_CASES)
def test_fused_vae_step_matches_float64_oracle(key, d, batch, form, beta, cursor, tr):
    """a. One train_step of snet_ae_kernel<16 | 32, true> (z sampling, KL partials, dL/dz -> [dL/dmu | dL/dlv] in LDS) at
    d = 1 .. 8, at the tile edges (a batch shorter than a tile, a last tile of one row, 2048 / 2049 rows, 16384 / 16385
    rows), gathered and contiguous, with and without the noise cursor moved first."""
    _fused_step(prepare_step(key, d, batch, form, beta, cursor), cursor, tr, f"fused {key} d={d} batch={batch} {form} beta={beta}")


@pytest.mark.parametrize("key,d,batch,form,beta", LAYER_CASES)
def test_layer_path_vae_step_matches_float64_oracle(key, d, batch, form, beta):
    """b. vae_sample_kernel, latent_backward_layer and vae_sample_backward_kernel at d = 1 .. 8 and at the block edges of the
    256-row sampling kernels.  z holds rtol 1e-5 / atol 1e-6 on the small networks; on W atol is Z_ATOL_W = 4.9e-6, four times
    the 1.23e-6 a float32 torch run of the same step leaves beyond rtol (see Z_ATOL_W; the kernel: 1.33e-6)."""
    _layer_step(prepare_step(key, d, batch, form, beta), key == "W", f"layer {key} d={d} batch={batch} {form} beta={beta}",
                Z_ATOL_W if key == "W" else Z_ATOL)


@pytest.mark.parametrize("key,path,batch,shift", LARGE_LV_CASES)
def test_large_log_variances(key, path, batch, shift):
    """c. The log-variance head's bias moved to +8 / -8 (exp(lv) from about 3e-4 to 3e3), d = 3, beta = 1, on both paths:
    the same relative bounds."""
    c = prepare_step(key, 3, batch, "idx", 1.0, lv_shift=shift)
    assert np.max(np.abs(c["o"]["lv"] - shift)) <= 4.0   # the shift really is where the log-variances sit
    what = f"lv bias {shift:+.0f}, path {path}, batch {batch}"
    if path == 1:
        _fused_step(c, False, 16, what)
    else:
        _layer_step(c, False, what)


@pytest.mark.parametrize("key,d,batch,form,path,tr", EVAL_CASES)
def test_vae_evaluation_records_match_float64_oracle(key, d, batch, form, path, tr):
    """d. eval_step, then eval_steps with 5 batches in one call (fused: ONE launch, batch j's noise at (j * R + r0) * d and
    its KL partials at j * wgpb): every record against the oracle's forward pass on that batch's rows and eps rows; the
    noise cursor advances by the rows consumed; no parameter changes."""
    c = prepare_eval(key, d, batch, form)
    eng = _engine(c, batch)
    Xd = torch.from_numpy(c["Xn"]).cuda()
    before = eng.params_view().clone()
    eng.eval_step(Xd, **_kw(c, 0, batch))
    assert eng.noise_position() == batch and eng.last_path() == path and tile_rows(eng) == tr
    kw = _kw(c, batch, EVAL_BATCHES * batch)
    kw.pop("batch", None)
    eng.eval_steps(Xd, batch, EVAL_BATCHES, **kw)
    assert eng.noise_position() == c["nb"] * batch and eng.last_path() == path and tile_rows(eng) == tr
    rec = eng.read_log()
    assert rec.shape == (c["nb"], 4)
    what = f"eval {key} d={d} batch={batch} {form}"
    worst = max(_check_record(rec[j], c["o"][j], batch, c["beta"], f"{what}, batch {j}") for j in range(c["nb"]))
    assert torch.equal(eng.params_view(), before), "an evaluation pass changed a parameter"
    eng.close()
    print(f"{what}: worst record deviation from float64 {worst:.2e}")


@pytest.mark.parametrize("dims,acts,match", [
    ([20, 12, 18, 12, 20], ["tanh", None, "tanh", None], "18"),                  # a head layer of 18 columns: d = 9
    ([20, 12, 5, 12, 20], ["tanh", None, "tanh", None], r"2 \* d <= 16"),        # a head layer of 5 columns: no [mean | log-variance] split
    ([20, 12, 6, 12, 20], ["tanh", "tanh", "tanh", None], "no activation"),      # an activation on the heads
])
def test_vae_refusals(dims, acts, match):
    """e. Refused at creation with the engine's error: nothing is allocated or launched."""
    from deep_cartograph_amd import hip

    with pytest.raises(hip.DcvError, match=match):
        hip.Mlp("vae", dims, acts, max_batch=64, latent_layer=2)
