"""Dropout and batch normalisation of the MLP engine, with the dropout masks pinned by an oracle that is not the engine
(tests/dropout_oracle.py: Philox-4x32 restated in NumPy, checked against Random123's known answers on the CPU).

A. dcv_mlp_dropout_mask equals the oracle bit for bit, over every field of the keying.
B. H_train = H_eval * mask bit for bit in every tile family of the forward products (plans asserted from hip.gemm_log()).
C. One training step under dropout against float64 autograd, given the ORACLE's masks, where the backward had not run.
D. Dropout and batch normalisation on the same layer: first step against float64, four SGD steps against float32.
E. The sensitivity pass through normalised layers (evaluation mode), every model kind.
Run on the GPU box: python -m pytest tests -m gpu"""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import nn as onn
from tests import dropout_oracle as do
from tests.test_mlp_gpu import _ncu, ar_features, assert_within, linears_of, normalized, push_params, rel_err
from tests.test_training_options_gpu import _bn_modules, _engine_grads, _queue_masks
from tests.test_vae_gpu import REF_ACTS, REF_DIMS
from tests.test_vae_gpu import _init as vae_init

pytestmark = pytest.mark.gpu

SEED_HI = 0x1234_5678_9ABC_DEF0   # a seed whose high word is in use (key word 1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_bits(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype == np.float32, (what, got.shape, exp.shape, got.dtype)
    bad = _bits(got) != _bits(exp)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}"


# ============================================================================= A. the mask hook against the oracle
MASK_WIDTHS = [(1, 130), (3, 33), (4, 5), (130, 1), (33, 3), (5, 4)]     # (width behind Linear 0, behind Linear 2): all six at both layers
MASK_STEPS = [0, 1, 2 ** 31 + 5]


@pytest.mark.parametrize("p", [1e-12, 0.1, 0.5, 0.999])
@pytest.mark.parametrize("seed", [77, SEED_HI])
def test_dropout_mask_equals_the_oracle_bit_for_bit(seed, p):
    """dcv_mlp_dropout_mask against tests/dropout_oracle.mask, element-wise equality, no exclusions: widths 1, 3, 4, 5, 33, 130
    at layers 0 and 2, rows 1 and 257 for every (step, rank) of steps {0, 1, 2^31 + 5} x ranks {0, 3}, and 70 000 rows (row
    indices above 2^16; at width 130 that is 2.3 M quads, more than the hook's 4096 blocks x 256 threads: the grid-stride
    loop) at one (step, rank) per (engine, layer), rotating so that every pair is taken.  p = 1e-12 gives thr = 1 (only
    the draw 0 is dropped), p = 0.999 the scale 1000.01.
    MEASURED on MI355X: 0 differing elements in every case."""
    from deep_cartograph_amd import hip

    turn = 0
    for w0, w2 in MASK_WIDTHS:
        dims = [8, w0, 8, w2, 2]
        eng = hip.Mlp("deep_tica", dims, [None] * 4, max_batch=8, lag=1, dropout=[p, 0.0, p, 0.0], seed=seed)
        for layer in (0, 2):
            width = dims[layer + 1]
            combos = [(step, rank) for step in MASK_STEPS for rank in (0, 3)]
            for step, rank in combos:
                eng.set_rank(rank)
                for rows in (1, 257):
                    got = eng.dropout_mask(layer, step, rows).cpu().numpy()
                    assert_same_bits(got, do.mask(seed, rank, layer, step, rows, width, p), (w0, w2, layer, step, rank, rows))
            step, rank = combos[turn % len(combos)]
            turn += 1
            eng.set_rank(rank)
            got = eng.dropout_mask(layer, step, 70_000).cpu().numpy()
            assert_same_bits(got, do.mask(seed, rank, layer, step, 70_000, width, p), (w0, w2, layer, step, rank, 70_000))
        eng.close()


@pytest.mark.parametrize("p", [1.0, 1.5, 0.99999999, -0.1, float("nan")])
def test_dropout_probability_outside_the_unit_interval_is_refused(p):
    """dcv_mlp_create refuses p >= 1 (1 / (1 - p) is infinite or negative; 0.99999999 IS 1 as the float32 the descriptor
    carries), a negative and a non-finite p with DCV_EINVAL (-1); the same descriptor with p = 0.5 is accepted."""
    from deep_cartograph_amd import hip

    with pytest.raises(hip.DcvError, match=r"code -1\).*dropout\[1\]"):
        hip.Mlp("deep_tica", [8, 6, 4, 2], ["tanh", "tanh", None], max_batch=16, lag=1, dropout=[0.0, p, 0.0])
    hip.Mlp("deep_tica", [8, 6, 4, 2], ["tanh", "tanh", None], max_batch=16, lag=1, dropout=[0.0, 0.5, 0.0]).close()


# ============================================================================= B. the mask in every forward tile family
def _identity_shapes(name):
    """name -> (K, N, rows, hidden activation, tile the plan rule must pick): layer 0 of the autoencoder [K, N, 12, 2, K] (the
    12-wide layer behind it keeps the narrow-layer fusion off).  pick_cfg<kNT> with want = 2 * CUs workgroups: N <= 32 ->
    128 x 32; fewer than `want` 128-row tiles and rows <= 256 -> 64 x 128; fewer than want / 2 64-row tiles -> 32 x 128;
    between want / 2 and want 64-row tiles and N % 64 == 0 -> 64 x 64; from `want` 128-row tiles up -> 128 x 128."""
    n = _ncu()
    return {
        "64x128": (40, 130, 250, "softplus", (64, 128)),      # a 58-row tail tile; columns 128 + 2
        "32x128": (37, 33, 300, "elu", (32, 128)),            # K % 4 != 0: scalar loaders (vec = False); a 12-row tail tile
        "128x32": (40, 5, 300, "custom_sigmoid", (128, 32)),  # one ragged column quad, a 44-row tail tile
        "64x64": (24, 512, 64 * ((n + 3) // 4) + 37, "shifted_softplus", (64, 64)),   # 4 column tiles x (CUs / 4 + 1) row tiles
        "128x128-tanh": (256, 256, 128 * n + 110, "tanh", (128, 128)),               # case b's layer 0 (test_mlp_gpu._big_case)
        "128x128-leaky_relu": (256, 256, 128 * n + 110, "leaky_relu", (128, 128)),   # ... with the sign-mask store
    }[name]


@pytest.mark.parametrize("mode", ["split", "native"])
@pytest.mark.parametrize("case", ["64x128", "32x128", "128x32", "64x64", "128x128-tanh", "128x128-leaky_relu"])
def test_training_forward_is_the_evaluation_forward_times_the_mask(case, mode):
    """For the first dropout layer, H_train == H_eval * mask(layer, step) bit for bit: the epilogue computes act(x + b) and
    then one float32 multiply by 0 or 1 / (1 - p) -- with the mask taken from the ORACLE, not from the engine.  Both forwards
    must have launched the same plans and layer 0 the tile family the case is named for (hip.gemm_log()).  The checked forward is
    training step 1 (a few rows went through step 0), so a generator that ignored the step word fails here too.
    gemm_log().vec names the 16-byte LOADERS (False for K = 37); the stores are 16-byte on interior tiles and
    store_quad(nvalid) on the tail row tile / the ragged column quad, and every case but the two 128 x 128 ones has both.
    Guard elements: layer_output has exactly `width` columns, and the rows of the engine's buffer behind the call's rows
    (max_batch = rows + 64) keep the bits they had before the two forwards.
    MEASURED on MI355X (256 CUs), both flavours: 0 differing elements in every case."""
    from deep_cartograph_amd import hip

    K, N, M, act, tile = _identity_shapes(case)
    p, seed = 0.3, SEED_HI + 17
    X = np.random.default_rng(3).standard_normal((M, K), dtype=np.float32)
    torch.manual_seed(21)
    dims = [K, N, 12, 2, K]
    lins = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(4)]
    prev = hip.get_gemm_mode()
    hip.set_gemm_mode(mode)
    try:
        eng = hip.Mlp("ae", dims, [act, "tanh", None, None], max_batch=M + 64, latent_layer=3, dropout=[p, 0.0, 0.0, 0.0], seed=seed)
        push_params(eng, lins)
        eng.set_feature_range(np.ones(K, np.float32))
        Xd = torch.from_numpy(X).cuda()
        eng.forward(Xd, row0=0, batch=8, train=True)   # training step 0 on a few rows: the identity is checked at step 1
        guard0 = eng.layer_output(0, M + 64)[M:].cpu().numpy()
        hip.gemm_log_reset()
        eng.forward(Xd, row0=0, batch=M, train=False)
        log_eval = hip.gemm_log()
        H_eval = eng.layer_output(0, M).cpu().numpy()
        step = eng.dropout_step()
        hip.gemm_log_reset()
        eng.forward(Xd, row0=0, batch=M, train=True)
        log_train = hip.gemm_log()
        H_train = eng.layer_output(0, M).cpu().numpy()
        guard1 = eng.layer_output(0, M + 64)[M:].cpu().numpy()
        assert eng.last_path() == 0 and step == 1 and eng.dropout_step() == 2
        eng.close()
    finally:
        hip.set_gemm_mode(prev)
    assert log_train == log_eval, (log_train, log_eval)
    e = log_train[0]
    assert (e.form, e.mode, e.tm, e.tn, e.split) == ("single", "nt", *tile, mode == "split"), log_train
    assert e.vec == (K % 4 == 0), e
    assert H_train.shape == H_eval.shape == (M, N)
    assert np.isfinite(H_eval).all()
    assert_same_bits(H_train, H_eval * do.mask(seed, 0, 0, step, M, N, p), f"{case} {mode}")
    assert_same_bits(guard1, guard0, f"{case} {mode}: rows behind the call")


@pytest.mark.parametrize("mode", ["split", "native"])
@pytest.mark.parametrize("d", [4, 8])
def test_fused_head_forward_under_dropout(d, mode):
    """EpiBiasActHead<4> / <8> (Deep-TICA 64 -> 128 -> d through an index list: 2 x 125 rows in both forwards, a 58-row tail
    tile) with dropout on the hidden layer: H_train == H_eval * oracle mask bit for bit, and the head's output Z against
    float64 computed from the engine's own dropped H, within the element-wise bound of forward_layers_against_float64
    (fp32 product bound + 1e-6 + 4 ulp).
    MEASURED on MI355X, both flavours: 0 differing elements of H; Z at most 0.057 of the bound."""
    from deep_cartograph_amd import hip

    B, lag, p, seed = 125, 3, 0.2, 77
    dims = [64, 128, d]
    Xn = np.random.default_rng(4).standard_normal((400, 64), dtype=np.float32)
    idx = torch.randperm(400 - lag, generator=torch.Generator().manual_seed(5))[:B].contiguous()
    torch.manual_seed(22)
    lins = [torch.nn.Linear(64, 128), torch.nn.Linear(128, d)]
    prev = hip.get_gemm_mode()
    hip.set_gemm_mode(mode)
    try:
        eng = hip.Mlp("deep_tica", dims, ["tanh", None], max_batch=B, lag=lag, tica_reg=1e-6, dropout=[p, 0.0], seed=seed)
        push_params(eng, lins)
        Xd, idx_d = torch.from_numpy(Xn).cuda(), idx.cuda()
        eng.forward(Xd, idx=idx_d[:8].contiguous(), train=True)   # training step 0: the identity is checked at step 1
        hip.gemm_log_reset()
        eng.forward(Xd, idx=idx_d, train=False)
        log_eval = hip.gemm_log()
        H_eval = eng.layer_output(0, 2 * B).cpu().numpy()
        step = eng.dropout_step()
        hip.gemm_log_reset()
        eng.forward(Xd, idx=idx_d, train=True)
        log_train = hip.gemm_log()
        H_train = eng.layer_output(0, 2 * B).cpu().numpy()
        Z = eng.layer_output(1, 2 * B).cpu().numpy()
        assert eng.last_path() == 0 and step == 1
        eng.close()
    finally:
        hip.set_gemm_mode(prev)
    assert log_train == log_eval, (log_train, log_eval)
    assert sum(1 for e in log_train if e.mode == "nt") == 1, log_train   # the head rode in layer 0's epilogue
    e = log_train[0]
    assert (e.mode, e.tm, e.tn, e.split, e.gather) == ("nt", 64, 128, mode == "split", True), log_train
    assert H_train.shape == (2 * B, 128) and Z.shape == (2 * B, d)
    assert_same_bits(H_train, H_eval * do.mask(seed, 0, 0, step, 2 * B, 128, p), f"head {d} {mode}")
    h = H_train.astype(np.float64)
    W, b = lins[1].weight.detach().double().numpy(), lins[1].bias.detach().double().numpy()
    ref = h @ W.T + b
    bound = 4e-7 * (np.abs(h) @ np.abs(W).T + np.abs(b)) + 1e-6 + 4 * 2.0 ** -24 * np.abs(ref)
    assert_within(f"head {d} {mode}: Z", Z, ref, bound)


# ============================================================================= C / D. training steps given the oracle's masks
T, F = True, False
# Inputs.  Data and weight seeds of c1 / d2 (33-17-5-3, three outputs from five hidden units) are chosen so that the batch's
# C0 is well conditioned: with the seeds of the other cases the float32 torch-CPU oracle itself misses the 5e-5 gradient
# tolerance against float64 on the same inputs and masks (2.3e-4 on c1, 6.8e-5 on d2); with these it is at 1.5e-6 / 1.7e-6.
# d4 (two rows through a normalisation): dz = weight * invstd * (dY - mean dY - xhat mean(dY xhat)) is the small difference
# eps / (h^2 + eps) of terms of size 1, h = half the distance of the two values of a column -- in ANY float32 implementation,
# so with activations of size 1 the float32 oracle misses float64 by 5e-3 on layer 0.  Rows of size 0.03 and no layer-0 bias
# (h^2 of the order of eps = 1e-5, half of the units on either side of the ReLU kink in either row) leave it at 9e-7.
# Every figure here is the float32 oracle's deviation from the float64 one, measured on the CPU; none comes from the engine.
CASES = {
    # C: backward under dropout where it had not run
    "c1": dict(kind="deep_tica", dims=[33, 17, 5, 3], acts=["softplus", "shifted_softplus", None], drops=[0.25, 0.1, 0.0], batch=257,
               gather=True, lag=4, weight_seed=2, tol=5e-5),
    "c2": dict(kind="deep_tica", dims=[64, 128, 4], acts=["custom_sigmoid", None], drops=[0.2, 0.0], batch=900, gather=False, lag=5,
               row0=11, n=2000, tol=5e-5),
    "c3": dict(kind="ae", dims=[40, 24, 8, 2, 8, 24, 40], latent=3, acts=["elu", "tanh", None, "tanh", "elu", None],
               drops=[0.1, 0.0, 0.0, 0.0, 0.2, 0.15], batch=700, row0=100, tol=1e-4),
    # D: dropout and batch normalisation on the same layer (the table of the issue)
    "d1": dict(kind="deep_tica", dims=[40, 24, 12, 2], acts=["leaky_relu", "tanh", None], drops=[0.1, 0.2, 0.0], bn=[T, T, F], batch=384,
               gather=False, lag=3, row0=5, tol=5e-5),
    "d2": dict(kind="deep_tica", dims=[33, 17, 5, 3], acts=["elu", "softplus", None], drops=[0.25, 0.1, 0.0], bn=[T, T, F], batch=257,
               gather=True, lag=4, data_seed=3, weight_seed=4, tol=5e-5),
    "d3": dict(kind="ae", dims=[40, 300, 2, 130, 40], latent=2, acts=["shifted_softplus", None, "custom_sigmoid", None],
               drops=[0.1, 0.0, 0.2, 0.1], bn=[T, F, T, T], batch=70, row0=5, tol=5e-5),
    "d4": dict(kind="ae", dims=[12, 8, 2, 8, 12], latent=2, acts=["relu", None, "relu", None], drops=[0.5, 0.0, 0.0, 0.0],
               bn=[T, F, F, F], batch=2, row0=5, dead_unit=3, data="small_rows", tol=5e-5),
}
ENGINE_SEED = SEED_HI + 5


def _setup(name):
    """The case's oracle model (float32, seeded), its data and its batches: everything but the engine, so that the float32
    oracle can be run against the float64 one without a GPU."""
    c = CASES[name]
    dims, acts, drops = c["dims"], c["acts"], c["drops"]
    L = len(dims) - 1
    bnf = c.get("bn") or [False] * L
    n, lag, B = c.get("n", 1600), c.get("lag", 0), c["batch"]
    if c.get("data") == "small_rows":   # rows of size 0.03 (see CASES["d4"])
        rng = np.random.default_rng(c.get("data_seed", 17))
        Xn = (0.03 * rng.standard_normal((n, dims[0]))).astype(np.float32)
    else:
        Xn = normalized(ar_features(n, dims[0], c.get("data_seed", 17)))[0]
    torch.manual_seed(c.get("weight_seed", 12))
    none0 = lambda ps: [p if p else None for p in ps]
    if c["kind"] == "ae":
        k = c["latent"]
        ref = onn.AEModel(dims[:k + 1], acts[:k], none0(drops[:k]), dims[k:], acts[k:], none0(drops[k:]), None, None,
                          enc_bn=bnf[:k], dec_bn=bnf[k:])
        seqs = lambda m: [m.encoder, m.decoder]
    else:
        ref = onn.DeepTICAModel(dims, acts, none0(drops), None, None, 1e-6, batchnorm=bnf)
        seqs = lambda m: [m.nn]
    lins_of = lambda m: [x for q in seqs(m) for x in linears_of(q)]
    bns_of = lambda m: [x for q in seqs(m) for x in _bn_modules(q)]
    with torch.no_grad():   # not the trivial weight 1 / bias 0
        for b in bns_of(ref):
            b.weight.uniform_(0.5, 1.5)
            b.bias.uniform_(-0.3, 0.3)
        if c.get("data") == "small_rows":   # ... and no bias: layer 0's pre-activations are small, half of them on either side of the kink
            lins_of(ref)[0].bias.zero_()
        if "dead_unit" in c:   # relu(w x - 10) = 0 on every row: a column of variance exactly 0 in front of the normalisation
            lins_of(ref)[0].bias[c["dead_unit"]] = -10.0
    bn_state, it = [], iter(bns_of(ref))
    for flag in bnf:
        b = next(it) if flag else None
        bn_state.append(None if b is None else {"weight": b.weight.detach().numpy().copy(), "bias": b.bias.detach().numpy().copy(),
                                                "running_mean": b.running_mean.numpy().copy(), "running_var": b.running_var.numpy().copy(),
                                                "num_batches_tracked": 0})
    linears = [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in lins_of(ref)]
    gen = torch.Generator().manual_seed(7)
    batches = []
    for i in range(6):
        if c.get("gather"):
            batches.append(torch.randperm(n - lag, generator=gen)[:B].contiguous())
        else:
            r0 = c.get("row0", 0) + (i * 131) % (n - B - lag - c.get("row0", 0))
            batches.append(torch.arange(r0, r0 + B))

    def engine_rows(i):
        return dict(idx=batches[i].cuda()) if c.get("gather") else dict(row0=int(batches[i][0]), batch=B)

    def ref_step(model, x, i):
        idx = batches[i]
        return model.step(x[idx])[0] if c["kind"] == "ae" else model.step(x[idx], x[idx + lag])[0]

    def give_masks(model, step, dtype):
        """the oracle's masks of training step `step` into the model's dropout modules (Deep-TICA: the x_t call takes rows
        [0, B) of the engine's 2 B rows, the x_lag call rows [B, 2 B))"""
        layers = [l for l in range(L) if drops[l] > 0]
        rows = B if c["kind"] == "ae" else 2 * B
        mk = {l: do.mask(ENGINE_SEED, 0, l, step, rows, dims[l + 1], drops[l]) for l in layers}
        if c["kind"] == "ae":
            k = c["latent"]
            mods = _queue_masks(model.encoder, [[mk[l] for l in layers if l < k]]) + _queue_masks(model.decoder, [[mk[l] for l in layers if l >= k]])
        else:
            mods = _queue_masks(model.nn, [[mk[l][:B] for l in layers], [mk[l][B:] for l in layers]])
        for dm in mods:
            dm.queue = [q.to(dtype) for q in dm.queue]

    # gradient tensors that are exactly zero by an invariance of the loss (see grad_deviation)
    zero = []
    if c["kind"] == "deep_tica" and drops[L - 1] == 0 and not bnf[L - 1]:
        zero.append(f"L{L - 1}.bias")            # a constant shift of the outputs: removed with the batch mean
        if bnf[L - 2]:
            zero.append(f"BN{L - 2}.bias")       # the bias of the normalisation feeding that Linear: the same constant shift
    for l in range(L):
        if bnf[l] and acts[l] is None and drops[l] == 0:
            zero.append(f"L{l}.bias")            # a constant shift right in front of a normalisation (no activation, no mask between)
    return SimpleNamespace(c=c, name=name, dims=dims, acts=acts, drops=drops, bnf=bnf, L=L, lag=lag, B=B, Xn=Xn, ref=ref, seqs=seqs,
                           lins_of=lins_of, bns_of=bns_of, bn_state=bn_state, linears=linears, engine_rows=engine_rows, ref_step=ref_step,
                           give_masks=give_masks, zero=zero)


def _engine(s):
    from deep_cartograph_amd import hip

    c = s.c
    kw = dict(max_batch=s.B, optimizer="SGD", lr=0.05, momentum=0.5, dropout=s.drops, batchnorm=s.bnf, seed=ENGINE_SEED)
    if c["kind"] == "ae":
        eng = hip.Mlp("ae", s.dims, s.acts, latent_layer=c["latent"], **kw)
        eng.set_feature_range(np.ones(s.dims[0], np.float32))
    else:
        eng = hip.Mlp("deep_tica", s.dims, s.acts, lag=s.lag, tica_reg=1e-6, **kw)
    eng.set_linears(s.linears, bn=s.bn_state)
    return eng


def named_gradients(s, model, eng=None):
    """name -> gradient tensor of the oracle model, or of the engine (same names, same shapes)"""
    out = {}
    lins = s.lins_of(model)
    linear = _engine_grads(eng, lins) if eng is not None else [(lin.weight.grad.numpy(), lin.bias.grad.numpy()) for lin in lins]
    g = eng.grads_view().cpu().numpy() if eng is not None else None
    it = iter(s.bns_of(model))
    for l in range(s.L):
        out[f"L{l}.weight"], out[f"L{l}.bias"] = linear[l]
        if s.bnf[l]:
            b = next(it)
            if eng is None:
                out[f"BN{l}.weight"], out[f"BN{l}.bias"] = b.weight.grad.numpy(), b.bias.grad.numpy()
            else:
                go, bo_ = eng.bn_offsets[l]
                out[f"BN{l}.weight"], out[f"BN{l}.bias"] = g[go:go + b.weight.numel()].copy(), g[bo_:bo_ + b.bias.numel()].copy()
    return out


def grad_deviation(got, exp, allowed_zero):
    """Worst relative deviation (max |got - exp| / max |exp| per tensor) over the gradient tensors.  The exact-zero rule of
    test_batchnorm_training_matches_torch: a tensor whose float64 gradient is below 1e-12 in EVERY entry is exactly zero by an
    invariance of the loss -- a constant shift in front of a normalisation with nothing nonlinear in between, or in front of
    Deep-TICA's mean removal (its last bias, or the bias of a normalisation feeding its last Linear) -- and the engine may
    hold only rounding noise there, below 1e-6 of the step's largest weight gradient.  Only the tensors that argument names
    (`allowed_zero`) may be skipped that way; their count is asserted."""
    gscale = max(float(np.max(np.abs(v))) for k, v in exp.items() if k.endswith(".weight") and k.startswith("L"))
    worst, skipped = ("", 0.0), []
    assert list(got) == list(exp)
    for k in exp:
        assert got[k].shape == exp[k].shape, k
        if np.max(np.abs(exp[k])) < 1e-12:
            assert np.max(np.abs(got[k])) < 1e-6 * gscale, (k, np.max(np.abs(got[k])), gscale)
            skipped.append(k)
            continue
        dev = rel_err(got[k], exp[k])
        if dev > worst[1]:
            worst = (k, dev)
    assert set(skipped) <= set(allowed_zero) and len(skipped) <= len(allowed_zero), (skipped, allowed_zero)
    return worst, skipped


def first_step_against_float64(s, eng):
    """forward(train) + backward of batch 0 on the engine against the float64 oracle given the oracle's masks; returns the
    loss deviation (relative to max(1, |loss|)) and the worst gradient deviation"""
    Xd, xt = torch.from_numpy(s.Xn).cuda(), torch.from_numpy(s.Xn).double()
    ref64 = copy.deepcopy(s.ref).double().train()
    eng.reset_log(8)
    step = eng.dropout_step()
    eng.forward(Xd, train=True, **s.engine_rows(0))
    eng.backward(Xd, **s.engine_rows(0))
    assert eng.last_path() == 0 and eng.dropout_step() == step + 1
    s.give_masks(ref64, step, torch.float64)
    loss = s.ref_step(ref64, xt, 0)
    loss.backward()
    loss = float(loss.detach())
    dloss = abs(eng.read_log()[0, 0] - loss) / max(1.0, abs(loss))
    worst, skipped = grad_deviation(named_gradients(s, ref64, eng), named_gradients(s, ref64), s.zero)
    print(f"{s.name}: first step: loss {loss:.6f}, deviation {dloss:.2e}; worst gradient deviation {worst[1]:.2e} ({worst[0]}); "
          f"exactly-zero tensors {skipped}")
    return dloss, worst, skipped


@pytest.mark.parametrize("name", ["c1", "c2", "c3"])
def test_dropout_step_matches_float64_given_the_oracle_masks(name):
    """One training step under dropout against float64 autograd, the masks from tests/dropout_oracle.py (the existing dropout
    tests hand the oracle the engine's own masks): loss within 2e-5 max(1, |loss|), every gradient tensor within 5e-5
    (Deep-TICA) / 1e-4 (AE) of its largest entry; Deep-TICA's last bias by the exact-zero rule (grad_deviation).
    c1: odd widths 33-17-5-3, softplus / shifted softplus: the derivative from the scaled stored output, gathered rows.
    c2: 64-128-4, custom sigmoid: the fused-head backward with drop_prev / hscale_prev.
    c3: autoencoder with dropout on the decoder's OUTPUT layer (the drop arm of ae_dY_kernel), elu / tanh hidden layers.
    MEASURED on MI355X: loss deviation 8.9e-11 / 5.2e-9 / 4.1e-9, worst gradient tensor 4.5e-6 (c1, bias 1) / 3.0e-7 / 5.4e-7;
    the float32 torch-CPU oracle on the same inputs and masks: 1.5e-6 / 1.3e-6 / 6.3e-7."""
    s = _setup(name)
    eng = _engine(s)
    dloss, worst, skipped = first_step_against_float64(s, eng)
    eng.close()
    assert dloss < 2e-5
    assert worst[1] < s.c["tol"], worst
    assert sorted(skipped) == sorted(s.zero)


@pytest.mark.parametrize("name", ["d1", "d2", "d3", "d4"])
def test_dropout_and_batchnorm_on_the_same_layer(name):
    """Dropout and batch normalisation behind the same Linear (the reference's default dropout [0.1, 0.1] plus `batchnorm:
    true`): the statistics are taken over the post-dropout output, the backward un-scales the kept values (hscale) inside
    bn_bwd_apply_kernel's drop arm; Deep-TICA: each half of the batch has its own mask rows and its own statistics.
    (i) first step against float64: loss (2e-5), Linear and normalisation gradients (5e-5), the exact-zero rule;
    (ii) fresh state, four SGD-with-momentum steps (lr 0.05, momentum 0.5; not Adam: DESIGN.md section 2, noise-driven
    parameters) against the float32 oracle, each given that step's masks: losses, parameters, running mean / variance,
    num_batches_tracked with the tolerances of test_batchnorm_training_matches_torch; (iii) an evaluation step and the
    inference path drop nothing and use the running statistics.
    d1: two halves of 384 rows = row blocks of 256 + 128 each.  d2: odd widths (c & 3), 257 rows = a one-row tail block per
    half.  d3: 300 columns (second column pass, one row lane), 130 (126 idle column threads), 2 (128 row lanes for 70 rows),
    normalisation and dropout behind the output layer.  d4: two rows (n - 1 = 1) and a unit that is dead on the whole batch
    (variance exactly 0, invstd = 1 / sqrt(eps)).
    MEASURED on MI355X (d1 / d2 / d3 / d4): first step: loss 1.8e-8 / 3.5e-8 / 6.4e-9 / 2.3e-9, worst gradient tensor 7.9e-7 /
    4.8e-7 / 4.9e-6 / 1.8e-6 (float32 torch-CPU oracle on the same inputs and masks: 4.6e-7 / 1.7e-6 / 6.5e-6 / 9.3e-7); after
    four steps: parameters 8.9e-8 / 2.1e-7 / 3.0e-8 / 1.7e-6, running mean 2.2e-8 / 3.0e-8 / 3.0e-8 / 6.5e-9, running variance
    (relative) 1.2e-7 / 1.9e-7 / 8.9e-8 / 0."""
    s = _setup(name)
    eng = _engine(s)
    Xd, xt = torch.from_numpy(s.Xn).cuda(), torch.from_numpy(s.Xn)
    # (i)
    dloss, worst, skipped = first_step_against_float64(s, eng)
    if "dead_unit" in s.c:
        assert not eng.layer_output(0, s.B)[:, s.c["dead_unit"]].any()   # the dead unit is dead on the engine too
    assert dloss < 2e-5
    assert worst[1] < s.c["tol"], worst
    assert sorted(skipped) == sorted(s.zero)
    # (ii) fresh optimiser state, running statistics and step counter
    eng.set_linears(s.linears, bn=s.bn_state)
    ref = s.ref.train()
    opt = torch.optim.SGD(ref.parameters(), lr=0.05, momentum=0.5)
    eng.reset_log(8)
    ref_losses = []
    for i in range(4):
        step = eng.dropout_step()
        assert step == i
        eng.train_step(Xd, **s.engine_rows(i))
        s.give_masks(ref, step, torch.float32)
        opt.zero_grad()
        loss = s.ref_step(ref, xt, i)
        loss.backward()
        opt.step()
        ref_losses.append(float(loss.detach()))
    got_losses = eng.read_log()[:, 0]
    print(f"{name}: losses {got_losses} against {ref_losses}")
    np.testing.assert_allclose(got_losses, ref_losses, rtol=2e-4, atol=2e-5)
    dev = {"w": 0.0, "bn": 0.0, "rm": 0.0, "rv": 0.0}
    for (w, b), lin in zip(eng.get_linears(), s.lins_of(ref)):
        dev["w"] = max(dev["w"], float(np.max(np.abs(w - lin.weight.detach().numpy()))), float(np.max(np.abs(b - lin.bias.detach().numpy()))))
        np.testing.assert_allclose(w, lin.weight.detach().numpy(), atol=5e-5)
        np.testing.assert_allclose(b, lin.bias.detach().numpy(), atol=5e-5)
    got_bn = [b for b in eng.get_bn() if b is not None]
    assert len(got_bn) == len(s.bns_of(ref))
    for gb_, b in zip(got_bn, s.bns_of(ref)):
        dev["bn"] = max(dev["bn"], float(np.max(np.abs(gb_["weight"] - b.weight.detach().numpy()))), float(np.max(np.abs(gb_["bias"] - b.bias.detach().numpy()))))
        dev["rm"] = max(dev["rm"], float(np.max(np.abs(gb_["running_mean"] - b.running_mean.numpy()))))
        dev["rv"] = max(dev["rv"], float(np.max(np.abs(gb_["running_var"] - b.running_var.numpy()) / np.abs(b.running_var.numpy()))))
    print(f"{name}: after 4 steps: parameters {dev['w']:.2e}, normalisation weight / bias {dev['bn']:.2e}, running mean {dev['rm']:.2e}, "
          f"running variance (relative) {dev['rv']:.2e}")
    for gb_, b in zip(got_bn, s.bns_of(ref)):
        np.testing.assert_allclose(gb_["weight"], b.weight.detach().numpy(), atol=5e-5)
        np.testing.assert_allclose(gb_["bias"], b.bias.detach().numpy(), atol=5e-5)
        np.testing.assert_allclose(gb_["running_mean"], b.running_mean.numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(gb_["running_var"], b.running_var.numpy(), rtol=1e-4, atol=1e-6)
        assert gb_["num_batches_tracked"] == int(b.num_batches_tracked) == (4 if s.c["kind"] == "ae" else 8)
    # (iii) evaluation mode: nothing dropped, running statistics, nothing tracked
    ref.eval()
    eng.reset_log(4)
    steps_before = eng.dropout_step()
    eng.eval_step(Xd, **s.engine_rows(5))
    rows = min(600, s.Xn.shape[0])
    with torch.no_grad():
        le = float(s.ref_step(ref, xt, 5))
        exp = (ref.forward_cv(xt[:rows]) if s.c["kind"] == "ae" else ref.forward_nn(xt[:rows])).numpy()
    assert abs(eng.read_log()[0, 0] - le) < 2e-4 * max(1.0, abs(le)), (eng.read_log()[0, 0], le)
    out, _ = eng.infer(Xd[:rows])
    np.testing.assert_allclose(out.cpu().numpy(), exp, atol=5e-5)
    assert eng.dropout_step() == steps_before
    assert [b["num_batches_tracked"] for b in eng.get_bn() if b is not None] == [int(b.num_batches_tracked) for b in s.bns_of(ref)]
    eng.close()


@pytest.mark.parametrize("kind", ["ae", "deep_tica"])
def test_one_row_training_forward_through_a_normalisation_is_refused(kind):
    """torch.nn.BatchNorm1d raises on a training forward call of one row; the engine would compute variance 0 and go on.
    A training forward whose call -- or either Deep-TICA half -- has one row while any layer is normalised is refused with
    DCV_EINVAL (-1) before any launch and before any state moves (dropout step, batches tracked, log); the engine and the
    stream stay usable: the same step with more rows runs, and so does a one-row EVALUATION step of the autoencoder (running
    statistics).  Without a normalisation a one-row training forward is still accepted."""
    from deep_cartograph_amd import hip

    Xd = torch.from_numpy(normalized(ar_features(300, 12, 3))[0]).cuda()
    torch.manual_seed(3)
    if kind == "ae":
        dims, acts, extra = [12, 8, 2, 8, 12], ["tanh", None, "tanh", None], dict(latent_layer=2)
    else:
        dims, acts, extra = [12, 8, 2], ["tanh", None], dict(lag=2, tica_reg=1e-6)
    lins = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]
    bn = [True] + [False] * (len(dims) - 2)
    eng = hip.Mlp(kind, dims, acts, max_batch=16, optimizer="SGD", lr=0.01, dropout=[0.1] + [0.0] * (len(dims) - 2), batchnorm=bn, **extra)
    push_params(eng, lins)
    if kind == "ae":
        eng.set_feature_range(np.ones(12, np.float32))
    eng.reset_log(8)
    one = dict(idx=torch.tensor([7]).cuda())
    for call in (lambda: eng.forward(Xd, train=True, **one), lambda: eng.train_step(Xd, **one), lambda: eng.train_step(Xd, row0=3, batch=1),
                 lambda: eng.train_steps(Xd, 1, 2, row0=0)):
        with pytest.raises(hip.DcvError, match=r"code -1\).*one row"):
            call()
    assert eng.dropout_step() == 0 and len(eng.read_log()) == 0
    assert [b["num_batches_tracked"] for b in eng.get_bn() if b is not None] == [0]
    eng.train_step(Xd, row0=3, batch=8)          # the engine and the stream are usable
    eng.train_step(Xd, row0=9, batch=16)
    if kind == "ae":
        eng.eval_step(Xd, row0=3, batch=1)       # evaluation mode normalises with the running statistics: one row is fine
    rec = eng.read_log()
    assert len(rec) == (3 if kind == "ae" else 2) and np.isfinite(rec[:, 0]).all()
    assert eng.dropout_step() == 2
    assert [b["num_batches_tracked"] for b in eng.get_bn() if b is not None] == [2 if kind == "ae" else 4]
    torch.cuda.synchronize()
    eng.close()
    free = hip.Mlp(kind, dims, acts, max_batch=16, dropout=[0.1] + [0.0] * (len(dims) - 2), **extra)   # no normalisation: accepted
    push_params(free, lins)
    if kind == "ae":
        free.set_feature_range(np.ones(12, np.float32))
    free.reset_log(2)
    free.forward(Xd, train=True, **one)
    free.close()


# ============================================================================= E. sensitivity pass
def _random_bn_state(rng, width):
    """non-trivial running statistics: mean ~ N(0, 0.3), variance ~ U(0.5, 2), weight ~ U(0.5, 1.5)"""
    return {"weight": rng.uniform(0.5, 1.5, width).astype(np.float32), "bias": rng.uniform(-0.3, 0.3, width).astype(np.float32),
            "running_mean": (0.3 * rng.standard_normal(width)).astype(np.float32), "running_var": rng.uniform(0.5, 2.0, width).astype(np.float32),
            "num_batches_tracked": 3}


def _chain64(linears, acts, bn_state):
    """float64 evaluation-mode chain Linear [, activation][, BatchNorm1d] from (weight, bias) pairs and normalisation states"""
    mods = []
    for (w, b), act, st in zip(linears, acts, bn_state):
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(np.asarray(w)))
            lin.bias.copy_(torch.from_numpy(np.asarray(b)))
        mods.append(lin)
        if onn.ACTIVATIONS[act] is not None:
            mods.append(onn.ACTIVATIONS[act]())
        if st is not None:
            norm = torch.nn.BatchNorm1d(w.shape[0])
            with torch.no_grad():
                norm.weight.copy_(torch.from_numpy(st["weight"]))
                norm.bias.copy_(torch.from_numpy(st["bias"]))
                norm.running_mean.copy_(torch.from_numpy(st["running_mean"]))
                norm.running_var.copy_(torch.from_numpy(st["running_var"]))
            mods.append(norm)
    return torch.nn.Sequential(*mods).double().eval()


SENS_CASES = {
    # a normalisation behind the LAST layer (the seed gradient with DCV_ACT_NONE, then bn_eval_backward); 1000 rows in chunks of
    # the engine's row capacity (2 x max_batch = 768 rows for a Deep-TICA engine)
    "deep_tica-bn": ("deep_tica", [70, 33, 17, 3], ["tanh", "elu", None], [T, F, T], 1000, 384),
    "ae-bn": ("ae", [54, 16, 2, 16, 54], ["softplus", None, "tanh", None], [T, T, F, F], 500, 500),        # n_run = latent_layer = 2
    "vae-bn": ("vae", REF_DIMS, REF_ACTS, [T, F, F, F, F, F], 500, 500),                                     # g = [1 / range | 0]
    # the activations the pass had never run
    "relu": ("deep_tica", [70, 33, 17, 3], ["relu", "relu", None], [F, F, F], 1000, 384),
    "shifted_softplus": ("deep_tica", [70, 33, 17, 3], ["shifted_softplus", "shifted_softplus", None], [F, F, F], 1000, 384),
    "custom_sigmoid": ("deep_tica", [70, 33, 17, 3], ["custom_sigmoid", "custom_sigmoid", None], [F, F, F], 1000, 384),
}


@pytest.mark.parametrize("case", list(SENS_CASES))
def test_input_sensitivity_through_normalised_layers(case):
    """dcv_mlp_input_sensitivity against float64 autograd through the evaluation-mode oracle chain (running statistics set
    through set_linears(bn=...)), rtol 2e-4 as test_input_sensitivity_matches_autograd: bn_eval_bwd_kernel behind hidden
    layers and behind the last layer of the pass, for a Deep-TICA chain, an autoencoder's encoder and a variational
    autoencoder's encoder with its heads (g = [1 / range | 0], VAECalculator.summed_cv_gradient); and relu, shifted softplus
    and custom sigmoid without a normalisation.
    MEASURED on MI355X, worst relative deviation: deep_tica-bn 3.0e-7, ae-bn 4.8e-7, vae-bn 1.6e-7, relu 1.9e-7,
    shifted_softplus 3.4e-7, custom_sigmoid 2.7e-7."""
    from deep_cartograph_amd import hip

    kind, dims, acts, bnf, n, cap = SENS_CASES[case]
    rng = np.random.default_rng(5)
    Xn = rng.standard_normal((n, dims[0])).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, dims[0]).astype(np.float32)
    L = len(dims) - 1
    bn_state = [_random_bn_state(rng, dims[l + 1]) if bnf[l] else None for l in range(L)]
    torch.manual_seed(9)
    if kind == "vae":
        linears, n_run = vae_init(dims, 3, 9), 3
        g = np.concatenate([1.0 / rng.uniform(0.5, 2.0, 2), np.zeros(2)]).astype(np.float32)
        eng = hip.Mlp("vae", dims, acts, max_batch=cap, latent_layer=3, batchnorm=bnf)
    else:
        in_dims = dims[:-1]
        linears = [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in (torch.nn.Linear(in_dims[i], dims[i + 1]) for i in range(L))]
        n_run = L if kind == "deep_tica" else 2
        g = rng.standard_normal(dims[n_run]).astype(np.float32)
        if kind == "ae":
            eng = hip.Mlp("ae", dims, acts, max_batch=cap, latent_layer=2, batchnorm=bnf)
        else:
            eng = hip.Mlp("deep_tica", dims, acts, max_batch=cap, lag=0, tica_reg=1e-6, batchnorm=bnf)
    eng.set_linears(linears, bn=bn_state if any(bnf) else None)
    got = eng.input_sensitivity(torch.from_numpy(Xn).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(scale).cuda()).cpu().numpy()
    eng.close()
    chain = _chain64(linears[:n_run], acts[:n_run], bn_state[:n_run])
    x = torch.from_numpy(Xn).double().requires_grad_(True)
    out = (chain(x) * torch.from_numpy(g).double()).sum()
    grad = torch.autograd.grad(out, x)[0].numpy()
    exp = (np.abs(grad) * scale.astype(np.float64)).sum(axis=0)
    assert got.shape == exp.shape
    print(f"sensitivity {case}: worst relative deviation {np.max(np.abs(got - exp) / exp):.2e}")
    np.testing.assert_allclose(got, exp, rtol=2e-4)
