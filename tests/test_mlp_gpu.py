"""Parity of the HIP MLP engine (Deep-TICA / autoencoder steps, training, inference) against
the torch-CPU autograd oracle.  Run on the GPU box: python -m pytest tests -m gpu"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import linear as ol
from oracle import nn as onn

pytestmark = pytest.mark.gpu


def ar_features(n, F, seed, k_slow=3):
    """SURVEY.md section 8d generator (small): AR(1) slow modes mixed into F features."""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = np.array([2000, 700, 250, 90][:k_slow], dtype=np.float64)
    rho = np.exp(-1.0 / T)
    z = np.zeros((n, k_slow))
    eta = rng.standard_normal((n, k_slow))
    for t in range(1, n):
        z[t] = rho * z[t - 1] + np.sqrt(1 - rho ** 2) * eta[t]
    A = rng.standard_normal((F, k_slow)) / np.sqrt(k_slow)
    X = z @ A.T + 0.5 * rng.standard_normal((n, F))
    X = X * rng.uniform(0.1, 10, F) + rng.uniform(-5, 5, F)
    return X.astype(np.float32)


def normalized(X):
    st = ol.feature_stats(X)
    m, r = ol.prepare_normalization(st, "mean_std")
    return ol.normalize(X, m, r), m.astype(np.float32), r.astype(np.float32)


def linears_of(seq):
    return [m for m in seq if isinstance(m, torch.nn.Linear)]


def push_params(eng, lins):
    eng.set_linears([(l.weight.detach().numpy(), l.bias.detach().numpy()) for l in lins])


def rel_err(a, b):
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


@pytest.mark.parametrize("mode", ["split", "native"])
@pytest.mark.parametrize("dims,n,lag,batch,gather", [
    ([54, 16, 8, 2], 164, 1, 131, True),
    ([54, 16, 8, 2], 164, 1, 100, False),
    ([256, 128, 64, 4], 6000, 10, 2048, True),
    ([64, 32, 3], 3000, 5, 777, False),
    ([40, 5], 1000, 2, 500, True),
    # the contract batch: 8192 pairs + lag = 8202 shared rows, one ragged row tile past a multiple of the
    # CU count -- the products take the contraction-split tail tile (gemm.h: GemmDims::tail_split).  tanh layers: with a
    # million leaky-ReLU units per batch a few pre-activations sit within float32 rounding of the kink, and one flipped
    # slope (1 vs 0.01) moves a gradient entry by 1e-4 of the largest one -- in the float32 oracle just as in either
    # arithmetic flavour of the engine (measured: FP32-input MFMA 3.8e-4, split 3e-7 on this very batch)
    ([512, 256, 128, 3, "tanh"], 8300, 10, 8192, False),
    # 4096 pairs + lag = 4106 shared rows: the row-limited weight-gradient plan (mlp.hip: wgrad_plan) takes 16 contraction
    # chunks of 257 rows -- chunk ends that are no stage multiple (the stage tail goes through registers), 64 x 64 tiles
    ([512, 256, 128, 3, "tanh"], 4200, 10, 4096, False),
    # the reference's DEFAULT loader at the contract batch (random split + shuffle: bench.py's `shuffled` block): 8192
    # gathered pairs = 2 x 8192 rows through the int64 index, the grouped weight / input gradient launch of mixed tile
    # families (pair.hip), 64 split-K slabs for layer 0
    ([512, 256, 128, 3, "tanh"], 8400, 10, 8192, True),
])
def test_deeptica_step_matches_autograd(features, dims, n, lag, batch, gather, mode):
    """One Deep-TICA step (statistics, loss, every gradient) against a FLOAT64 run of the autograd oracle on the same
    float32 parameters and inputs, in both arithmetic flavours of the matrix products.  Tolerance 2e-5 of the
    largest gradient entry per tensor (the engine computes in float32; the float32 oracle itself sits 1e-6 .. 3e-3
    from the float64 one on these cases -- its d x d Cholesky / eigh run in float32)."""
    import copy

    from deep_cartograph_amd import hip

    hidden_act = "leaky_relu"
    if isinstance(dims[-1], str):
        dims, hidden_act = dims[:-1], dims[-1]
    X = features[0] if dims[0] == 54 else ar_features(n, dims[0], 11)
    Xn, _, _ = normalized(X)
    P = Xn.shape[0] - lag
    acts = [hidden_act] * (len(dims) - 2) + [None]
    torch.manual_seed(3)
    ref = onn.DeepTICAModel(dims, acts, None, None, None, 1e-6)
    ref64 = copy.deepcopy(ref).double()
    prev = hip.get_gemm_mode()
    hip.set_gemm_mode(mode)
    try:
        eng = hip.Mlp("deep_tica", dims, acts, max_batch=batch, lag=lag, tica_reg=1e-6)
        lins = linears_of(ref64.nn)
        push_params(eng, linears_of(ref.nn))
        Xd = torch.from_numpy(Xn).cuda()
        if gather:
            idx = torch.randperm(P)[:batch].contiguous()
            kw = dict(idx=idx.cuda())
        else:
            idx = torch.arange(7, 7 + batch)
            kw = dict(row0=7, batch=batch)
        eng.reset_log(2)
        eng.forward(Xd, **kw)
        stats = eng.stats_view().cpu().numpy()
        eng.backward(Xd, **kw)
        g = eng.grads_view().cpu().numpy()
        rec = eng.read_log()[0]
        eng.close()
    finally:
        hip.set_gemm_mode(prev)
    xt = torch.from_numpy(Xn).double()
    loss, _ = ref64.step(xt[idx], xt[idx + lag])
    loss.backward()
    with torch.no_grad():
        f_t = ref64.forward_nn(xt[idx])
        f_l = ref64.forward_nn(xt[idx + lag])
    d = dims[-1]
    np.testing.assert_allclose(stats[:d], f_t.sum(0).numpy(), rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(stats[2 * d:2 * d + d * d].reshape(d, d), (f_t.T @ f_t).numpy(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(stats[2 * d + d * d:].reshape(d, d), (f_t.T @ f_l).numpy(), rtol=2e-5, atol=2e-5)
    assert abs(rec[0] - float(loss)) < 1e-5 * max(1.0, abs(float(loss)))
    assert rec[1] == batch
    worst = 0.0
    for l, lin in enumerate(lins):
        wo, bo = eng.offsets[l]
        gw = lin.weight.grad.numpy()
        gb = lin.bias.grad.numpy()
        ew = rel_err(g[wo:wo + gw.size].reshape(gw.shape), gw)
        worst = max(worst, ew)
        assert ew < 2e-5, f"layer {l} weight: {ew:.2e}"
        if l < len(lins) - 1:
            eb = rel_err(g[bo:bo + gb.size], gb)
            worst = max(worst, eb)
            assert eb < 2e-5, f"layer {l} bias: {eb:.2e}"
        else:
            # the loss is invariant to a constant shift of the outputs (TICA removes the mean), so
            # the exact gradient of the last bias is 0: the engine holds float32 rounding noise only
            assert np.max(np.abs(g[bo:bo + gb.size])) < 2e-5 * max(1.0, np.max(np.abs(gw))), f"layer {l} bias"
    print(f"{mode} {dims} batch {batch}: worst gradient deviation from float64 = {worst:.2e} of the largest entry")


def ar_features_fast(n, F, seed, k_slow=3):
    """ar_features' process (same generator, same draws) with the AR(1) recurrence in blocks of 256 rows instead of a Python
    loop over every row: inside a block z[i] = rho^(i+1) z[-1] + rho^i cumsum(c eta[j] rho^-j)[i], exact up to float64
    rounding (rho^-256 <= 18 for the shortest time scale)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = np.array([2000, 700, 250, 90][:k_slow], dtype=np.float64)
    rho = np.exp(-1.0 / T)
    eta = rng.standard_normal((n, k_slow)) * np.sqrt(1 - rho ** 2)
    eta[0] = 0.0
    z = np.empty((n, k_slow))
    prev = np.zeros(k_slow)
    blk = 256
    up, down = rho ** np.arange(blk)[:, None], rho ** -np.arange(blk)[:, None]
    for b0 in range(0, n, blk):
        m = min(blk, n - b0)
        z[b0:b0 + m] = up[:m] * (rho * prev + np.cumsum(eta[b0:b0 + m] * down[:m], axis=0))
        prev = z[b0 + m - 1]
    A = rng.standard_normal((F, k_slow)) / np.sqrt(k_slow)
    X = z @ A.T + 0.5 * rng.standard_normal((n, F))
    X = X * rng.uniform(0.1, 10, F) + rng.uniform(-5, 5, F)
    return X.astype(np.float32)


def step_oracle(x, Ws, bs, hidden_act, patterns, n_t, lag_off, dtype=torch.float64):
    """One Deep-TICA step on the rows x (the engine's logical order: f_t = f[:n_t], f_lag = f[lag_off:lag_off + n_t]) with
    plain torch in `dtype`.  leaky_relu: patterns[l] is a boolean slope pattern of hidden layer l to hold fixed (the network
    is then piecewise linear), or None for the layer's own.  Returns the pre-activations' slope decisions, sum f_t, f_t^T f_t,
    f_t^T f_lag, the loss and the weight / bias gradients as float64 NumPy arrays."""
    W = [w.to(dtype).clone().requires_grad_(True) for w in Ws]
    b = [v.to(dtype).clone().requires_grad_(True) for v in bs]
    h, own, zs = x.to(dtype), [], []
    for l in range(len(W) - 1):
        z = h @ W[l].T + b[l]
        if hidden_act == "leaky_relu":
            own.append(z.detach() > 0)
            zs.append(z.detach())
            m = own[-1] if patterns is None or patterns[l] is None else patterns[l]
            h = z * torch.where(m, 1.0, 0.01).to(dtype)
        else:
            assert hidden_act == "tanh"
            h = torch.tanh(z)
    f = h @ W[-1].T + b[-1]
    f_t, f_l = f[:n_t], f[lag_off:lag_off + n_t]
    evals, _, _ = onn.batch_tica(f_t, f_l, 1e-6)
    loss = onn.deeptica_loss(evals)
    loss.backward()
    np64 = lambda t: t.detach().double().numpy()
    return dict(own=own, z=zs, sum_t=np64(f_t.sum(0)), c00=np64(f_t.T @ f_t), c0t=np64(f_t.T @ f_l), loss=float(loss.detach()),
                gw=[np64(w.grad) for w in W], gb=[np64(v.grad) for v in b])


def check_step_against_float64(mode, dims, batch, lag, row0, gather, row_sharing, *, Xn, weight_seed, hidden_act="leaky_relu",
                               train_step=False, label=""):
    """One step of the block engine on `batch` pairs of Xn against float64, kink-aware for leaky-ReLU networks: (i) the
    engine's slope decisions (sign of its stored activations) may differ from the float64 ones only where the float64
    pre-activation is within 1e-5 of zero; (ii) given the engine's slope pattern -- the network is then piecewise linear with
    that pattern fixed -- every gradient tensor, the statistics and the loss must agree with the float64 evaluation to the
    tolerances of test_deeptica_step_matches_autograd.  train_step: the same batch once more as a one-GPU training step (update
    fused in), whose gradients are held to the same criterion.  Returns the product plans the engine launched
    (hip.gemm_log()) for the forward + backward and for the training step."""
    from deep_cartograph_amd import hip

    L = len(dims) - 1
    acts = [hidden_act] * (L - 1) + [None]
    torch.manual_seed(weight_seed)
    ref = onn.DeepTICAModel(dims, acts, None, None, None, 1e-6)
    if gather:
        idx = torch.from_numpy(np.random.Generator(np.random.PCG64(weight_seed)).permutation(Xn.shape[0] - lag)[:batch].astype(np.int64))
        kw = dict(idx=idx.cuda())
    else:
        idx = torch.arange(row0, row0 + batch)
        kw = dict(row0=row0, batch=batch)
    shared = not gather and row_sharing
    rows = torch.arange(row0, row0 + batch + lag) if shared else torch.cat([idx, idx + lag])
    R, lag_off = int(rows.numel()), (lag if shared else batch)
    prev = hip.get_gemm_mode()
    hip.set_gemm_mode(mode)
    logs, g_step = {}, None
    try:
        eng = hip.Mlp("deep_tica", dims, acts, max_batch=batch, lag=lag, tica_reg=1e-6)
        push_params(eng, linears_of(ref.nn))
        eng.set_row_sharing(row_sharing)
        Xd = torch.from_numpy(Xn).cuda()
        eng.reset_log(4)
        hip.gemm_log_reset()
        eng.forward(Xd, **kw)
        stats = eng.stats_view().cpu().numpy()
        H = [eng.layer_output(l, R).cpu().numpy() for l in range(L - 1)] if hidden_act == "leaky_relu" else []
        eng.backward(Xd, **kw)
        g = eng.grads_view().cpu().numpy()
        rec = eng.read_log()[0]
        assert eng.last_path() == 0, eng.last_path()
        logs["step"] = hip.gemm_log()
        if train_step:
            hip.gemm_log_reset()
            eng.train_step(Xd, **kw)
            g_step = eng.grads_view().cpu().numpy()
            rec_step = eng.read_log()[1]
            assert eng.last_path() == 0, eng.last_path()
            logs["train_step"] = hip.gemm_log()
            logs["ride"] = eng.last_ride()
        offsets = list(eng.offsets)
        eng.close()
    finally:
        hip.set_gemm_mode(prev)
    print(f"{label} {mode}: product plans {[tuple(e) for e in logs['step']]}" + (f"; training step {[tuple(e) for e in logs['train_step']]}" if train_step else ""))
    Ws = [l.weight.detach() for l in linears_of(ref.nn)]
    bs = [l.bias.detach() for l in linears_of(ref.nn)]
    x = torch.from_numpy(Xn)[rows]
    patterns = [torch.from_numpy(h > 0) for h in H] if hidden_act == "leaky_relu" else None
    o = step_oracle(x, Ws, bs, hidden_act, patterns, batch, lag_off)
    flips = []
    for l in range(len(H)):
        differ = patterns[l] != o["own"][l]
        flips.append(int(differ.sum()))
        if differ.any():   # (i): only units within float32 rounding of the kink
            assert float(o["z"][l].abs()[differ].max()) < 1e-5, f"layer {l}: slope decision differs away from the kink"
    d = dims[-1]
    np.testing.assert_allclose(stats[:d], o["sum_t"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(stats[2 * d:2 * d + d * d].reshape(d, d), o["c00"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(stats[2 * d + d * d:].reshape(d, d), o["c0t"], rtol=2e-5, atol=2e-5)
    loss = o["loss"]
    print(f"{label} {mode}: loss deviation {abs(rec[0] - loss) / max(1.0, abs(loss)):.2e}")
    assert abs(rec[0] - loss) < 1e-5 * max(1.0, abs(loss))
    if train_step:
        assert abs(rec_step[0] - loss) < 1e-5 * max(1.0, abs(loss))
    for what, gv in (("", g), (" (training step)", g_step)):
        if gv is None:
            continue
        dev = {}
        for l in range(L):
            wo, bo = offsets[l]
            gw, gb = o["gw"][l], o["gb"][l]
            dev[f"layer {l} weight"] = rel_err(gv[wo:wo + gw.size].reshape(gw.shape), gw)
            if l < L - 1:
                dev[f"layer {l} bias"] = rel_err(gv[bo:bo + gb.size], gb)
        last_bias = float(np.max(np.abs(gv[offsets[L - 1][1]:offsets[L - 1][1] + dims[-1]])))
        print(f"{label} {mode}{what}: slope decisions differing from float64 (all within 1e-5 of the kink): {flips}; gradient deviations "
              f"from float64 given the slope pattern, of the largest entry: { {k: '%.2e' % v for k, v in dev.items()} }; last bias {last_bias:.2e}")
        for k, v in dev.items():
            assert v < 2e-5, f"{k}{what}: {v:.2e}"
        # the loss is invariant to a constant shift of the outputs (TICA removes the mean), so the exact gradient of the last
        # bias is 0: the engine holds float32 rounding noise only
        assert last_bias < 2e-5 * max(1.0, np.max(np.abs(o["gw"][L - 1]))), "last bias" + what
    return logs


@pytest.mark.parametrize("mode", ["split", "native"])
def test_contract_batch_leaky_relu_step_kink_aware(mode):
    """The bench's own configuration -- 512-256-128-4, leaky-ReLU, 8192 contiguous pairs + lag 10 -- against float64.
    Among the three million hidden units of such a batch a few pre-activations sit within float32 rounding of the kink,
    and one flipped slope (1 vs 0.01) moves a gradient entry by 1e-4 of the largest one in ANY float32 implementation.
    Kink-aware criterion: see check_step_against_float64."""
    Xn, _, _ = normalized(ar_features(8300, 512, 31))
    check_step_against_float64(mode, [512, 256, 128, 4], 8192, 10, 7, False, True, Xn=Xn, weight_seed=6, label="contract batch, leaky-ReLU")


@functools.lru_cache(maxsize=None)
def big_features(n, F):
    """Normalised AR(1) features of the 128-row-tile cases, generated once per shape and shared (never written to)."""
    return normalized(ar_features_fast(n, F, 41))[0]


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# Whole-step float64 oracle where the row-parallel products take 128 x 128 tiles: from 128 * 2 * CUs / column tiles rows up,
# i.e. more rows than any other oracle test gathers.  Shapes follow the CU count; on 256 CUs: 32 878 shared rows = 257 row
# tiles (cases a, b, d), 65 510 rows = 512 row tiles of a one-column-tile layer (c), 2 x 16 500 gathered rows (e), two halves
# of 16 450 rows (f); and 16 310 rows (g: the ride launch, see there).  name -> (dims, hidden activation, batch, gather, row sharing, training step too)
def _big_case(name):
    n = _ncu()
    return {
        # layer 0 NT 128 x 128 with the contraction-split tail tile (257 x 2 workgroups, K = 512), sign-mask store and its
        # read-back by the 128 x 128 NN input gradient (side-operand prefetch); layer 1 at 64 x 128 with the fused head;
        # layer-0 weight gradient TN 128 x 128 on its own.  NOT here: the 128 x 128 / 128 x 128 pair (layer 1's 128 x 256 weight
        # gradient takes 64 x 64 tiles at this row count, so its two products launch apart: cases b, e have the pair) and the
        # ride launch (case g)
        "a": ([512, 256, 128, 4], "leaky_relu", 128 * n + 100, False, True, False),
        # both hidden forward products 128 x 128 with the tail cut at K = 256; unfused narrow head; NN 128 x 128 with K = 3
        # (scalar loaders, gather-capable kernel form); weight + input gradient of layer 1 as one 128 x 128 / 128 x 128 launch
        "b": ([256, 256, 160, 3], "tanh", 128 * n + 100, False, True, False),
        # the fused head on a 128 x 128 tile (one column tile: 2 * CUs row tiles of 128 rows), head backward
        "c": ([64, 128, 4], "leaky_relu", 256 * n - 36, False, True, False),
        # layer 1: input gradient 128 wide (64 x 128 tiles), weight gradient 512 x 128 in 128 x 128 tiles: one launch of
        # mixed families (a 256-wide layer's weight gradient takes 64 x 64 tiles at this row count: 2 tiles x 64 chunks)
        "d": ([96, 128, 512, 3], "leaky_relu", 128 * n + 100, False, True, False),
        # case b through a random int64 index: the gathering loaders at 128 x 128 (NT layer 0, TN layer-0 weight gradient)
        # gathered rows are not wrapped by the weight gradient + reduction launch: as a training step too, which must end on
        # the single reduction (no ride) with the layer-0 weight gradient launched alone
        "e": ([256, 256, 160, 3], "tanh", 64 * n + 116, True, True, True),
        # case a as two halves: the x_t / x_lag seam inside a 128-row tile and inside a weight-gradient chunk
        "f": ([512, 256, 128, 4], "leaky_relu", 64 * n + 66, False, False, False),
        # The layer-0 weight gradient + reduction launch at 128 x 128 (test_step_chain_gpu.py's big_tiles shape).  It needs the
        # flat-grid reduction -- at most 512 partials per weight -- and the head's backward leaves one partial per 32 rows, so it
        # ends at 16 384 rows, while the 256 x 512 weight gradient takes 128 x 128 tiles from 64 * CUs - 255 rows: a window below
        # every case above, where the forward products take 64 x 64 tiles.  64 * CUs - 74 rows.  So the 128 x 128 ride launch
        # is only ever checked next to 64 x 64 forwards, and no whole step above 32 768 pairs rides: none can.
        "g": ([512, 256, 128, 4], "leaky_relu", 64 * n - 84, False, True, True),
    }[name]


def _has(log, **want):
    """an entry of hip.gemm_log() with these fields; a callable value is a predicate on the field"""
    hit = lambda e: all(v(getattr(e, k)) if callable(v) else getattr(e, k) == v for k, v in want.items())
    return any(hit(e) for e in log)


@pytest.mark.parametrize("mode", ["split", "native"])
@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e", "f", "g"])
def test_step_at_128_row_tiles_kink_aware(case, mode):
    """check_step_against_float64 at the batch sizes where the block engine takes its 128 x 128 tile family, with the launched
    plans asserted from hip.gemm_log() (see _big_case for what each case reaches).  Tolerances: those of the contract-batch test;
    the float32 torch-CPU oracle's own deviation from float64 on these cases (slope pattern fixed) is at most 1.5e-6 per gradient
    tensor, 4.8e-7 on the loss and 4.0e-6 on the statistics, so 2e-5 / 1e-5 stand.
    MEASURED on MI355X (256 CUs), both flavours, cases a, c, d, f, g: worst gradient deviation 7.5e-7 of the largest entry
    (case f, layer-0 weights), loss 3.2e-8, at most 2 slope decisions differing from float64, all within 1e-5 of the kink.
    Cases b and e (tanh): gradients 3.7e-7, loss 1.4e-8 (native).  Their split cases failed on sum f_t (1.9e-4 and 1.4e-3
    relative) until the defect described in test_forward_at_128_row_tiles_other_activations was fixed."""
    dims, act, batch, gather, sharing, train_step = _big_case(case)
    lag, row0 = 10, 7
    n = 2 * batch if gather else batch + lag + row0 + 5
    logs = check_step_against_float64(mode, dims, batch, lag, row0, gather, sharing, Xn=big_features(n, dims[0]), weight_seed=6,
                                      hidden_act=act, train_step=train_step, label=f"128-row tiles, case {case}")
    log = logs["step"]
    assert all(e.split == (mode == "split") for e in log), log
    big = dict(tm=128, tn=128)
    cut = lambda t: t >= 2
    if case == "a":
        assert _has(log, form="single", mode="nt", vec=True, gather=False, tail_split=cut, **big), log
        assert _has(log, form="single", mode="nt", tm=64, tn=128), log
        assert _has(log, mode="nn", vec=True, **big), log
        assert _has(log, form="single", mode="tn", splits=cut, **big), log
    elif case == "b":
        assert sum(1 for e in log if e.mode == "nt" and (e.tm, e.tn) == (128, 128) and e.tail_split >= 2 and e.vec) == 2, log
        assert _has(log, mode="nt", tn=32), log
        assert _has(log, form="single", mode="nn", vec=False, gather=True, **big), log
        assert _has(log, form="pair", mode="tn", splits=cut, **big) and _has(log, form="pair", mode="nn", **big), log
        assert _has(log, form="single", mode="tn", splits=cut, **big), log
    elif case == "c":
        assert log[0].mode == "nt" and (log[0].tm, log[0].tn) == (128, 128) and log[0].vec, log
        assert sum(1 for e in log if e.mode == "nt") == 1, log   # the head rode in layer 0's epilogue
        assert _has(log, form="single", mode="tn", splits=cut, **big), log
    elif case == "d":
        assert _has(log, form="single", mode="nt", tm=64, tn=128), log
        assert _has(log, form="single", mode="nt", **big), log
        assert _has(log, form="pair", mode="tn", splits=cut, **big) and _has(log, form="pair", mode="nn", tm=64, tn=128), log
    elif case == "e":
        assert _has(log, form="single", mode="nt", vec=True, gather=True, **big), log
        assert _has(log, form="single", mode="tn", vec=True, gather=True, splits=cut, **big), log
        assert _has(log, form="pair", mode="tn", **big) and _has(log, form="pair", mode="nn", **big), log
        step = logs["train_step"]
        assert all(e.split == (mode == "split") for e in step), step
        assert logs["ride"] == 0 and not _has(step, form="ride"), (logs["ride"], step)
        assert _has(step, form="single", mode="tn", vec=True, gather=True, splits=cut, **big), step
    elif case == "f":
        assert _has(log, form="single", mode="nt", vec=True, gather=False, **big), log
        assert _has(log, mode="nn", vec=True, **big), log
        assert _has(log, form="single", mode="tn", splits=cut, **big), log
    else:
        ride = logs["train_step"]
        assert all(e.split == (mode == "split") for e in ride), ride
        assert logs["ride"] > 0 and _has(ride, form="ride", mode="tn", splits=cut, **big), (logs["ride"], ride)


def forward_layers_against_float64(case, act, mode):
    """One forward of the case's network with `act` on its hidden layers; the launch log and, per layer, the engine's output,
    its float64 value computed from the engine's own input to that layer, and the element-wise bound: the fp32 product bound of
    test_gemm_random_fp32 on the pre-activation (tanh and elu have slope <= 1) plus 4 ulp of the result for the library
    function."""
    from deep_cartograph_amd import hip

    dims, _, batch, _, _, _ = _big_case(case)
    L = len(dims) - 1
    lag, row0 = 10, 7
    R = batch + lag
    Xn = big_features(batch + lag + row0 + 5, dims[0])
    torch.manual_seed(6)
    lins = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(L)]
    prev = hip.get_gemm_mode()
    hip.set_gemm_mode(mode)
    try:
        eng = hip.Mlp("deep_tica", dims, [act] * (L - 1) + [None], max_batch=batch, lag=lag, tica_reg=1e-6)
        push_params(eng, lins)
        eng.reset_log(2)
        hip.gemm_log_reset()
        eng.forward(torch.from_numpy(Xn).cuda(), row0=row0, batch=batch)
        log = hip.gemm_log()
        H = [eng.layer_output(l, R).cpu().numpy()[:, :dims[l + 1]] for l in range(L)]
        assert eng.last_path() == 0
        eng.close()
    finally:
        hip.set_gemm_mode(prev)
    out, x = [], Xn[row0:row0 + R].astype(np.float64)
    for l in range(L):
        W, b = lins[l].weight.detach().double().numpy(), lins[l].bias.detach().double().numpy()
        z = x @ W.T + b
        ref = z if l == L - 1 else (np.tanh(z) if act == "tanh" else np.where(z > 0, z, np.expm1(np.minimum(z, 0))))
        bound = 4e-7 * (np.abs(x) @ np.abs(W).T + np.abs(b)) + 1e-6 + 4 * 2.0 ** -24 * np.abs(ref)
        out.append((H[l], ref, bound))
        x = H[l].astype(np.float64)
    return log, out


def assert_within(name, got, ref, bound):
    err = np.abs(got - ref)
    print(f"{name}: worst error / bound {np.max(err / bound):.3g}, elements beyond the bound {int((err > bound).sum())}")
    assert np.all(err <= bound), f"{name}: {int((err > bound).sum())} elements beyond the bound, worst {err.max():.3e}"


@pytest.mark.parametrize("mode", ["split", "native"])
@pytest.mark.parametrize("act", ["tanh", "elu"])
def test_forward_at_128_row_tiles_other_activations(act, mode):
    """Layer 0 of case b alone (256 -> 256 on 128 * CUs + 110 rows: NT, 128 x 128 tiles, EpiBiasAct) with an activation outside
    the ReLU family, element by element against float64 (bound: forward_layers_against_float64).
    This test found a defect whose cause is unknown: while the epilogues applied act(x + bias) in one pass (gemm_kernels.h:
    bias_then_act has the two-pass form they use now), the split flavour lost 16 .. 192 elements per forward here (six forwards
    each with tanh, elu, softplus; also with plain stores, DCV_WT=0): always 16 at a time -- one row, every fourth column of
    the upper half of a column tile, i.e. the third float of the first row segment an epilogue thread handles, in lanes 48..63
    of its wave -- other elements each launch, their value exactly act(bias): the product term was lost.  The native flavour
    and leaky-ReLU / ReLU / linear layers were never affected.
    MEASURED on MI355X (256 CUs) since: 0 elements beyond the bound in 30 split forwards; worst error 0.29 of the bound (native)."""
    log, layers = forward_layers_against_float64("b", act, mode)
    assert (log[0].mode, log[0].tm, log[0].tn, log[0].split, log[0].vec) == ("nt", 128, 128, mode == "split", True), log
    assert_within(f"{act} {mode} layer 0", *layers[0])


@pytest.mark.parametrize("mode", ["split", "native"])
@pytest.mark.parametrize("act", ["tanh", "elu"])
def test_fused_head_forward_at_128_row_tiles_other_activations(act, mode):
    """The same for the fused head on a 128 x 128 tile (case c's 64 -> 128 -> 4 on 256 * CUs - 26 rows: EpiBiasActHead<4>, one
    NT launch for both layers): the hidden activations H it stores, and the head's outputs given those H.
    MEASURED on MI355X (256 CUs): 0 elements beyond either bound in 4 forwards per activation and flavour, with the one-pass
    form of the epilogue as with bias_then_act: the loss seen in EpiBiasAct never showed here.  As its cause is unknown, that
    is no proof of absence; the epilogue shares bias_then_act and this test watches it."""
    log, layers = forward_layers_against_float64("c", act, mode)
    assert (log[0].mode, log[0].tm, log[0].tn, log[0].split, log[0].vec) == ("nt", 128, 128, mode == "split", True), log
    assert sum(1 for e in log if e.mode == "nt") == 1, log   # the head rode in layer 0's epilogue
    assert_within(f"{act} {mode} hidden layer", *layers[0])
    assert_within(f"{act} {mode} head", *layers[1])


def test_contract_batch_step_is_reproducible():
    """The contraction-split tail tile (8202 rows: 512 regular + 32 tail-chunk workgroups per product) adds its chunks up in
    chunk order whatever the arrival order: statistics, loss and every gradient of repeated steps on the same weights are
    bit-identical, in two engines and across repetitions."""
    from deep_cartograph_amd import hip

    dims, lag, batch = [512, 256, 128, 3], 10, 8192
    acts = ["leaky_relu", "leaky_relu", None]
    Xn, _, _ = normalized(ar_features(8300, dims[0], 21))
    torch.manual_seed(4)
    ref = onn.DeepTICAModel(dims, acts, None, None, None, 1e-6)
    Xd = torch.from_numpy(Xn).cuda()
    seen = []
    for _ in range(2):
        eng = hip.Mlp("deep_tica", dims, acts, max_batch=batch, lag=lag, tica_reg=1e-6)
        push_params(eng, linears_of(ref.nn))
        eng.reset_log(8)
        for _rep in range(3):
            eng.forward(Xd, row0=5, batch=batch)
            stats = eng.stats_view().cpu().numpy().copy()
            eng.backward(Xd, row0=5, batch=batch)
            seen.append((stats, eng.grads_view().cpu().numpy().copy()))
        log = eng.read_log()
        assert np.all(log[:, 0] == log[0, 0])
        eng.close()
    for st, g in seen[1:]:
        np.testing.assert_array_equal(st, seen[0][0])
        np.testing.assert_array_equal(g, seen[0][1])


def test_deeptica_row_sharing_equivalence():
    """Contiguous batches evaluate the network once on the batch + lag rows both halves share; the
    result must equal the two-halves evaluation (same rows through the same weights)."""
    from deep_cartograph_amd import hip

    n, F, lag, batch = 5000, 96, 7, 1500
    dims, acts = [F, 48, 24, 3], ["leaky_relu", "tanh", None]
    Xn, _, _ = normalized(ar_features(n, F, 9))
    torch.manual_seed(5)
    ref = onn.DeepTICAModel(dims, acts, None, None, None, 1e-6)
    Xd = torch.from_numpy(Xn).cuda()
    out = {}
    for share in (True, False):
        eng = hip.Mlp("deep_tica", dims, acts, max_batch=batch, lag=lag, tica_reg=1e-6)
        push_params(eng, linears_of(ref.nn))
        eng.set_row_sharing(share)
        eng.reset_log(2)
        eng.forward(Xd, row0=11, batch=batch)
        stats = eng.stats_view().cpu().numpy().copy()
        eng.backward(Xd, row0=11, batch=batch)
        out[share] = (stats, eng.read_log()[0].copy(), eng.grads_view().cpu().numpy().copy())
        eng.close()
    np.testing.assert_allclose(out[True][0], out[False][0], rtol=1e-12)   # identical outputs -> identical float64 sums
    np.testing.assert_allclose(out[True][1], out[False][1], rtol=1e-10)
    g1, g0 = out[True][2], out[False][2]
    assert np.max(np.abs(g1 - g0)) < 2e-6 * np.max(np.abs(g0))           # same gradient, different fp32 summation order
    # and a gathered batch with the same samples agrees too
    eng = hip.Mlp("deep_tica", dims, acts, max_batch=batch, lag=lag, tica_reg=1e-6)
    push_params(eng, linears_of(ref.nn))
    eng.reset_log(2)
    idx = torch.arange(11, 11 + batch).cuda()
    eng.forward(Xd, idx=idx)
    eng.backward(Xd, idx=idx)
    np.testing.assert_allclose(eng.read_log()[0], out[True][1], rtol=1e-10)
    eng.close()


# measured after 30 Adam steps: loss 4.6e-6 (relative), weights 1.3e-7, hidden biases 7.6e-8.  The other side is the FLOAT32 oracle,
# whose own rounding depends on the host BLAS of the box it runs on: ~7 x the measured deviations rather than 3 x
DT_TRAIN_TOL = {"loss": 3e-5, "w": 1e-6, "b": 6e-7}


def test_deeptica_training_matches_oracle():
    from deep_cartograph_amd import hip

    n, F, lag, bs = 3000, 32, 5, 256
    dims, acts = [F, 16, 8, 2], ["leaky_relu", "leaky_relu", None]
    Xn, _, _ = normalized(ar_features(n, F, 5))
    P = n - lag
    gen = torch.manual_seed(44)
    ref = onn.DeepTICAModel(dims, acts, None, None, None, 1e-6)
    tr, va = onn.split_indices(P, [0.8, 0.2], True, gen)
    eng = hip.Mlp("deep_tica", dims, acts, max_batch=bs, lag=lag, tica_reg=1e-6, lr=1e-3)
    lins = linears_of(ref.nn)
    push_params(eng, lins)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    xt = torch.from_numpy(Xn)
    Xd = xt.cuda()
    ref_losses = []
    eng.reset_log(256)
    for epoch in range(3):
        for b in onn.batches(tr, bs, False):
            opt.zero_grad()
            loss, _ = ref.step(xt[b], xt[b + lag])
            loss.backward()
            opt.step()
            ref_losses.append(float(loss))
            eng.train_step(Xd, idx=b.cuda())
    log = eng.read_log()
    assert log.shape[0] == len(ref_losses)
    dev_loss = float(np.max(np.abs(log[:, 0] - np.asarray(ref_losses)) / np.maximum(np.abs(ref_losses), 0.1)))
    dev_w = max(float(np.max(np.abs(w - lin.weight.detach().numpy()))) for (w, _), lin in zip(eng.get_linears(), lins))
    dev_b = max(float(np.max(np.abs(b - lin.bias.detach().numpy()))) for (_, b), lin in zip(eng.get_linears()[:-1], lins[:-1]))
    print(f"deep-tica training vs float32 oracle after {len(ref_losses)} steps: loss {dev_loss:.2e} (relative), weights {dev_w:.2e}, hidden biases {dev_b:.2e}")
    np.testing.assert_allclose(log[:, 0], ref_losses, rtol=DT_TRAIN_TOL["loss"], atol=DT_TRAIN_TOL["loss"] * 0.1)
    for l, ((w, b), lin) in enumerate(zip(eng.get_linears(), lins)):
        np.testing.assert_allclose(w, lin.weight.detach().numpy(), atol=DT_TRAIN_TOL["w"])
        if l < len(lins) - 1:  # last bias: zero exact gradient, Adam amplifies rounding noise on both sides
            np.testing.assert_allclose(b, lin.bias.detach().numpy(), atol=DT_TRAIN_TOL["b"])
    # validation pass: eval steps log the loss and leave the parameters alone
    before = eng.get_linears()
    eng.reset_log(8)
    for b in onn.batches(va, bs, False):
        eng.eval_step(Xd, idx=b.cuda())
    vlog = eng.read_log()
    ref.eval()
    with torch.no_grad():
        vref = [float(ref.step(xt[b], xt[b + lag])[0]) for b in onn.batches(va, bs, False)]
    np.testing.assert_allclose(vlog[:, 0], vref, rtol=2e-3, atol=2e-4)
    for (w0, b0), (w1, b1) in zip(before, eng.get_linears()):
        np.testing.assert_array_equal(w0, w1)
    # logged C0 / Ctau reproduce the oracle's batch TICA eigenvalues
    d = 2
    rec = vlog[-1]
    C0 = torch.tensor(rec[2:2 + d * d].reshape(d, d))
    Ct = torch.tensor(rec[2 + d * d:2 + 2 * d * d].reshape(d, d))
    ev, _ = ol.cholesky_eigh(Ct, C0, 1e-6)
    with torch.no_grad():
        b = onn.batches(va, bs, False)[-1]
        ev_ref, _, _ = onn.batch_tica(ref.forward_nn(xt[b]), ref.forward_nn(xt[b + lag]), 1e-6)
    np.testing.assert_allclose(ev.numpy(), ev_ref.numpy(), atol=5e-4)
    eng.close()


def test_ae_training_matches_oracle(features):
    from deep_cartograph_amd import hip

    X = features[0]
    Xn, m, r = normalized(X)
    F = 54
    gen = torch.manual_seed(45)
    ref = onn.AEModel([F, 16, 8, 2], ["leaky_relu", "leaky_relu", None], None, [2, 4, 8, F], ["leaky_relu", "leaky_relu", None], None, m, r)
    tr, va = onn.split_indices(164, [0.8, 0.2], True, gen)
    dims = [F, 16, 8, 2, 4, 8, F]
    acts = ["leaky_relu", "leaky_relu", None, "leaky_relu", "leaky_relu", None]
    eng = hip.Mlp("ae", dims, acts, max_batch=64, latent_layer=3, lr=1e-3)
    lins = linears_of(ref.encoder) + linears_of(ref.decoder)
    push_params(eng, lins)
    eng.set_feature_range(r)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    xt = torch.from_numpy(X)
    Xd = torch.from_numpy(Xn).cuda()
    ref_losses = []
    eng.reset_log(64)
    # first step: gradients
    b0 = onn.batches(tr, 64, False)[0]
    eng.forward(Xd, idx=b0.cuda())
    eng.backward(Xd, idx=b0.cuda())
    loss, _ = ref.step(xt[b0])
    opt.zero_grad()
    loss.backward()
    g = eng.grads_view().cpu().numpy()
    for l, lin in enumerate(lins):
        wo, bo = eng.offsets[l]
        gw = lin.weight.grad.numpy()
        assert rel_err(g[wo:wo + gw.size].reshape(gw.shape), gw) < 1e-3, f"layer {l}"
        assert rel_err(g[bo:bo + lin.bias.numel()], lin.bias.grad.numpy()) < 1e-3, f"bias {l}"
    eng.reset_log(64)
    for epoch in range(5):
        for b in onn.batches(tr, 64, False):
            opt.zero_grad()
            loss, _ = ref.step(xt[b])
            loss.backward()
            opt.step()
            ref_losses.append(float(loss))
            eng.train_step(Xd, idx=b.cuda())
    log = eng.read_log()
    np.testing.assert_allclose(log[:, 0], ref_losses, rtol=1e-4)
    for (w, b), lin in zip(eng.get_linears(), lins):
        np.testing.assert_allclose(w, lin.weight.detach().numpy(), atol=1e-4)
    # encoder inference + min/max
    ref.eval()
    with torch.no_grad():
        Y = ref.forward_cv(xt).numpy()
    out, mm = eng.infer(Xd, want_minmax=True)
    np.testing.assert_allclose(out.cpu().numpy(), Y, atol=2e-5)
    np.testing.assert_allclose(mm.cpu().numpy(), np.stack([Y.min(0), Y.max(0)]), atol=2e-5)
    eng.close()


@pytest.mark.parametrize("model", ["ae", "deep_tica"])
def test_ragged_width_training_matches_oracle(model):
    """Widths that are no multiple of 4 (odd weight counts, rows that are not 16-byte aligned): the scalar loaders of the
    block engine, the scalar items of the gradient reduction, the partial units of the fused small-network staging and
    its 4-byte partial stores.  Same step sequence as the oracle (torch CPU autograd, float32), SGD with momentum so
    that a parameter with an exactly-zero gradient is not noise-driven."""
    from deep_cartograph_amd import hip

    n, F, lag, bs = 1500, 37, 3, 200
    X = ar_features(n, F, 11)
    Xn, m, r = normalized(X)
    torch.manual_seed(46)
    if model == "ae":
        ref = onn.AEModel([F, 19, 7, 3], ["leaky_relu", "tanh", None], None, [3, 7, 19, F], ["leaky_relu", "tanh", None], None, m, r)
        dims, acts = [F, 19, 7, 3, 7, 19, F], ["leaky_relu", "tanh", None, "leaky_relu", "tanh", None]
        eng = hip.Mlp("ae", dims, acts, max_batch=bs, latent_layer=3, optimizer="SGD", lr=1e-2, momentum=0.9)
        lins = linears_of(ref.encoder) + linears_of(ref.decoder)
        xt = torch.from_numpy(X)
    else:
        dims, acts = [F, 19, 7, 3], ["leaky_relu", "tanh", None]
        ref = onn.DeepTICAModel(dims, acts, None, None, None, 1e-6)
        eng = hip.Mlp("deep_tica", dims, acts, max_batch=bs, lag=lag, tica_reg=1e-6, optimizer="SGD", lr=1e-2, momentum=0.9)
        lins = linears_of(ref.nn)
        xt = torch.from_numpy(Xn)
    push_params(eng, lins)
    if model == "ae":
        eng.set_feature_range(r)
    opt = torch.optim.SGD(ref.parameters(), lr=1e-2, momentum=0.9)
    Xd = torch.from_numpy(Xn).cuda()
    eng.reset_log(64)
    ref_losses = []
    for step in range(12):
        b = torch.arange(step * 97, step * 97 + (bs if step % 3 else bs - 13))   # ragged batch every third step
        opt.zero_grad()
        loss = ref.step(xt[b])[0] if model == "ae" else ref.step(xt[b], xt[b + lag])[0]
        loss.backward()
        opt.step()
        ref_losses.append(float(loss))
        if step % 2:
            eng.train_step(Xd, idx=b.cuda())                 # gathered rows
        else:
            eng.train_step(Xd, row0=int(b[0]), batch=len(b))  # contiguous rows
    log = eng.read_log()
    dev_w = max(float(np.max(np.abs(w - lin.weight.detach().numpy()))) for (w, _), lin in zip(eng.get_linears(), lins))
    dev_b = max(float(np.max(np.abs(b_ - lin.bias.detach().numpy()))) for (_, b_), lin in zip(eng.get_linears(), lins))
    print(f"ragged widths, {model}: loss dev {np.max(np.abs(log[:, 0] - ref_losses) / np.abs(ref_losses)):.2e}, weights {dev_w:.2e}, biases {dev_b:.2e}")
    # measured: loss 1.3e-7 (ae) / 2.0e-6 (deep_tica), weights 1.4e-7, biases 1.3e-7
    np.testing.assert_allclose(log[:, 0], ref_losses, rtol=8e-6)
    assert dev_w < 5e-7 and dev_b < 5e-7
    eng.close()


def test_infer_reproduces_reference_torchscript(features, golden_nn, golden_proj):
    """a15: the bundled deep_tica model.zip (parameters + buffers) through the HIP engine
    gives the reference's own outputs."""
    from deep_cartograph_amd import hip

    X = features[0]
    g = golden_nn
    mean = g["deep_tica.buffer.norm_in.mean"]
    rng = g["deep_tica.buffer.norm_in.range"]
    Xd = torch.from_numpy(X).cuda()
    Xn = hip.normalize(Xd, torch.from_numpy(mean).cuda(), torch.from_numpy(rng).cuda())
    eng = hip.Mlp("deep_tica", [54, 16, 8, 2], ["leaky_relu", "leaky_relu", None], max_batch=100, lag=1)
    eng.set_linears([(g[f"deep_tica.param.nn.nn.{i}.weight"], g[f"deep_tica.param.nn.nn.{i}.bias"]) for i in (0, 3, 6)])
    out, _ = eng.infer(Xn, tmean=torch.from_numpy(g["deep_tica.buffer.tica.mean"]).cuda(),
                       tevecs=torch.from_numpy(g["deep_tica.buffer.tica.evecs"]).cuda(),
                       pmean=torch.from_numpy(g["deep_tica.buffer.postprocessing.mean"]).cuda(),
                       prange=torch.from_numpy(g["deep_tica.buffer.postprocessing.range"]).cuda())
    np.testing.assert_allclose(out.cpu().numpy(), g["deep_tica.output"], atol=2e-5)
    assert np.mean(ol.csv_round4(out.cpu().numpy()) == golden_proj["deep_tica"]) > 0.97
    eng.close()


@pytest.mark.parametrize("dims,acts,n,cap", [
    ([70, 33, 17, 3], ["tanh", "leaky_relu", None], 1000, 384),       # ragged widths, chunked (3 calls)
    ([512, 256, 128, 4], ["leaky_relu", "leaky_relu", None], 5000, 8192),
    ([54, 5], [None], 164, 164),                                      # a single Linear
])
def test_input_sensitivity_matches_autograd(dims, acts, n, cap):
    """dcv_mlp_input_sensitivity: sum_r |d(g . net(xn_r))/d xn_i| * scale_i against float64
    autograd through the same Linear chain; tolerance 2e-4 relative (fp32 products vs float64)."""
    from deep_cartograph_amd import hip

    rng = np.random.default_rng(5)
    Xn = rng.standard_normal((n, dims[0])).astype(np.float32)
    torch.manual_seed(9)
    seq = onn.feed_forward(dims, acts)
    lins = linears_of(seq)
    g = rng.standard_normal(dims[-1]).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, dims[0]).astype(np.float32)
    eng = hip.Mlp("deep_tica", dims, acts, max_batch=cap, lag=0, tica_reg=1e-6)
    push_params(eng, lins)
    got = eng.input_sensitivity(torch.from_numpy(Xn).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(scale).cuda()).cpu().numpy()
    ref = seq.double()
    x = torch.from_numpy(Xn).double().requires_grad_(True)
    out = (ref(x) * torch.from_numpy(g).double()).sum()
    grad = torch.autograd.grad(out, x)[0].numpy()
    exp = (np.abs(grad) * scale.astype(np.float64)).sum(axis=0)
    assert got.shape == exp.shape
    np.testing.assert_allclose(got, exp, rtol=2e-4)
    eng.close()


# ----------------------------------------------------------------------------- two ranks on one GPU (gloo)
def _dp_rank(rank, world, port, tmpdir):
    """One data-parallel rank of the bench's collective path: forward, all-reduce of the batch statistics, backward,
    all-reduce of the gradient buffer, Adam -- on this rank's contiguous block of frames."""
    import os

    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deep_cartograph_amd import hip

    torch.cuda.set_device(0)
    z = np.load(os.path.join(tmpdir, "dp.npz"))
    Xn, dims, lag, lb, steps = z["Xn"], [int(v) for v in z["dims"]], int(z["lag"]), int(z["lb"]), int(z["steps"])
    n_local = Xn.shape[0] // world
    Xd = torch.from_numpy(Xn[rank * n_local:(rank + 1) * n_local]).cuda()
    acts = ["leaky_relu"] * (len(dims) - 2) + [None]
    eng = hip.Mlp("deep_tica", dims, acts, max_batch=lb, lag=lag, tica_reg=1e-6, lr=1e-3)
    eng.set_linears([(z[f"w{i}"], z[f"b{i}"]) for i in range(len(dims) - 1)])
    eng.reset_log(4 * steps + 8)
    sv, gv = eng.stats_view(), eng.grads_view()
    for i in range(steps):
        r0 = i * lb
        if i % 2 == 0:   # the engine's own sequence, in both forms: the two-piece one (upper-layer gradients all-reduced
            # under the layer-0 weight gradient; the default from 32768 rows per rank up) and the one-piece one
            os.environ["DCV_DP_OVERLAP"] = "1" if i % 4 == 0 else "0"
            eng.data_parallel_step(Xd, dist, lb * world, row0=r0, batch=lb)
            del os.environ["DCV_DP_OVERLAP"]
        else:            # the same step written out with one gradient all-reduce
            eng.forward(Xd, row0=r0, batch=lb)
            dist.all_reduce(sv, op=dist.ReduceOp.SUM)
            eng.backward(Xd, row0=r0, batch=lb, global_batch=lb * world, train=True)
            dist.all_reduce(gv, op=dist.ReduceOp.SUM)
            eng.apply()
    torch.cuda.synchronize()
    lin = eng.get_linears()
    np.savez(os.path.join(tmpdir, f"dp_rank{rank}.npz"), loss=eng.read_log()[:steps, 0], **{f"w{i}": w for i, (w, _) in enumerate(lin)})
    eng.close()
    dist.destroy_process_group()


def test_data_parallel_two_ranks_match_single_process(tmp_path):
    """SURVEY 8e, Deep-TICA step: two ranks (frame blocks, batch statistics and gradients all-reduced) follow the same
    trajectory as one process given the union batch through a gather index; tolerance 2e-5 on the weights after 4 steps
    (summation order of the fp32 partial sums differs), losses 1e-5."""
    import socket

    import torch.multiprocessing as mp

    from deep_cartograph_amd import hip

    dims, lag, lb, steps, world = [64, 32, 16, 3], 5, 640, 4, 2
    X = ar_features(2 * 3000, dims[0], 21)
    Xn, _, _ = normalized(X)
    torch.manual_seed(4)
    acts = ["leaky_relu"] * (len(dims) - 2) + [None]
    seq = onn.feed_forward(dims, acts)
    lins = linears_of(seq)
    save = {f"w{i}": l.weight.detach().numpy() for i, l in enumerate(lins)}
    save.update({f"b{i}": l.bias.detach().numpy() for i, l in enumerate(lins)})
    np.savez(tmp_path / "dp.npz", Xn=Xn, dims=np.array(dims), lag=lag, lb=lb, steps=steps, **save)
    # single process: the same pairs per step (rank-major) through a gather index
    n_local = Xn.shape[0] // world
    eng = hip.Mlp("deep_tica", dims, acts, max_batch=lb * world, lag=lag, tica_reg=1e-6, lr=1e-3)
    push_params(eng, lins)
    eng.reset_log(4 * steps + 8)
    Xd = torch.from_numpy(Xn).cuda()
    for i in range(steps):
        idx = torch.cat([torch.arange(r * n_local + i * lb, r * n_local + (i + 1) * lb) for r in range(world)]).cuda()
        eng.train_step(Xd, idx=idx)
    torch.cuda.synchronize()
    ref_lin = eng.get_linears()
    ref_loss = eng.read_log()[:steps, 0]
    eng.close()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_dp_rank, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        z = np.load(tmp_path / f"dp_rank{r}.npz")
        np.testing.assert_allclose(z["loss"], ref_loss, rtol=1e-5, atol=1e-6)
        for i, (w, _) in enumerate(ref_lin):
            np.testing.assert_allclose(z[f"w{i}"], w, atol=2e-5)


def test_graphed_steps_match_plain_launches():
    """With step graphs switched on (dcv_mlp_set_graph / DCV_GRAPH=1), on a capturing-capable (non-null) stream a step is captured into a hipGraph whose
    instantiation is updated in place every call (dcv_mlp_train_step / forward / backward / eval_step); on the null
    stream the same kernels are launched one by one.  Same kernels, same order: the parameters after several steps, with changing batch offsets,
    an evaluation step in between and a changing batch size, must be bit-identical."""
    from deep_cartograph_amd import hip

    dims, lag = [64, 32, 16, 3], 5
    acts = ["leaky_relu", "leaky_relu", None]
    X = ar_features(6000, dims[0], 31)
    Xn, _, _ = normalized(X)
    torch.manual_seed(6)
    lins = linears_of(onn.feed_forward(dims, acts))
    Xd = torch.from_numpy(Xn).cuda()

    def run(stream):
        eng = hip.Mlp("deep_tica", dims, acts, max_batch=1024, lag=lag, tica_reg=1e-6, lr=1e-3)
        push_params(eng, lins)
        eng.reset_log(64)
        eng.set_graph(True)
        ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.default_stream())
        with ctx:
            for i in range(5):
                eng.train_step(Xd, row0=100 * i, batch=1024)
            eng.eval_step(Xd, row0=3000, batch=1024)
            for i in range(3):                       # split calls, as the data-parallel path makes them
                eng.forward(Xd, row0=50 * i, batch=768)
                eng.backward(Xd, row0=50 * i, batch=768, global_batch=768, train=True)
                eng.apply()
            eng.train_step(Xd, row0=7, batch=1024)
        torch.cuda.synchronize()
        out = eng.get_linears(), eng.read_log()[:10].copy(), eng.graph_launches()
        eng.close()
        return out

    plain, plain_log, n_plain = run(None)
    side = torch.cuda.Stream()
    graphed, graphed_log, n_graphed = run(side)
    assert n_plain == 0          # the default stream cannot capture
    assert n_graphed >= 8        # every call after the first of each kind went out as a graph
    for (w0, b0), (w1, b1) in zip(plain, graphed):
        np.testing.assert_array_equal(w0, w1)
        np.testing.assert_array_equal(b0, b1)
    np.testing.assert_array_equal(plain_log, graphed_log)


def test_native_rccl_communicator_world1():
    """dcv_comm_* (the library's own RCCL communicator) with one rank: creation from a unique id, an in-place all-reduce,
    and data-parallel steps through dcv_mlp_dp_step + dcv_comm_dp_allreduce_fn -- entirely inside the library -- against
    the same steps through the torch.distributed-free single-GPU path.  (No multi-GPU node is available to the builder:
    a multi-rank communicator has not executed; bench.py --native-rccl is the switch for a node that has one.)"""
    from deep_cartograph_amd import hip

    comm = hip.RcclComm(None)
    assert comm.world == 1 and comm.rank == 0
    t = torch.arange(1000, dtype=torch.float64, device="cuda")
    comm.all_reduce(t)
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), torch.arange(1000, dtype=torch.float64))
    dims, lag, batch = [64, 32, 16, 3], 5, 1024
    acts = ["leaky_relu", "tanh", None]
    Xn, _, _ = normalized(ar_features(4000, dims[0], 3))
    torch.manual_seed(9)
    ref = onn.DeepTICAModel(dims, acts, None, None, None, 1e-6)
    Xd = torch.from_numpy(Xn).cuda()
    res = {}
    for mode in ("native", "single", "native_overlap"):
        eng = hip.Mlp("deep_tica", dims, acts, max_batch=batch, lag=lag, tica_reg=1e-6, lr=1e-3)
        push_params(eng, linears_of(ref.nn))
        eng.reset_log(16)
        if mode == "native_overlap":
            os_env = __import__("os").environ
            os_env["DCV_DP_OVERLAP"] = "1"
        for i in range(5):
            if mode == "single":
                eng.train_step(Xd, row0=17 * i, batch=batch)
            else:
                eng.data_parallel_step(Xd, comm, batch, row0=17 * i, batch=batch, train=True)
        if mode != "single":
            eng.data_parallel_step(Xd, comm, batch, row0=2000, batch=batch, train=False)
        else:
            eng.eval_step(Xd, row0=2000, batch=batch)
        if mode == "native_overlap":
            os_env.pop("DCV_DP_OVERLAP", None)
        res[mode] = (eng.read_log()[:, 0].copy(), [w for w, _ in eng.get_linears()])
        eng.close()
    for mode in ("native", "native_overlap"):
        np.testing.assert_allclose(res[mode][0], res["single"][0], rtol=1e-5, atol=1e-6)
        for w, w0 in zip(res[mode][1], res["single"][1]):
            np.testing.assert_allclose(w, w0, atol=2e-6)
    comm.close()


_SWITCH_SCRIPT = r"""
import ctypes, hashlib, sys
import numpy as np, torch
sys.path.insert(0, {root!r})
from deep_cartograph_amd import _lib, hip
tile_rows = _lib.load().dcv_debug_snet_tile_rows
tile_rows.restype, tile_rows.argtypes = ctypes.c_int, [ctypes.c_void_p]
rng = np.random.Generator(np.random.PCG64(5))
model = sys.argv[1]
F, n, batches, path = 96, 12000, [1999, 2048] * 4, 2 if model.startswith("deep_tica") else 1
if model == "deep_tica":
    dims, acts = [96, 64, 32, 3], ["leaky_relu", "tanh", None]
    eng = hip.Mlp("deep_tica", dims, acts, max_batch=2048, lag=7, tica_reg=1e-6, lr=1e-3)
elif model == "deep_tica_d4":   # d = 4, its backward stages 464 table entries; 16- to 128-row tiles
    F, n, batches = 54, 20000, [1000, 4000, 6000, 8193, 12000, 1000, 6000, 12000]
    dims, acts = [54, 32, 32, 16, 4], ["tanh", "tanh", "tanh", None]
    eng = hip.Mlp("deep_tica", dims, acts, max_batch=12000, lag=7, tica_reg=1e-6, lr=1e-3)
elif model == "vae":
    dims, acts = [96, 48, 16, 4, 16, 48, 96], ["leaky_relu", "leaky_relu", None, "leaky_relu", "leaky_relu", None]
    batches = [1999, 4096] * 4
    eng = hip.Mlp("vae", dims, acts, max_batch=4096, latent_layer=3, lr=1e-3)
    eng.set_feature_range(np.ones(96, np.float32))
    eng.set_kl_beta(0.5)
    eng.set_noise(torch.from_numpy(rng.standard_normal((sum(batches), 2)).astype(np.float32)).cuda())
else:
    dims, acts = [96, 48, 16, 2, 16, 48, 96], ["leaky_relu", "leaky_relu", None, "leaky_relu", "leaky_relu", None]
    eng = hip.Mlp("ae", dims, acts, max_batch=2048, latent_layer=3, lr=1e-3)
    eng.set_feature_range(np.ones(96, np.float32))
torch.manual_seed(3)
lins = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]
if model == "vae":   # the decoder's first Linear reads z: half the heads' outputs
    lins[3] = torch.nn.Linear(2, dims[4])
eng.set_linears([(l.weight.detach().numpy(), l.bias.detach().numpy()) for l in lins])
X = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32).cumsum(0) * 0.02 + rng.standard_normal((n, F)).astype(np.float32)).cuda()
eng.reset_log(64)
trs = []
for i, b in enumerate(batches):
    eng.train_step(X, row0=i * 1000 if b + 8 <= n - i * 1000 else n - b - 8, batch=b)
    assert eng.last_path() == path, (model, b, eng.last_path())
    trs.append(tile_rows(eng.h))
torch.cuda.synchronize()
h = hashlib.sha256()
for w, b in eng.get_linears():
    h.update(np.ascontiguousarray(w).tobytes()); h.update(np.ascontiguousarray(b).tobytes())
h.update(np.ascontiguousarray(eng.read_log()[:8]).tobytes())
print("TILES", trs)
print("HASH", h.hexdigest())
"""


@pytest.mark.parametrize("model", ["deep_tica", "ae", "deep_tica_d4", "vae"])
def test_launch_time_switches_leave_the_bits_alone(model, tmp_path):
    """The speed switches of the library change how results are stored or summed up in the SAME order, never the results:
    write-through epilogue stores (DCV_WT), the flat-grid gradient reduction (DCV_REDUCE_QUAD), the grouped weight /
    input gradient launch (DCV_NO_PAIR), the table-driven weight staging of the fused small-network kernels in place of the
    weight image (DCV_SNET_IMG=0).  Eight training steps in fresh processes (the switches are read once per process), every
    one on the fused kernels; parameters and loss records hashed."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "switch_run.py"
    script.write_text(_SWITCH_SCRIPT.format(root=root))
    hashes, tiles = {}, {}
    for name, env in (("default", {}), ("plain stores", {"DCV_WT": "0"}), ("round-2 reduction", {"DCV_REDUCE_QUAD": "0"}),
                      ("two launches", {"DCV_NO_PAIR": "1"}), ("table staging", {"DCV_SNET_IMG": "0"})):
        e = dict(os.environ)
        e.update(env)
        out = subprocess.run([sys.executable, str(script), model], env=e, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        hashes[name] = [l for l in out.stdout.splitlines() if l.startswith("HASH")][-1]
        tiles[name] = [l for l in out.stdout.splitlines() if l.startswith("TILES")][-1]
    assert len(set(hashes.values())) == 1, hashes
    expect = {"deep_tica": [32] * 8, "ae": [16] * 8, "vae": [16, 32] * 4, "deep_tica_d4": [16, 32, 64, 128, 128, 16, 64, 128]}[model]
    assert set(tiles.values()) == {f"TILES {expect}"}, tiles


def _fuzz_seeds():
    """The ten seeds of the suite, plus a range for one-off sweeps: DCV_FUZZ_SEEDS=100:200 (profiles/r04_gpu_calls.log has the
    sweeps that were run)."""
    extra = os.environ.get("DCV_FUZZ_SEEDS", "")
    if ":" in extra:
        lo, hi = extra.split(":")
        return list(range(10)) + list(range(int(lo), int(hi)))
    return list(range(10))


@pytest.mark.parametrize("seed", _fuzz_seeds())
def test_random_configurations_match_oracle(seed):
    """Random small configurations (widths 2..150 incl. odd ones, 1-3 hidden layers, batch 20..700, gathered or contiguous
    rows, both models, mixed activations): three SGD steps against the float32 autograd oracle.  Exercises whichever tile
    shapes, split plans, scalar / vector loaders and reduction items the shapes select."""
    from deep_cartograph_amd import hip

    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    model = "ae" if seed % 2 else "deep_tica"
    F = int(rng.integers(5, 150))
    hidden = [int(rng.integers(3, 120)) for _ in range(int(rng.integers(1, 4)))]
    d = int(rng.integers(1, 5))
    lag = int(rng.integers(1, 9))
    bs = int(rng.integers(20, 700))
    n = bs + lag + 64
    act_pool = ["leaky_relu", "tanh", "relu", "elu", "softplus"]
    X = ar_features(n, F, 300 + seed)
    Xn, m, r = normalized(X)
    torch.manual_seed(500 + seed)
    enc_dims = [F] + hidden + [d]
    enc_acts = [act_pool[int(rng.integers(0, len(act_pool)))] for _ in hidden] + [None]
    if model == "ae":
        dec_dims = enc_dims[::-1]
        dec_acts = [act_pool[int(rng.integers(0, len(act_pool)))] for _ in hidden] + [None]
        ref = onn.AEModel(enc_dims, enc_acts, None, dec_dims, dec_acts, None, m, r)
        dims, acts = enc_dims + dec_dims[1:], enc_acts + dec_acts
        eng = hip.Mlp("ae", dims, acts, max_batch=bs, latent_layer=len(enc_dims) - 1, optimizer="SGD", lr=5e-3, momentum=0.5)
        eng.set_feature_range(r)
        lins = linears_of(ref.encoder) + linears_of(ref.decoder)
        xt = torch.from_numpy(X)
    else:
        ref = onn.DeepTICAModel(enc_dims, enc_acts, None, None, None, 1e-6)
        dims, acts = enc_dims, enc_acts
        eng = hip.Mlp("deep_tica", dims, acts, max_batch=bs, lag=lag, tica_reg=1e-6, optimizer="SGD", lr=5e-3, momentum=0.5)
        lins = linears_of(ref.nn)
        xt = torch.from_numpy(Xn)
    push_params(eng, lins)
    opt = torch.optim.SGD(ref.parameters(), lr=5e-3, momentum=0.5)
    Xd = torch.from_numpy(Xn).cuda()
    eng.reset_log(8)
    ref_losses = []
    for step in range(3):
        nb = bs if step != 1 else max(8, bs - int(rng.integers(1, 17)))
        start = int(rng.integers(0, 32))
        b = torch.arange(start, start + nb)
        opt.zero_grad()
        loss = ref.step(xt[b])[0] if model == "ae" else ref.step(xt[b], xt[b + lag])[0]
        loss.backward()
        opt.step()
        ref_losses.append(float(loss))
        if (seed + step) % 2:
            eng.train_step(Xd, idx=b.cuda())
        else:
            eng.train_step(Xd, row0=start, batch=nb)
    log = eng.read_log()[:3, 0]
    assert np.all(np.isfinite(log)), (model, dims, acts, bs, log)
    scale = max(1.0, max(float(l.weight.abs().max()) for l in lins))
    dev_w = max(float(np.max(np.abs(w - lin.weight.detach().numpy()))) for (w, _), lin in zip(eng.get_linears(), lins)) / scale
    dev_l = float(np.max(np.abs(log - ref_losses) / np.maximum(np.abs(ref_losses), 1e-3)))
    print(f"random config {seed}: {model} {dims} {acts} batch {bs} lag {lag}: loss dev {dev_l:.1e}, weight dev {dev_w:.1e}")
    assert dev_l < 1e-5 and dev_w < 3e-7, (model, dims, acts, bs, lag, dev_l, dev_w)   # measured: <= 2.4e-6 / 6.0e-8
    eng.close()
