"""One autoencoder step in plain torch (float64 by default), kink-aware, and the case tables of tests/test_ae_block_gpu.py:
the shapes at which an autoencoder / VAE step leaves the fused small-network kernel and runs on the block engine (run_forward /
backward_impl in csrc/mlp.hip, the products of gemm_kernels.h, pair.hip, ride.hip, the reductions of mlp_opt.hip).

    h = act_l(h W_l^T + b_l) for every Linear;  loss = mean(((x_hat - xn) * range)^2)

Nothing here needs a GPU: tests/test_ae_block_oracle_cpu.py pins ae_step against float64 autograd of oracle.nn.AEModel, checks
that every case is well conditioned (the float32 run of ae_step against the float64 one) and counts the arithmetic claims
of the tables.  The tables are functions of the CU count n, as _big_case (tests/test_mlp_gpu.py): the tile choice (pick_cfg)
and several thresholds follow it."""
import functools

import numpy as np
import torch

from oracle import nn as onn
from tests.test_mlp_gpu import ar_features_fast, linears_of, normalized

GRAD_TOL, REC_TOL = 2e-5, 1e-5   # tests/test_snet_dt_gpu.py, tests/test_vae_step_gpu.py
KINK = 1e-5                      # check_step_against_float64 (tests/test_mlp_gpu.py): slope decisions may differ inside it
LEAKY_SLOPE = 0.01


@functools.lru_cache(maxsize=2)   # the two flavours of a case run back to back
def _features(n, F, seed):
    """(Xn, range) of n rows x F features, generated once per shape and shared (never written to)."""
    Xn, _, r = normalized(ar_features_fast(n, F, seed))
    return Xn, r


def ae_case(dims, acts, latent, n, seed):
    """Inputs and float32 parameters of one case: n rows of normalised AR(1) features, their range (the standard deviations
    of the raw features, 0.1 .. 10: range^2 enters ae_dY_kernel), and the Linears of a seeded oracle.nn.AEModel, which reads
    x = Xn * range with a zero mean (tests/test_snet_dt_gpu.py: _ae_setup), so that its loss is the engine's."""
    Xn, r = _features(n, dims[0], 29)
    torch.manual_seed(seed)
    ref = onn.AEModel(dims[:latent + 1], acts[:latent], None, dims[latent:], acts[latent:], None, np.zeros(dims[0], np.float32), r)
    lins = linears_of(ref.encoder) + linears_of(ref.decoder)
    return dict(dims=list(dims), acts=list(acts), latent=latent, Xn=Xn, range=r, ref=ref,
                Ws=[l.weight.detach().clone() for l in lins], bs=[l.bias.detach().clone() for l in lins])


ROW0 = 7


def matrix_rows(rows):
    """rows of the feature matrix of a case that steps on `rows` of them: room for row0 and a few hundred more, so that an
    inference pass over the whole matrix crosses a chunk seam (the engine's row capacity is the batch)"""
    return rows + ROW0 + 300


def rows_of(c, rows, form, seed):
    """The logical rows of a batch: a random permutation of the matrix's rows (gathered) or the contiguous rows from ROW0."""
    if form == "idx":
        return np.random.Generator(np.random.PCG64(seed)).permutation(c["Xn"].shape[0])[:rows].astype(np.int64)
    return np.arange(ROW0, ROW0 + rows, dtype=np.int64)


def kink_layers(acts):
    """Layers whose activation has a kink: their slope decisions are compared, and may be held fixed."""
    return [l for l, a in enumerate(acts) if a in ("leaky_relu", "relu")]


def ae_step(x, Ws, bs, acts, rng, patterns=None, dtype=torch.float64):
    """One autoencoder step on the rows x in `dtype`.  patterns: {layer: boolean slope pattern} of leaky-ReLU / ReLU layers to
    hold fixed (the network is then piecewise linear in them); layers not named take their own.  Returns the slope decisions
    `own` and pre-activations `z` of those layers ({layer: tensor}), the loss, the sum of squared errors, and the weight /
    bias gradients as float64 NumPy arrays in layer order."""
    W = [w.to(dtype).clone().requires_grad_(True) for w in Ws]
    b = [v.to(dtype).clone().requires_grad_(True) for v in bs]
    xn = torch.as_tensor(x).to(dtype)
    r = torch.as_tensor(rng).to(dtype)
    h, own, zs = xn, {}, {}
    for l, a in enumerate(acts):
        z = h @ W[l].T + b[l]
        if a in ("leaky_relu", "relu"):
            own[l], zs[l] = z.detach() > 0, z.detach()
            m = own[l] if patterns is None or patterns.get(l) is None else patterns[l]
            # (the two slopes as tensors of `dtype`: torch.where on Python scalars would round 0.01 to float32 first)
            h = z * torch.where(m, torch.ones((), dtype=dtype), torch.tensor(LEAKY_SLOPE if a == "leaky_relu" else 0.0, dtype=dtype))
        elif a == "tanh":
            h = torch.tanh(z)
        elif a == "elu":
            h = torch.nn.functional.elu(z)
        else:
            assert a is None, f"ae_step: activation {a!r} is not restated here"
            h = z
    sq = ((h - xn) * r).square()
    loss = sq.mean()
    loss.backward()
    np64 = lambda t: t.detach().double().numpy()
    return dict(own=own, z=zs, loss=float(loss.detach()), sse=float(sq.detach().sum()), gw=[np64(w.grad) for w in W], gb=[np64(v.grad) for v in b])


def rel_dev(a, b):
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300))


def step_deviation(o, ref):
    """(worst gradient tensor deviation of o from ref, relative to the tensor's largest entry; relative loss deviation)."""
    g = max(max(rel_dev(a, b) for a, b in zip(o["gw"], ref["gw"])), max(rel_dev(a, b) for a, b in zip(o["gb"], ref["gb"])))
    return g, abs(o["loss"] - ref["loss"]) / abs(ref["loss"])


def encoder_with_bound(x, Ws, bs, acts, n_layers):
    """The first n_layers layers in float64 on the float32 rows x, and an element-wise bound on what a float32 evaluation may
    deviate by: per layer the float32 product bound of forward_layers_against_float64 (tests/test_mlp_gpu.py) on the
    pre-activation plus 4 ulp of the result, plus the bound of the layer's input carried through |W| (every activation here
    has slope <= 1)."""
    h = np.asarray(x, dtype=np.float64)
    e = np.zeros_like(h)
    for l in range(n_layers):
        W, b = Ws[l].double().numpy(), bs[l].double().numpy()
        z = h @ W.T + b
        a = acts[l]
        ref = z if a is None else np.tanh(z) if a == "tanh" else np.where(z > 0, z, np.expm1(np.minimum(z, 0))) if a == "elu" else \
            np.where(z > 0, z, (LEAKY_SLOPE if a == "leaky_relu" else 0.0) * z)
        e = 4e-7 * (np.abs(h) @ np.abs(W).T + np.abs(b)) + 1e-6 + 4 * 2.0 ** -24 * np.abs(ref) + e @ np.abs(W).T
        h = ref
    return h, e


# ---------------------------------------------------------------------------------------------- plans restated from csrc
def cdiv(a, b):
    return -(-a // b)


K_SSE_ROWS = 16   # csrc/mlp_state.h: kSseRows


def ae_sse_plan(R, F):
    """ae_sse (csrc/mlp_heads.hip) restated: (regime, rows per block, blocks, whether the kSseRows clamp
    set the rows per block).  Regimes by R * F: '16/thread' (one block per
    4096 elements, at most 128), 'floor128' (128 blocks), '64/thread' (one block per 16 384 elements), 'cap512'."""
    elems = R * F
    want, regime = cdiv(elems, 256 * 16), "16/thread"
    if want > 128:
        w64 = cdiv(elems, 256 * 64)
        want, regime = (w64, "64/thread") if w64 > 128 else (128, "floor128")
    if want > 512:
        want, regime = 512, "cap512"
    want = max(want, 1)
    rpb = cdiv(R, want)
    clamped = rpb < K_SSE_ROWS
    rpb = max(rpb, K_SSE_ROWS)
    return regime, rpb, cdiv(R, rpb), clamped


def dY_trips(R, F, n):
    """trips of ae_dY_kernel's grid-stride loop: the grid is capped at 16 blocks of 256 threads per CU (loss_gradient)"""
    return cdiv(R * F, min(cdiv(R * F, 256), 16 * n) * 256)


def bias_partials(R):
    """bias-gradient partials a last layer leaves: one per kColsumRows = 32 rows (seed_gradient, csrc/mlp.hip)"""
    return cdiv(R, 32)


def off_the_fused_kernel(dims, R):
    """an autoencoder leaves the fused kernel when a width exceeds 256 (snet_layout) or the batch 16 384 rows"""
    return max(dims) > 256 or R > 16384


# ---------------------------------------------------------------------------------------------- case tables
CONTRACT = [512, 256, 128, 2, 128, 256, 512]


def _acts(dims, hidden, latent, latent_act=None, out_act=None):
    a = [hidden] * (len(dims) - 1)
    a[latent - 1], a[-1] = latent_act, out_act
    return a


def step_cases(n):
    """Group A.  name -> dict(dims, acts, latent, rows, form 'row0' | 'idx', train_step, sgd, seed, reach).  At n = 256 CUs:
    8 202, 8 192, 8 202, 16 257, 32 705 and 32 868 rows."""
    t = _acts(CONTRACT, "tanh", 3)
    return {
        # the contract shape.  One ragged row tile past a multiple of the CU count: layer 0 forward at 64 x 64 with the
        # contraction-split tail tile; the latent Linear rides in layer 1's epilogue (head4); first decoder Linear with K = 2
        # (scalar loaders); last layer 64 x 128 tiles at N = 512; last layer's weight + input gradient as ONE launch (pair.hip,
        # 64 x 64 / 64 x 64, N = F); colsum_kernel over 512 columns; as a training step the layer-0 weight gradient carries the
        # reduction of the other five layers (ride.hip, a six-layer item list)
        "A1": dict(dims=CONTRACT, acts=t, latent=3, rows=32 * n + 10, form="row0", train_step=True, sgd=False, seed=6,
                   reach="tail_split, pair 64x64/64x64 at N = F, ride with six layers"),
        # through a random int64 index: gathering loaders on layer 0 (forward and weight gradient); a gathered batch does not ride
        "A2": dict(dims=CONTRACT, acts=t, latent=3, rows=32 * n, form="idx", train_step=True, sgd=False, seed=7,
                   reach="gathering loaders, no ride"),
        # every hidden layer leaky-ReLU: the sign-mask store of the forward epilogues and its read-back by the input gradients
        "A3": dict(dims=CONTRACT, acts=_acts(CONTRACT, "leaky_relu", 3), latent=3, rows=32 * n + 10, form="row0", train_step=False, sgd=False,
                   seed=8, reach="sign masks, kink-aware"),
        # 64 n - 127 rows: the smallest count at which the last layer's forward (N = F = 512: four column tiles) has 2 n tiles of
        # 128 x 128, the last one of a single row.  Its weight gradient is 128 x 128 too but its input gradient (N = 256) takes
        # 64 x 64 tiles: no pair form, the two products launch apart ('single' fallback); layer 1 pairs 64 x 64 / 64 x 64
        "A4a": dict(dims=CONTRACT, acts=t, latent=3, rows=64 * n - 127, form="row0", train_step=False, sgd=False, seed=9,
                    reach="last layer NT 128x128 ragged, single fallback, pair quarter/quarter"),
        # 128 n - 63 rows: the 256-wide layer's input gradient (two column tiles) has 2 n tiles of 128 x 128, the last one ragged, and
        # the 128-wide one 2 n tiles of 64 x 128: the last layer's pair is 128 x 128 / 128 x 128, layer 4's (128 -> 256) is 64 x 64 /
        # 64 x 128; layer 1's products (64 x 64 weight gradient, 128 x 128 input gradient) have no pair form.  The hidden widths are
        # what those forms need: 256 for the first, 128 behind it for the second.  (At the smallest such count, 128 n - 127, the
        # 128-wide input gradient still takes 64 x 64 tiles: the pair A4a shows already.)
        "A4b": dict(dims=CONTRACT, acts=t, latent=3, rows=128 * n - 63, form="row0", train_step=False, sgd=False, seed=10,
                    reach="NN 128x128 ragged, pair big/big and quarter/half"),
        # more than 32 * 1024 rows with F = 320 > 256: cdiv(R, 32) > 1024 bias partials of the last layer, past what the flat-grid
        # reduction takes (quad_takes): the 16-wave reduction kernel, and nothing rides; the training step under plain SGD
        "A5": dict(dims=[320, 128, 4, 128, 320], acts=_acts([320, 128, 4, 128, 320], "tanh", 2), latent=2, rows=128 * n + 100, form="row0",
                   train_step=True, sgd=True, seed=11, reach="last_reduce() == 3, no ride, SGD update"),
    }


NARROW_ROWS = 777


def narrow_cases():
    """Group B: (name, dims, acts, latent, form, mode, rides as, K = d loaders vector).  F = 260: just off the fused kernel.
    The latent Linear rides in the epilogue of the 128-wide layer before it when it has at most 8 outputs (head4 up to 4, head8
    up to 8: next_layer_fusable, run_forward); the first decoder Linear has K = d, with 16-byte loaders only when d % 4 == 0.
    Gathered / contiguous rows and the two flavours alternate so that every d sees both flavours over the table."""
    out = []
    for i, (d, lat_act) in enumerate([(1, None), (2, None), (3, None), (3, "tanh"), (4, None), (5, None), (8, None), (9, None)]):
        dims = [260, 128, d, 128, 260]
        rides = "head4" if d <= 4 else "head8" if d <= 8 else None
        for j, mode in enumerate(("split", "native")):
            form = "idx" if (i + j) % 2 else "row0"
            out.append((f"d{d}{'t' if lat_act else ''}-{mode}", dims, _acts(dims, "tanh", 2, lat_act), 2, form, mode, rides, d % 4 == 0))
    # the layer before the latent too wide to carry it (256 > 128): the unfused narrow products
    for j, mode in enumerate(("split", "native")):
        dims = [260, 256, 3, 256, 260]
        out.append((f"wide3-{mode}", dims, _acts(dims, "tanh", 2), 2, "idx" if j else "row0", mode, None, False))
    return out


LOSS_DIMS = [512, 8, 2, 8, 512]


def loss_rows(n):
    """Group C row counts at F = 512: the kSseRows clamp (1, 17), the last row count of each ae_sse regime and the first of the
    next, the last row count the clamp decides and the first it does not (1 920 / 1 921: at 512 columns the clamp to 16 rows per
    block overrides the whole first regime), and 8 n + 1, the first second trip of ae_dY_kernel's grid-stride loop.
    -> [(rows, whole step too)]"""
    return [(1, False), (17, True), (1024, False), (1025, False), (1920, False), (1921, False), (4096, False), (4097, False), (16384, False), (16385, False), (8 * n + 1, True)]


# the regime each of those counts is there for (checked from ae_sse_plan by the CPU test)
LOSS_REGIMES = {1: "16/thread", 17: "16/thread", 1024: "16/thread", 1025: "floor128", 4096: "floor128", 4097: "64/thread",
                16384: "64/thread", 16385: "cap512"}

# colsum_kernel on a wide last layer: 320 columns take a second, ragged pass (64 of 256); 301 columns the scalar edge
# (n % 4 != 0), with an activation on the output Linear so that act' in ae_dY_kernel is not the identity
COLSUM_NETS = [([320, 64, 3, 64, 320], None), ([301, 64, 3, 64, 301], "tanh")]
COLSUM_ROWS = [77, 1000]

# Group D: (name, dims, latent, d, rides as).  The heads (2 d columns) ride in the 128-wide layer's epilogue, or stand alone
VAE_NETS = [
    ("h4", [512, 256, 128, 4, 128, 256, 512], 3, 2, "head4"),
    ("h8", [512, 256, 128, 8, 128, 256, 512], 3, 4, "head8"),
    ("own", [512, 256, 6, 256, 512], 2, 3, None),
]


def vae_cases(n):
    """(network, rows, form, beta): 32 n + 10 contiguous and 32 n gathered rows; every network sees both betas"""
    out = []
    for i, (name, _, _, _, _) in enumerate(VAE_NETS):
        out.append((name, 32 * n + 10, "row0", (0.3, 4.0)[i % 2]))
        out.append((name, 32 * n, "idx", (4.0, 0.3)[i % 2]))
    return out
