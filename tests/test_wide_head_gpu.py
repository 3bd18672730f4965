"""The Deep-TICA loss head at 5 to 16 outputs against float64, on every form the step takes above d = 4 (DESIGN.md section 2,
"Deep-TICA at 5 to 16 outputs"): the <8> forward head with padded columns, tica_stats_kernel + sum_partials_kernel,
tica_grad_kernel<5> / <6> / <0>, head_backward_kernel<5 .. 8> on either side of head_fusable, tica_dF_kernel, the
2 + 2 d^2 + d record columns, and the entry points that reach them (forward + backward, train_step, eval_step, eval_steps,
train_steps, data_parallel_step).

Oracle: the float64 torch-CPU autograd model (oracle/nn.py) on the engine's float32 parameters and inputs, and beside it the
loss restated from the definition in mlp_heads.hip with torch.linalg.solve -- no Cholesky, no eigh, no code of oracle/nn.py;
the two float64 losses must agree to 1e-10 before the engine is held to either.

Conditioning: a case pins something only where the float32 torch-CPU oracle itself stays within 1e-5 of the float64 one
(worst weight-gradient tensor).  The value measured on the CPU stands beside each case; `python -m tests.test_wide_head_gpu`
prints the table again (no GPU needed) and must be run for any shape, seed or index that changes.
Run on the GPU box: python -m pytest tests -m gpu"""
import copy
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import nn as onn
from tests import dropout_oracle as do
from tests.test_mlp_gpu import ar_features_fast, linears_of, normalized, push_params, rel_err
from tests.test_snet_dt_gpu import _TwoRanksInOneProcess
from tests.test_training_options_gpu import _queue_masks

pytestmark = pytest.mark.gpu

REG = 1e-6
ROW0 = 7                                   # contiguous batches begin here
ENGINE_SEED = 0x1234_5678_9ABC_DEF0 + 5    # dropout cases: a seed whose high word is in use


def _case(dims, batch, lag=1, gather=False, last_act=None, drops=None, n=700):
    return SimpleNamespace(dims=dims, batch=batch, lag=lag, gather=gather, last_act=last_act, drops=drops, n=n, reg=REG)


# name -> case.  Hidden layers tanh, weights from torch.manual_seed(3), features ar_features_fast(n, F, 17) normalised, contiguous
# rows from row 7 or the first `batch` entries of a PCG64(5) permutation.  Behind each case: the float32 oracle's deviation from
# the float64 one (worst weight-gradient tensor; the condition is < 1e-5) and cond(C0), measured on the CPU.
CASES = {
    # ---- every width once; K = 16: C4 = 4 lanes per row group, fused backward up to d = 8
    "d5": _case([40, 16, 5], 100),                                # 8.6e-07, cond 15    one ragged statistics block
    "d6-b129-lag5": _case([40, 16, 6], 129, lag=5),               # 1.4e-06, cond 15    second block of one pair; interior rows: both terms
    "d6-lag150": _case([40, 16, 6], 100, lag=150),                # 2.2e-06, cond 17    lag > batch: test_lag_beyond_the_batch_is_two_halves
    "d6-tanh": _case([40, 16, 6], 100, last_act="tanh"),          # 1.1e-06, cond 16    act'(f) in the fused backward: pick()
    "d6-gather": _case([40, 16, 6], 100, gather=True),            # 1.6e-06, cond 18    lag_off = B, halves disjoint
    "d7-b257": _case([40, 16, 7], 257),                           # 8.8e-07, cond 22    three blocks; <0> head behind the <8> forward
    "d8": _case([40, 16, 8], 100),                                # 1.8e-06, cond 59
    "d8-gather": _case([40, 16, 8], 100, gather=True),            # 6.7e-06, cond 86
    # ---- head_fusable boundaries (K = hidden width in front of the head)
    "k8-d5": _case([40, 8, 5], 100),                              # 1.6e-06, cond 25    C4 = 2 < d: the i += C4 loop
    "k8-d6": _case([40, 8, 6], 100),                              # 2.7e-06, cond 31
    "k8-d7": _case([40, 8, 7], 100, n=1000),                      # 6.0e-06, cond 62    50.4 KB of the 60 KB of LDS (n = 700: 2.8e-5, not usable)
    "k12-d6": _case([40, 12, 6], 100),                            # 2.5e-06, cond 15    256 % 3 != 0: not fused
    "k15-d7": _case([40, 15, 7], 100),                            # 1.3e-06, cond 12    no multiple of 4: not fused
    "k128-d5": _case([64, 128, 5], 300, lag=2),                   # 1.9e-06, cond 4     C4 = 32, eight row groups
    "k256-d8": _case([64, 256, 8], 300),                          # 8.5e-07, cond 11    C4 = 64, four row groups; the head a product of its own
    "k260-d8": _case([64, 260, 8], 300),                          # 8.9e-07, cond 5     C4 = 65 > 64: not fused
    # ---- d = 9 .. 16: a forward product of its own, tica_grad_kernel<0>, tica_dF_kernel
    "d9": _case([40, 16, 9], 100),                                # 2.8e-06, cond 217
    "d9-gather": _case([40, 32, 9], 100, gather=True),            # 1.9e-06, cond 13    ([40, 16, 9] gathered: 1.7e-5, not usable)
    "d10-b257": _case([40, 20, 10], 257),                         # 3.7e-06, cond 36
    "d11": _case([40, 22, 11], 300),                              # 2.7e-06, cond 32
    "d12-lag3": _case([40, 24, 12], 300, lag=3, n=1000),          # 4.8e-06, cond 70
    "d13": _case([40, 32, 13], 300),                              # 2.5e-06, cond 19
    "d14": _case([40, 32, 14], 300),                              # 2.9e-06, cond 40
    "d15": _case([40, 32, 15], 300),                              # 2.3e-06, cond 43
    "d16": _case([40, 32, 16], 300),                              # 2.8e-06, cond 44
    "d16-gather": _case([40, 32, 16], 300, gather=True),          # 4.9e-06, cond 97
    "d16-tanh": _case([40, 32, 16], 300, last_act="tanh"),        # 3.1e-06, cond 42    act'(f) in tica_dF_kernel
    "d16-one-linear": _case([24, 16], 300),                       # 7.5e-06, cond 141   no hidden layer: no input gradient at all
    # ---- 66 statistics blocks: a second round of wave_sum_in_order; 521 blocks of 32 rows in the fused backward
    "d6-b8321": _case([24, 16, 6], 8321, n=8500),                 # 2.9e-06, cond 34
    "d9-b8321": _case([24, 32, 9], 8321, n=8500),                 # 4.3e-06, cond 89
    # ---- more rows than 4 x CUs x 32 = 32 768: 64 rows per block in head_plan.  (No smaller batch gets there: the block count is
    # min(4 x CUs, rows_cap / 32) whatever max_batch is, so 8322 rows run as 521 blocks of 32.)
    "d6-b16401-gather": _case([24, 16, 6], 16401, gather=True, n=33000),   # 2.3e-06, cond 24
    # ---- dropout, the masks from tests/dropout_oracle.py (training under dropout: two halves, lag_off = B)
    "d6-drop-out": _case([40, 16, 6], 100, drops=[0.0, 0.2]),     # 1.6e-06, cond 10    output mask, columns 4 .. 5: the second quad
    "d9-drop-out": _case([40, 32, 9], 100, drops=[0.0, 0.2]),     # 8.8e-07, cond 7     output mask, columns 4 .. 8: second and third quad
    "d6-drop-prev": _case([40, 16, 6], 100, drops=[0.2, 0.0]),    # 7.5e-07, cond 18    drop_prev / hscale_prev of the fused backward
}


@functools.lru_cache(maxsize=None)
def features(n, F):
    """Normalised AR(1) features, generated once per shape and shared (never written to)."""
    return normalized(ar_features_fast(n, F, 17))[0]


def acts_of(c):
    return ["tanh"] * (len(c.dims) - 2) + [c.last_act]


def model_of(c):
    torch.manual_seed(3)
    drops = None if c.drops is None else [p if p else None for p in c.drops]
    return onn.DeepTICAModel(c.dims, acts_of(c), drops, None, None, c.reg)


def index_of(c):
    """the batch's row index (CPU int64) and the keyword arguments that hand the same batch to the engine"""
    if c.gather:
        idx = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).permutation(c.n - c.lag)[:c.batch].astype(np.int64))
        return idx, lambda: dict(idx=idx.cuda())
    return torch.arange(ROW0, ROW0 + c.batch), lambda: dict(row0=ROW0, batch=c.batch)


def loss_from_the_definition(f_t, f_l, reg):
    """mlp_heads.hip, tica_grad_body: mu, mu_lag from the batch; C0 = F^T F / B - mu mu^T; Ctau = sym(F^T F_lag / B - mu mu_lag^T);
    loss = -tr(((C0 + reg I)^-1 Ctau)^2), the inverse applied by an LU solve."""
    B, d = f_t.shape
    mu, ml = f_t.sum(0) / B, f_l.sum(0) / B
    C0 = f_t.T @ f_t / B - torch.outer(mu, mu)
    Ct = f_t.T @ f_l / B - torch.outer(mu, ml)
    Ct = 0.5 * (Ct + Ct.T)
    K = torch.linalg.solve(C0 + reg * torch.eye(d, dtype=f_t.dtype), Ct)
    return -torch.trace(K @ K), C0, Ct, mu


def run_oracle(c, dtype=torch.float64, idx=None):
    """One step of the autograd oracle in `dtype` on the case's batch (or on `idx`): step, backward; the dropout masks of training
    step 0 from tests/dropout_oracle.py (x_t call: rows [0, B) of the engine's 2 B rows, x_lag call: rows [B, 2 B))."""
    m = copy.deepcopy(model_of(c)).to(dtype)
    idx = index_of(c)[0] if idx is None else idx
    B = int(idx.numel())
    if c.drops is not None:
        m.train()
        layers = [l for l, p in enumerate(c.drops) if p > 0]
        mk = {l: do.mask(ENGINE_SEED, 0, l, 0, 2 * B, c.dims[l + 1], c.drops[l]) for l in layers}
        for dm in _queue_masks(m.nn, [[mk[l][:B] for l in layers], [mk[l][B:] for l in layers]]):
            dm.queue = [q.to(dtype) for q in dm.queue]
    outs = []
    hook = m.nn.register_forward_hook(lambda mod, inp, out: outs.append(out.detach().double()))
    x = torch.from_numpy(features(c.n, c.dims[0])).to(dtype)
    loss, _ = m.step(x[idx], x[idx + c.lag])
    loss.backward()
    hook.remove()
    f_t, f_l = outs
    lins = linears_of(m.nn)
    return SimpleNamespace(B=B, d=c.dims[-1], loss=float(loss.detach()), f_t=f_t, f_l=f_l,
                           gw=[l.weight.grad.double().numpy() for l in lins], gb=[l.bias.grad.double().numpy() for l in lins])


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """The float64 oracle of a case, computed once and shared by the tests that need it (never written to)."""
    c = CASES[name]
    o = run_oracle(c)
    ld, o.C0, o.Ct, o.mu = loss_from_the_definition(o.f_t, o.f_l, c.reg)
    assert abs(float(ld) - o.loss) < 1e-10, (name, float(ld), o.loss)   # eigh route vs LU route, both float64
    return o


def float32_oracle_deviation(c, idx=None):
    """The conditioning of a case: worst weight-gradient tensor of the float32 oracle against the float64 one, and cond(C0)."""
    o64, o32 = run_oracle(c, torch.float64, idx), run_oracle(c, torch.float32, idx)
    C0 = loss_from_the_definition(o64.f_t, o64.f_l, c.reg)[1]
    return max(rel_err(a, b) for a, b in zip(o32.gw, o64.gw)), float(np.linalg.cond(C0.numpy()))


# ----------------------------------------------------------------------------- comparison
def used(got, exp, rtol, atol):
    """the share of np.testing.assert_allclose's tolerance the worst entry uses (<= 1 passes)"""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    return float(np.max(np.abs(got - exp) / (atol + rtol * np.abs(exp))))


def compare(c, o, label, *, stats=None, rec=None, grads=None, offsets=None, weight=None):
    """Engine against the float64 oracle `o`, every figure printed before anything is asserted.
    stats: stats_view(), all 2 d + 2 d^2 entries -- rtol 2e-5, atol 2e-5 (sums: atol 1e-4).
    rec: one loss record [loss | weight | C0 | Ctau | mu] -- loss 1e-5 max(1, |loss|); the matrices and the mean are the
         statistics divided by the batch size, and so are their absolute tolerances.
    grads: grads_view() -- max |difference| / max |float64 entry| < 2e-5 per tensor; the last bias without an activation or a
         mask behind the last Linear is exactly zero (the loss ignores a constant shift of the outputs): rounding noise only."""
    d, B = o.d, o.B
    fig, bad = {}, []

    def hold(name, value, bound=1.0):
        fig[name] = value
        if not value < bound:
            bad.append(f"{name}: {value:.3e} (bound {bound:g})")

    if stats is not None:
        assert stats.shape == (2 * d + 2 * d * d,)
        hold("sum f_t", used(stats[:d], o.f_t.sum(0).numpy(), 2e-5, 1e-4))
        hold("sum f_lag", used(stats[d:2 * d], o.f_l.sum(0).numpy(), 2e-5, 1e-4))
        hold("f_t^T f_t", used(stats[2 * d:2 * d + d * d].reshape(d, d), (o.f_t.T @ o.f_t).numpy(), 2e-5, 2e-5))
        hold("f_t^T f_lag", used(stats[2 * d + d * d:].reshape(d, d), (o.f_t.T @ o.f_l).numpy(), 2e-5, 2e-5))
    if rec is not None:
        assert rec.shape == (2 + 2 * d * d + d,)
        assert rec[1] == (B if weight is None else weight), rec[1]
        hold("loss", abs(rec[0] - o.loss) / max(1.0, abs(o.loss)), 1e-5)
        hold("C0", used(rec[2:2 + d * d].reshape(d, d), o.C0.numpy(), 2e-5, 2e-5 / B))
        hold("Ctau", used(rec[2 + d * d:2 + 2 * d * d].reshape(d, d), o.Ct.numpy(), 2e-5, 2e-5 / B))
        hold("mu", used(rec[2 + 2 * d * d:], o.mu.numpy(), 2e-5, 1e-4 / B))
    if grads is not None:
        L = len(o.gw)
        for l in range(L):
            wo, bo = offsets[l]
            gw, gb = o.gw[l], o.gb[l]
            hold(f"W{l}", rel_err(grads[wo:wo + gw.size].reshape(gw.shape), gw), 2e-5)
            if l < L - 1 or c.last_act is not None or (c.drops is not None and c.drops[l] > 0):
                hold(f"b{l}", rel_err(grads[bo:bo + gb.size], gb), 2e-5)
            else:
                hold(f"b{l} (exactly 0)", float(np.max(np.abs(grads[bo:bo + gb.size]))) / max(1.0, float(np.max(np.abs(gw)))), 2e-5)
    print(f"WIDE-HEAD {label}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert not bad, f"{label}: " + "; ".join(bad)
    return fig


# ----------------------------------------------------------------------------- the engine's rules, restated
def rides_forward(c):
    """mlp_state.h, next_layer_fusable: the last Linear rides in the product in front of it"""
    return len(c.dims) > 2 and c.dims[-1] <= 8 and c.dims[-2] <= 128 and not (c.drops and c.drops[-1] > 0)


def fuses_backward(c):
    """mlp_heads.hip, head_fusable: loss gradient + last-layer backward in one pass over the hidden activations"""
    if len(c.dims) < 3 or (c.drops and c.drops[-1] > 0):
        return False
    K, D = c.dims[-2], c.dims[-1]
    if D > 8 or K % 4 != 0 or 256 % (K // 4) != 0 or K // 4 > 64:
        return False
    groups = 256 // (K // 4)
    return (2 * D + 2 * D * D) * 8 + (groups * 4 * D + groups * ((D + 1) * K + D)) * 4 <= 60 * 1024


def head_rows_per_block(R, max_batch):
    """mlp_heads.hip, head_plan (with the bound dcv_mlp_create puts on the partial buffers)"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    want = min(4 * ncu, -(-2 * max_batch // 32))
    return max(32, -(-(-(-R // want)) // 32) * 32)


def engine_of(c, max_batch=None, **kw):
    from deep_cartograph_amd import hip

    eng = hip.Mlp("deep_tica", c.dims, acts_of(c), max_batch=max_batch or c.batch, lag=c.lag, tica_reg=c.reg, dropout=c.drops, seed=ENGINE_SEED, **kw)
    push_params(eng, linears_of(model_of(c).nn))
    assert eng.log_width == 2 + 2 * c.dims[-1] ** 2 + c.dims[-1]
    return eng


# ----------------------------------------------------------------------------- one step, every case
@pytest.mark.parametrize("mode", ["split", "native"])
@pytest.mark.parametrize("name", list(CASES))
def test_wide_head_step_matches_float64(name, mode):
    """forward + backward of one batch (the loss head a launch of its own between them) against float64: statistics, record,
    every gradient tensor; in both arithmetic flavours of the matrix products.  Which forms ran is read from hip.gemm_log(),
    which lists the products of the block engine and none of the head's kernels: the forward logs one 'nt' product per Linear,
    less one when the last Linear rode in the epilogue of the one in front (rides_forward); the backward logs one 'tn' (weight
    gradient) per Linear and one 'nn' (input gradient) per Linear above layer 0 -- less one of each when head_backward_kernel
    took the last layer's (fuses_backward), which is what "fused" means below.
    MEASURED on MI355X over the 34 cases, both flavours: worst gradient tensor 5.4e-6 of its largest entry (d6-tanh, last bias;
    without an output activation 2.4e-6), last bias where it is exactly zero 4.7e-7, loss 1.1e-7, statistics at most 0.58 of
    their tolerance (one nearly cancelling entry of sum f_t f_lag^T at 8321 pairs, split flavour; otherwise below 0.12), C0 / Ctau /
    mu at most 0.14.  Per case: DESIGN.md section 2."""
    from deep_cartograph_amd import hip

    c, o = CASES[name], oracle_of(name)
    L = len(c.dims) - 1
    _, kw = index_of(c)
    prev = hip.get_gemm_mode()
    hip.set_gemm_mode(mode)
    try:
        eng = engine_of(c)
        Xd = torch.from_numpy(features(c.n, c.dims[0])).cuda()
        eng.reset_log(2)
        hip.gemm_log_reset()
        eng.forward(Xd, **kw())
        fwd = hip.gemm_log()
        stats = eng.stats_view().cpu().numpy()
        hip.gemm_log_reset()
        eng.backward(Xd, **kw())
        bwd = hip.gemm_log()
        grads = eng.grads_view().cpu().numpy()
        rec = eng.read_log()
        assert eng.last_path() == 0, eng.last_path()
        offsets = list(eng.offsets)
        eng.close()
    finally:
        hip.set_gemm_mode(prev)
    count = lambda log, m: sum(1 for e in log if e.mode == m)
    fused = fuses_backward(c)
    print(f"WIDE-HEAD {name} {mode}: forward products {count(fwd, 'nt')}, backward products {count(bwd, 'tn')} tn + {count(bwd, 'nn')} nn"
          f" -> last Linear {'rides' if rides_forward(c) else 'a product of its own'}, backward {'fused' if fused else 'not fused'}")
    assert all(e.split == (mode == "split") for e in fwd + bwd)
    assert count(fwd, "nt") == L - (1 if rides_forward(c) else 0), fwd
    assert (count(bwd, "tn"), count(bwd, "nn")) == ((L - 1, L - 2) if fused else (L, L - 1)), bwd   # the unfused rule: L and L - 1
    if name == "d6-b16401-gather":   # 32 802 rows over at most 4 x CUs blocks: more than 32 rows each
        assert head_rows_per_block(2 * c.batch, c.batch) > 32
    elif fused:                      # ... every other fused case: 32 rows per block, the last block ragged
        R = c.batch + (c.lag if not c.gather and c.lag <= c.batch and c.drops is None else c.batch)
        assert head_rows_per_block(R, c.batch) == 32 and R % 32 != 0
    assert len(rec) == 1
    compare(c, o, f"{name} {mode}", stats=stats, rec=rec[0], grads=grads, offsets=offsets)


def test_lag_beyond_the_batch_is_two_halves():
    """A contiguous batch whose lag exceeds it (lag 150, 100 pairs) shares no rows: mlp_state.h, shared_rows asks for
    lag <= batch, so lag_offset returns the batch size -- lag_off = 100 as for a gathered batch, 200 rows, and no row of
    tica_dF_kernel / head_backward_kernel is without a term (with shared rows, rows 100 .. 149 would receive neither).  Read from
    the engine: the hidden activations of the step hold 2 B rows, rows [B, 2 B) those of x[row0 + lag ...]."""
    c = CASES["d6-lag150"]
    eng = engine_of(c)
    Xn = features(c.n, c.dims[0])
    Xd = torch.from_numpy(Xn).cuda()
    eng.reset_log(1)
    eng.forward(Xd, row0=ROW0, batch=c.batch)
    H = eng.layer_output(0, 2 * c.batch).cpu().double().numpy()
    eng.close()
    lin = linears_of(model_of(c).nn)[0]
    rows = np.concatenate([np.arange(ROW0, ROW0 + c.batch), np.arange(ROW0 + c.lag, ROW0 + c.lag + c.batch)])
    exp = np.tanh(Xn[rows].astype(np.float64) @ lin.weight.detach().double().numpy().T + lin.bias.detach().double().numpy())
    np.testing.assert_allclose(H, exp, rtol=0, atol=1e-5)


# ----------------------------------------------------------------------------- entry points at d = 6 and d = 12
ENTRY = {6: "d6-b129-lag5", 12: "d12-lag3"}


@pytest.mark.parametrize("mode", ["split", "native"])
@pytest.mark.parametrize("d", [6, 12])
def test_train_step_and_eval_step_match_float64(d, mode):
    """dcv_mlp_train_step (the update fused into the reduction; the gradients stay in grads_view) and dcv_mlp_eval_step (no
    gradient matrices, no backward) on the batch of the step test, each against float64."""
    from deep_cartograph_amd import hip

    name = ENTRY[d]
    c, o = CASES[name], oracle_of(name)
    _, kw = index_of(c)
    prev = hip.get_gemm_mode()
    hip.set_gemm_mode(mode)
    try:
        eng = engine_of(c, lr=1e-3)
        Xd = torch.from_numpy(features(c.n, c.dims[0])).cuda()
        eng.reset_log(2)
        eng.eval_step(Xd, **kw())
        ev_stats = eng.stats_view().cpu().numpy()
        eng.train_step(Xd, **kw())
        grads = eng.grads_view().cpu().numpy()
        stats = eng.stats_view().cpu().numpy()
        rec = eng.read_log()
        assert eng.last_path() == 0
        offsets = list(eng.offsets)
        eng.close()
    finally:
        hip.set_gemm_mode(prev)
    assert len(rec) == 2
    compare(c, o, f"{name} {mode} eval_step", stats=ev_stats, rec=rec[0])
    compare(c, o, f"{name} {mode} train_step", stats=stats, rec=rec[1], grads=grads, offsets=offsets)


def _pass_setup(d, nb):
    c = CASES[ENTRY[d]]
    Xd = torch.from_numpy(features(c.n, c.dims[0])).cuda()
    assert ROW0 + nb * c.batch + c.lag <= c.n
    return c, Xd


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("d", [6, 12])
def test_eval_steps_equal_stepping_bit_for_bit(d, gather):
    """dcv_mlp_eval_steps at more than 4 outputs steps batch by batch behind the call (tica_stats_groupable is false:
    dcv_mlp_last_eval_group says 0): three batches from a log counter of one -- records and the statistics left behind
    bit for bit those of three dcv_mlp_eval_step calls, and the first of them against float64."""
    nb = 3
    c, Xd = _pass_setup(d, nb)
    B = c.batch
    idx = torch.from_numpy(np.random.Generator(np.random.PCG64(9)).permutation(c.n - c.lag)[:nb * B].astype(np.int64)).cuda() if gather else None
    kw = lambda j: dict(idx=idx[j * B:(j + 1) * B]) if gather else dict(row0=ROW0 + j * B, batch=B)
    eng = engine_of(c)
    eng.reset_log(nb + 1)
    eng.eval_step(Xd, **kw(1))
    for j in range(nb):
        eng.eval_step(Xd, **kw(j))
    a, sa = eng.read_log(), eng.stats_view().clone()
    eng.reset_log(nb + 1)
    eng.eval_step(Xd, **kw(1))
    eng.eval_steps(Xd, B, nb, idx=idx, row0=0 if gather else ROW0)
    b, sb = eng.read_log(), eng.stats_view().clone()
    group = int(eng.lib.dcv_mlp_last_eval_group(eng.h))
    assert eng.last_path() == 0
    eng.close()
    assert group == 0, group
    assert a.shape == b.shape == (nb + 1, 2 + 2 * d * d + d) and np.isfinite(a).all()
    assert len(np.unique(a[1:, 0])) == nb and np.array_equal(a[0], a[2])   # the batches differ; the leading record is batch 1's
    assert np.array_equal(a, b)
    assert torch.equal(sa, sb)
    if not gather:   # batch 0 is the step test's batch
        compare(c, oracle_of(ENTRY[d]), f"{ENTRY[d]} eval_steps, first record", stats=None, rec=b[1])


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("d", [6, 12])
def test_train_steps_equal_stepping_bit_for_bit(d, gather):
    """dcv_mlp_train_steps: records, parameters and the step behind them bit for bit those of dcv_mlp_train_step calls."""
    nsteps = 3
    c, Xd = _pass_setup(d, nsteps)
    B = c.batch
    idx = torch.from_numpy(np.random.Generator(np.random.PCG64(9)).permutation(c.n - c.lag)[:nsteps * B].astype(np.int64)).cuda() if gather else None
    kw = lambda j: dict(idx=idx[j * B:(j + 1) * B]) if gather else dict(row0=ROW0 + j * B, batch=B)
    a, b = engine_of(c, lr=1e-3), engine_of(c, lr=1e-3)
    for e in (a, b):
        e.reset_log(2 * nsteps)
    for j in range(nsteps):
        a.train_step(Xd, **kw(j))
    b.train_steps(Xd, B, nsteps, idx=idx, row0=0 if gather else ROW0)
    assert a.last_path() == b.last_path() == 0
    ra, rb = a.read_log(), b.read_log()
    assert ra.shape == (nsteps, a.log_width) and np.isfinite(ra).all() and len(np.unique(ra[:, 0])) == nsteps
    assert np.array_equal(ra, rb)
    assert torch.equal(a.params_view(), b.params_view())
    a.train_step(Xd, **kw(0))
    b.train_step(Xd, **kw(0))
    assert torch.equal(a.params_view(), b.params_view())
    if not gather:
        compare(c, oracle_of(ENTRY[d]), f"{ENTRY[d]} train_steps, first record", rec=rb[0])
    a.close()
    b.close()


# ----------------------------------------------------------------------------- two ranks in one process
class _Replay(_TwoRanksInOneProcess):
    """Two ranks stepped one after the other cannot exchange buffers inside a collective, so the step is replayed: every
    all-reduce call keeps a copy of what its rank brought (`local`) and, where the sum over the ranks is known from the pass
    before (`total`), writes it into the buffer.  Pass 1 learns the summed statistics, pass 2 (statistics summed) the summed
    gradients, pass 3 is the data-parallel step itself: each rank's head runs on the all-reduced statistics, its update on the
    all-reduced gradients."""

    def __init__(self):
        self.local, self.total, self.rank, self.call = {}, {}, 0, 0

    def all_reduce(self, t, op=None, group=None, async_op=False):
        assert op == self.ReduceOp.SUM and not async_op
        key, self.call = self.call, self.call + 1
        self.local[(self.rank, key)] = t.clone()
        if key in self.total:
            t.copy_(self.total[key])


@pytest.mark.parametrize("d,name,lb", [(6, "d6-b129-lag5", 100), (12, "d12-lag3", 150)])
def test_two_rank_step_matches_float64_and_the_one_process_step(d, name, lb):
    """dcv_mlp_dp_step with two ranks (contiguous blocks of `lb` pairs each): the head runs on the all-reduced sums as a launch of
    its own.  The summed gradients and the record against float64 on the full batch of 2 lb pairs (conditioning, float32 oracle
    vs float64: 2.4e-06 at d = 6, 4.8e-06 at d = 12); losses and weights after the update against dcv_mlp_train_step on
    the full batch to the criterion of test_data_parallel_two_ranks_match_single_process (loss rtol 1e-5 / atol 1e-6, weights
    atol 2e-5; the summation order of the float32 partial sums differs)."""
    c = CASES[name]
    Xd = torch.from_numpy(features(c.n, c.dims[0])).cuda()
    full = torch.arange(ROW0, ROW0 + 2 * lb)
    o = run_oracle(c, idx=full)
    ld, o.C0, o.Ct, o.mu = loss_from_the_definition(o.f_t, o.f_l, c.reg)
    assert abs(float(ld) - o.loss) < 1e-10
    rp = _Replay()

    def one_pass():
        out = []
        for r in range(2):
            eng = engine_of(c, max_batch=lb, lr=1e-3)
            eng.reset_log(2)
            rp.rank, rp.call = r, 0
            eng.data_parallel_step(Xd, rp, 2 * lb, row0=ROW0 + r * lb, batch=lb, train=True)
            assert eng.last_path() == 0 and rp.call == 2   # statistics, gradients
            out.append(SimpleNamespace(rec=eng.read_log(), stats=eng.stats_view().cpu().numpy(), lin=eng.get_linears(), offsets=list(eng.offsets),
                                       n_params=eng.n_params))
            eng.close()
        return out

    one_pass()
    own_stats = [rp.local[(r, 0)].clone() for r in range(2)]
    rp.total[0] = own_stats[0] + own_stats[1]
    one_pass()
    assert all(torch.equal(rp.local[(r, 0)], own_stats[r]) for r in range(2))   # a rank's own sums do not depend on the pass
    own_grads = [rp.local[(r, 1)].clone() for r in range(2)]
    rp.total[1] = own_grads[0] + own_grads[1]
    ranks = one_pass()
    assert all(torch.equal(rp.local[(r, 1)], own_grads[r]) for r in range(2))
    assert rp.total[1].numel() == ranks[0].n_params
    for r in range(2):
        assert len(ranks[r].rec) == 1
        compare(c, o, f"{name} two ranks, rank {r}", stats=ranks[r].stats, rec=ranks[r].rec[0], grads=rp.total[1].cpu().numpy(),
                offsets=ranks[r].offsets, weight=2 * lb)
    eng = engine_of(c, max_batch=2 * lb, lr=1e-3)
    eng.reset_log(2)
    eng.train_step(Xd, row0=ROW0, batch=2 * lb)
    one_rec, one_lin = eng.read_log(), eng.get_linears()
    eng.close()
    for r in range(2):
        np.testing.assert_allclose(ranks[r].rec[0, 0], one_rec[0, 0], rtol=1e-5, atol=1e-6)
        for (w, _), (w1, _) in zip(ranks[r].lin, one_lin):
            np.testing.assert_allclose(w, w1, atol=2e-5)


# ----------------------------------------------------------------------------- degenerate head
@pytest.mark.parametrize("d", [3, 6, 9])
def test_degenerate_head_reports_nan_at_every_width(d):
    """tica_reg = 0 and a last Linear of zeros (weight and bias: the outputs are exactly 0, so C0 is exactly 0 and the first
    Cholesky pivot is not positive): the wave form (d = 3), tica_grad_kernel<6> and <0> (d = 9) each carry an `ok` flag of their
    own and must all report the loss as NaN, in an evaluation step and in a training step.  Nothing else is asserted."""
    c = _case([40, 16, d], 100)
    c.reg = 0.0
    eng = engine_of(c)
    lins = [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in linears_of(model_of(c).nn)]
    lins[-1] = (np.zeros_like(lins[-1][0]), np.zeros_like(lins[-1][1]))
    eng.set_linears(lins)
    Xd = torch.from_numpy(features(c.n, c.dims[0])).cuda()
    eng.reset_log(2)
    eng.eval_step(Xd, row0=ROW0, batch=c.batch)
    eng.train_step(Xd, row0=ROW0, batch=c.batch)
    rec = eng.read_log()
    eng.close()
    assert rec.shape == (2, 2 + 2 * d * d + d)
    assert np.isnan(rec[0, 0]) and np.isnan(rec[1, 0]), rec[:, 0]
    assert np.all(rec[:, 1] == c.batch)


if __name__ == "__main__":   # the conditioning table, on the CPU
    for name, c in CASES.items():
        dev, cond = float32_oracle_deviation(c)
        oracle_of(name)   # the 1e-10 agreement of the two float64 losses
        print(f"{name:20s} {str(c.dims):16s} batch {c.batch:5d} lag {c.lag:3d}: float32 oracle vs float64 {dev:.1e}, cond(C0) {cond:.0f}"
              + ("" if dev < 1e-5 else "   NOT USABLE"))
    for name, lb in (("d6-b129-lag5", 100), ("d12-lag3", 150)):
        dev, cond = float32_oracle_deviation(CASES[name], torch.arange(ROW0, ROW0 + 2 * lb))
        print(f"{name:20s} two ranks, full batch {2 * lb}: float32 oracle vs float64 {dev:.1e}, cond(C0) {cond:.0f}")
