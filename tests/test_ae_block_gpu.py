"""The autoencoder and the VAE on the block engine (run_forward / backward_impl in csrc/mlp.hip, the products of gemm_kernels.h,
pair.hip, ride.hip, the reductions of mlp_opt.hip, the loss kernels of mlp_heads.hip) against float64: tests/ae_block_oracle.py
for the autoencoder, tests/vae_oracle.py for the VAE.  The case tables live in tests/ae_block_oracle.py and are checked without
a GPU by tests/test_ae_block_oracle_cpu.py (oracle against autograd, conditioning of every case, the arithmetic of the tables).

Bounds (tests/test_snet_dt_gpu.py, tests/test_vae_step_gpu.py): every gradient tensor within 2e-5 of the oracle tensor's largest
entry; loss / reconstruction / KL records within 1e-5 relative; the record's weight equal to the batch; z at rtol 1e-5 and
atol Z_ATOL_W.  Leaky-ReLU networks are held to the kink-aware criterion of check_step_against_float64 (tests/test_mlp_gpu.py).

Every case asserts that the block engine ran (last_path() == 0) and, from hip.gemm_log() / last_ride() / last_reduce(), that the
launch forms it is listed for were the ones launched; it prints the plan and its measured deviations first."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests import ae_block_oracle as ab
from tests import test_vae_step_gpu as vs
from tests import vae_oracle as vo
from tests.test_mlp_gpu import _has, _ncu, assert_within, rel_err

pytestmark = pytest.mark.gpu

MODES = ["split", "native"]
BIG, HALF, QUARTER = dict(tm=128, tn=128), dict(tm=64, tn=128), dict(tm=64, tn=64)
cut = lambda t: t >= 2


@contextlib.contextmanager
def gemm_mode(mode):
    from deep_cartograph_amd import hip

    prev = hip.get_gemm_mode()
    hip.set_gemm_mode(mode)
    try:
        yield
    finally:
        hip.set_gemm_mode(prev)


def _engine(c, max_batch, **opt):
    from deep_cartograph_amd import hip

    opt.setdefault("lr", 1e-3)
    eng = hip.Mlp("ae", c["dims"], c["acts"], max_batch=max_batch, latent_layer=c["latent"], **opt)
    eng.set_linears([(w.numpy(), b.numpy()) for w, b in zip(c["Ws"], c["bs"])])
    eng.set_feature_range(c["range"])
    eng.reset_log(8)
    return eng


def _kw(rows, form):
    if form == "idx":
        return dict(idx=torch.from_numpy(rows).cuda())
    return dict(row0=int(rows[0]), batch=len(rows))


def _plan(log):
    return [tuple(e) for e in log]


def _nt(log):
    return sum(1 for e in log if e.mode == "nt")


def _grad_deviations(g, offsets, o):
    dev = {}
    for l, (gw, gb) in enumerate(zip(o["gw"], o["gb"])):
        wo, bo = offsets[l]
        dev[f"layer {l} weight"] = rel_err(g[wo:wo + gw.size].reshape(gw.shape), gw)
        dev[f"layer {l} bias"] = rel_err(g[bo:bo + gb.size], gb)
    return dev


SGD_LR = 0.5   # large enough for the update to stand clear of the float32 rounding of the parameters


def check_ae_step(c, rows, form, mode, label, *, train_step=False, sgd=False):
    """One step of the block engine on `rows` of the case as forward + backward (and once more as a one-GPU training step) against
    ae_step in float64, kink-aware: (i) the engine's slope decisions (sign of the activations it stored) differ from the float64
    ones only where the float64 pre-activation is within 1e-5 of zero; (ii) with the engine's slope pattern held fixed, the loss
    record and every weight and bias gradient agree to REC_TOL / GRAD_TOL.  sgd: plain SGD, and the parameters after the training
    step equal parameters - lr * float64 gradient to lr * GRAD_TOL of the gradient tensor's largest entry plus two float32
    roundings of the result.  Returns the plans launched and last_ride() / last_reduce() of each form."""
    from deep_cartograph_amd import hip

    R, kinks = len(rows), ab.kink_layers(c["acts"])
    kw = _kw(rows, form)
    out, g_step, rec_step, p0, p1 = {}, None, None, None, None
    with gemm_mode(mode):
        eng = _engine(c, R, **(dict(optimizer="SGD", momentum=0.0, lr=SGD_LR) if sgd else {}))
        Xd = torch.from_numpy(c["Xn"]).cuda()
        hip.gemm_log_reset()
        eng.forward(Xd, **kw)
        H = {l: eng.layer_output(l, R).cpu().numpy() for l in kinks}
        eng.backward(Xd, **kw)
        g = eng.grads_view().cpu().numpy()
        rec = eng.read_log()[0]
        assert eng.last_path() == 0, eng.last_path()
        out.update(step=hip.gemm_log(), step_ride=eng.last_ride(), step_reduce=eng.last_reduce())
        if train_step:
            p0 = eng.params_view().cpu().numpy().astype(np.float64)
            hip.gemm_log_reset()
            eng.train_step(Xd, **kw)
            g_step = eng.grads_view().cpu().numpy()
            rec_step = eng.read_log()[1]
            p1 = eng.params_view().cpu().numpy().astype(np.float64)
            assert eng.last_path() == 0, eng.last_path()
            out.update(train_step=hip.gemm_log(), ride=eng.last_ride(), reduce=eng.last_reduce())
        offsets = list(eng.offsets)
        eng.close()
    print(f"{label} {mode}: product plans {_plan(out['step'])}, reduction kind {out['step_reduce']}"
          + (f"; training step {_plan(out['train_step'])}, ride blocks {out['ride']}, reduction kind {out['reduce']}" if train_step else ""))
    assert all(e.split == (mode == "split") for e in out["step"] + out.get("train_step", [])), out
    x = torch.from_numpy(c["Xn"])[torch.from_numpy(rows)]
    patterns = {l: torch.from_numpy(H[l] > 0) for l in kinks}
    o = ab.ae_step(x, c["Ws"], c["bs"], c["acts"], c["range"], patterns)
    flips = {}
    for l in kinks:
        differ = patterns[l] != o["own"][l]
        flips[l] = int(differ.sum())
        if differ.any():   # (i): only units within float32 rounding of the kink
            assert float(o["z"][l].abs()[differ].max()) < ab.KINK, f"layer {l}: slope decision differs away from the kink"
    for what, gv, rc in (("", g, rec), (" (training step)", g_step, rec_step)):
        if gv is None:
            continue
        ldev = abs(rc[0] - o["loss"]) / abs(o["loss"])
        dev = _grad_deviations(gv, offsets, o)
        print(f"{label} {mode}{what}: loss deviation {ldev:.2e}; slope decisions differing from float64 (all within 1e-5 of the kink): {flips}; "
              f"worst gradient deviation {max(dev.values()):.2e}: { {k: '%.2e' % v for k, v in dev.items()} }")
        assert rc[1] == R, f"record weight {rc[1]} != {R}"
        assert ldev < ab.REC_TOL, f"loss record{what}: {rc[0]!r} vs {o['loss']!r} ({ldev:.2e})"
        for k, v in dev.items():
            assert v < ab.GRAD_TOL, f"{k}{what}: {v:.2e}"
    if sgd:
        worst = 0.0
        for l, (gw, gb) in enumerate(zip(o["gw"], o["gb"])):
            for off, gt in ((offsets[l][0], gw), (offsets[l][1], gb)):
                want = p0[off:off + gt.size] - SGD_LR * gt.ravel()
                err = np.abs(p1[off:off + gt.size] - want)
                bound = SGD_LR * ab.GRAD_TOL * np.max(np.abs(gt)) + 2.0 ** -23 * np.abs(want)
                worst = max(worst, float(np.max(err / bound)))
                assert np.all(err <= bound), f"layer {l}: parameters after the SGD step, worst {err.max():.2e}"
        print(f"{label} {mode}: parameters after the SGD step: worst error / bound {worst:.3g}")
    return out


@functools.lru_cache(maxsize=2)   # the two flavours of a case run back to back
def _step_case(name):
    k = ab.step_cases(_ncu())[name]
    c = ab.ae_case(k["dims"], k["acts"], k["latent"], ab.matrix_rows(k["rows"]), k["seed"])
    return k, c, ab.rows_of(c, k["rows"], k["form"], k["seed"])


# ------------------------------------------------------------------------------------------------ A: one step against float64
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["A1", "A2", "A3", "A4a", "A4b", "A5"])
def test_ae_step_on_the_block_engine_matches_float64(name, mode):
    """Group A (ae_block_oracle.step_cases: what each case reaches): 512-256-128-2-128-256-512 at the contract shape (A1), gathered
    (A2), leaky-ReLU (A3), at the first row counts of ragged 128 x 128 tiles (A4a, A4b), and 320-128-4-128-320 past 32 768 rows
    (A5: the 16-wave reduction, the SGD update); forward + backward, and where listed a training step.
    MEASURED on MI355X (256 CUs), worst gradient tensor / loss, split | native: A1 9.2e-7 / 1.9e-9 | 8.2e-7 / 9.7e-11 (the training
    step the same to every digit printed); A2 6.3e-7 / 3.2e-9 | 2.0e-7 / 1.4e-10; A3 1.7e-6 / 1.3e-9 | 1.5e-6 / 2.0e-10, one slope
    decision differing from float64 in each of layers 0 and 1, both within 1e-5 of the kink; A4a 9.2e-7 / 2.2e-9 | 3.2e-7 / 2.1e-10;
    A4b 3.6e-7 / 1.9e-9 | 2.7e-7 / 6.6e-11; A5 3.1e-7 / 3.5e-9 | 1.4e-7 / 2.0e-10, parameters after the SGD step 0.018 of their bound.
    float32 torch-CPU oracle against float64 (slope pattern fixed), worst gradient tensor / loss: A1 7.9e-7 / 5.8e-8, A2 2.3e-7 /
    6.9e-8, A3 9.1e-7 / 5.1e-8, A4a 1.0e-6 / 9.3e-8, A4b 2.5e-7 / 3.8e-8, A5 1.8e-7 / 9.6e-10 (the last three run once by hand: the
    CPU test stops at 8 300 rows).  The engine's loss is closer than the float32 oracle's because it sums the squares in float64."""
    k, c, rows = _step_case(name)
    out = check_ae_step(c, rows, k["form"], mode, f"{name} ({k['rows']} rows)", train_step=k["train_step"], sgd=k["sgd"])
    log, n = out["step"], _ncu()
    gathered = k["form"] == "idx"
    assert out["step_ride"] == 0
    if name in ("A1", "A2", "A3"):
        assert _nt(log) == 5, log   # six Linears: the latent one rode in the epilogue of the 128-wide layer before it (head4)
        assert log[0].mode == "nt" and (log[0].tm, log[0].tn) == (64, 64) and log[0].vec and log[0].gather == gathered, log
        assert (log[0].tail_split >= 2) == (name != "A2"), log   # the ragged row tile of 32 n + 10 rows is cut along the contraction
        assert _has(log, form="single", mode="nt", vec=False, gather=True), log   # first decoder Linear: K = 2, scalar loaders
        assert _has(log, form="single", mode="nt", vec=True, **HALF), log           # last layer, N = F = 512
        # last layer (N = F) and layer 1: weight + input gradient in one launch; layer 4's input gradient (N = 128) takes 32 x 128
        # tiles, outside the pair forms: launched apart
        assert sum(1 for e in log if e.form == "pair" and e.mode == "tn" and (e.tm, e.tn) == (64, 64) and e.splits >= 2) == 2, log
        assert sum(1 for e in log if e.form == "pair" and e.mode == "nn" and (e.tm, e.tn) == (64, 64)) == 2, log
        assert _has(log, form="single", mode="nn", tm=32, tn=128), log
        assert _has(log, form="single", mode="tn", vec=True, gather=gathered, splits=cut, **QUARTER), log   # layer-0 weight gradient
        assert out["step_reduce"] == 1
    if name == "A1":
        step = out["train_step"]
        assert out["ride"] > 0 and out["reduce"] == 1, out
        assert _has(step, form="ride", mode="tn", splits=cut, **QUARTER) and sum(1 for e in step if e.form == "ride") == 1, step
        # the same products as forward + backward, the layer-0 weight gradient now inside the ride launch
        assert [(e.mode, e.tm, e.tn, e.splits) for e in step] == [(e.mode, e.tm, e.tn, e.splits) for e in log] and step[-1].form == "ride", step
    if name == "A2":
        step = out["train_step"]
        assert out["ride"] == 0 and not _has(step, form="ride") and out["reduce"] == 1, out
        assert _has(step, form="single", mode="tn", vec=True, gather=True, splits=cut, **QUARTER), step
    if name == "A4a":
        last_fwd = [e for e in log if e.mode == "nt"][-1]
        assert (last_fwd.form, last_fwd.tm, last_fwd.tn, last_fwd.vec) == ("single", 128, 128, True), log
        # last layer: 128 x 128 weight gradient, 64 x 64 input gradient -- no pair form, two launches; layer 1: 64 x 64 / 64 x 64
        assert _has(log, form="single", mode="tn", splits=cut, **BIG) and _has(log, form="single", mode="nn", **QUARTER), log
        assert _has(log, form="pair", mode="tn", **QUARTER) and _has(log, form="pair", mode="nn", **QUARTER), log
        assert not _has(log, form="pair", **BIG), log
    if name == "A4b":
        assert _has(log, form="pair", mode="tn", splits=cut, **BIG) and _has(log, form="pair", mode="nn", **BIG), log
        assert _has(log, form="pair", mode="tn", **QUARTER) and _has(log, form="pair", mode="nn", **HALF), log
        # layer 1: 64 x 64 weight gradient, 128 x 128 input gradient, apart
        assert _has(log, form="single", mode="nn", vec=True, **BIG) and _has(log, form="single", mode="tn", vec=True, **QUARTER), log
    if name == "A5":
        assert ab.bias_partials(k["rows"]) > 1024
        assert out["step_reduce"] == 3 and out["reduce"] == 3 and out["ride"] == 0 and not _has(out["train_step"], form="ride"), out


# ------------------------------------------------------------------------------------------------ B: the narrow middle
@pytest.mark.parametrize("name,dims,acts,latent,form,mode,rides,vec", ab.narrow_cases(), ids=[k[0] for k in ab.narrow_cases()])
def test_narrow_latent_layer_matches_float64(name, dims, acts, latent, form, mode, rides, vec):
    """Group B: 260-128-d-128-260 (and 260-256-3-256-260) at 777 rows.  Forward: the latent Linear in the epilogue of the layer before
    it (d <= 4: gemm_nt_head4, d <= 8: gemm_nt_head8, else and behind a 256-wide layer on its own), the first decoder Linear with
    K = d; backward: weight / input gradients with N = d and with M = d / K = d.
    MEASURED on MI355X (256 CUs): at most 6.5e-7 per gradient tensor (d = 3, split), 6.8e-9 on the loss (d = 2, split).
    float32 torch-CPU oracle against float64: at most 7.6e-7 per gradient tensor, 1.1e-7 on the loss."""
    c = ab.ae_case(dims, acts, latent, ab.matrix_rows(ab.NARROW_ROWS), 12)
    rows = ab.rows_of(c, ab.NARROW_ROWS, form, 12)
    out = check_ae_step(c, rows, form, mode, f"narrow {name} {form}")
    log = out["step"]
    assert _nt(log) == (3 if rides else 4), log   # four Linears, less the latent one when it rode (head4 / head8 by its width)
    first_dec = [e for e in log if e.mode == "nt"][-2]   # K = d: 16-byte loaders only for d % 4 == 0
    assert first_dec.vec == vec and first_dec.form == "single", log
    if not rides:
        assert _has(log, form="single", mode="nt", tn=32), log   # the latent Linear as a narrow product of its own
    assert log[0].mode == "nt" and log[0].gather == (form == "idx") and log[0].vec, log
    nn = [e for e in log if e.mode == "nn"]   # input gradients of the output Linear, the first decoder Linear (N = d), the latent Linear (K = d)
    assert len(nn) == 3 and nn[1].tn == 32 and (nn[2].tm, nn[2].tn, nn[2].vec) == (32, 128, vec), log
    assert _has(log, mode="tn", tn=32) and _has(log, mode="tn", tm=32), log   # weight gradients with N = d and with M = d


# ------------------------------------------------------------------------------------------------ C: loss and seed gradient
def _loss_case(rows):
    c = ab.ae_case(ab.LOSS_DIMS, ab._acts(ab.LOSS_DIMS, "tanh", 2), 2, ab.matrix_rows(rows), 13)
    return c, ab.rows_of(c, rows, "row0", 13)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", range(len(ab.loss_rows(256))))
def test_loss_record_ticketed_and_unticketed(which, mode):
    """Group C: 512-8-2-8-512 at the row counts of ae_block_oracle.loss_rows (the kSseRows clamp, both sides of every regime edge of
    ae_sse's block plan, the first second trip of ae_dY_kernel's grid-stride loop).  eval_step (ticketed sum, record written by
    ae_sse_kernel's last block) and forward + backward(train=False) (partials summed by sum_partials_kernel, record by
    ae_log_kernel) must leave the same record bit for bit, within REC_TOL of float64; [SSE] in stats_view() likewise.
    MEASURED on MI355X (256 CUs): the two records equal at every row count; loss and SSE at most 1.3e-8 from float64 (1 row,
    native), 4.9e-9 (split, 1 025 rows); whole steps at 17 and 2 049 rows: gradients at most 4.5e-7, loss 4.2e-9.
    float32 torch-CPU oracle against float64: loss at most 1.2e-7, gradients at most 5.2e-7."""
    from deep_cartograph_amd import hip

    R, whole = ab.loss_rows(_ncu())[which]
    c, rows = _loss_case(R)
    kw = _kw(rows, "row0")
    with gemm_mode(mode):
        eng = _engine(c, R)
        Xd = torch.from_numpy(c["Xn"]).cuda()
        hip.gemm_log_reset()
        eng.eval_step(Xd, **kw)
        assert eng.last_path() == 0
        log = hip.gemm_log()
        sse_e = float(eng.stats_view().cpu().numpy()[0])
        eng.forward(Xd, **kw)
        eng.backward(Xd, train=False, **kw)
        assert eng.last_path() == 0
        sse_f = float(eng.stats_view().cpu().numpy()[0])
        recs = eng.read_log()
        eng.close()
    o = ab.ae_step(torch.from_numpy(c["Xn"])[torch.from_numpy(rows)], c["Ws"], c["bs"], c["acts"], c["range"])
    dev = abs(recs[0][0] - o["loss"]) / o["loss"]
    print(f"loss network, {R} rows, {mode}: ae_sse plan (regime, rows per block, blocks, clamped) {ab.ae_sse_plan(R, ab.LOSS_DIMS[0])}, ae_dY trips "
          f"{ab.dY_trips(R, ab.LOSS_DIMS[0], _ncu())}; products {_plan(log)}; record deviation from float64 {dev:.2e}, SSE {abs(sse_e - o['sse']) / o['sse']:.2e}")
    assert recs.shape[0] == 2 and np.array_equal(recs[0], recs[1]), (recs[0], recs[1])
    assert sse_e == sse_f
    assert recs[0][1] == R
    assert dev < ab.REC_TOL and abs(sse_e - o["sse"]) / o["sse"] < ab.REC_TOL
    assert _nt(log) == 3 and all(e.split == (mode == "split") for e in log), log   # the latent Linear rode behind the 8-wide layer
    if whole:   # the seed gradient shows in the last layer's gradients (and in every one below)
        check_ae_step(c, rows, "row0", mode, f"loss network, {R} rows, whole step")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows", ab.COLSUM_ROWS)
@pytest.mark.parametrize("dims,out_act", ab.COLSUM_NETS, ids=["320", "301-tanh"])
def test_wide_last_layer_bias_gradient(dims, out_act, rows, mode):
    """Group C, colsum_kernel over a wide last layer: 320 columns (a second, ragged column pass) and 301 columns (the scalar edge;
    tanh on the output Linear, so that act' in ae_dY_kernel is not the identity) at 77 and 1 000 gathered rows: a whole step.
    MEASURED on MI355X (256 CUs): at most 8.9e-7 per gradient tensor (320 columns, 77 rows, native), 3.0e-9 on the loss.
    float32 torch-CPU oracle against float64: at most 5.7e-7 per gradient tensor, 6.5e-8 on the loss."""
    c = ab.ae_case(dims, ab._acts(dims, "tanh", 2, None, out_act), 2, ab.matrix_rows(rows), 14)
    out = check_ae_step(c, ab.rows_of(c, rows, "idx", 14), "idx", mode, f"{dims} {rows} rows")
    log = out["step"]
    assert _nt(log) == 3 and log[0].gather and log[0].vec == (dims[0] % 4 == 0), log   # 301 features: scalar loaders on layer 0
    assert _has(log, mode="nt", vec=False, gather=True), log   # first decoder Linear, K = 3


# ------------------------------------------------------------------------------------------------ D: VAE behind wide layers
@functools.lru_cache(maxsize=2)   # the two flavours of a case run back to back
def _vae_case(name, rows, form, beta):
    _, dims, latent, d, rides = next(k for k in ab.VAE_NETS if k[0] == name)
    acts = ab._acts(dims, "tanh", latent)
    n, row0 = rows + 13, 3
    c = vo.case(dims, acts, latent, n, 1000 * d + len(dims))
    r = vs._rows(form, n, rows, np.random.Generator(np.random.PCG64(d * 1000 + rows)), row0)
    c.update(rows=r, form=form, row0=row0, batch=rows, beta=beta, e0=0, rides=rides,
             o=vo.step(c["lins"], acts, latent, c["Xn"][r], c["eps"][:rows], c["range"], beta))
    return c


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", range(6))
def test_vae_step_behind_wide_layers_matches_float64_oracle(which, mode):
    """Group D (ae_block_oracle.VAE_NETS, vae_cases): vae_sample_kernel, latent_backward_layer and vae_sample_backward_kernel between
    products that are not narrow, by the method of test_layer_path_vae_step_matches_float64_oracle (tests/test_vae_step_gpu.py:
    _layer_step; z at atol Z_ATOL_W: the heads read 128- and 256-term float32 sums, as network W's 300-term ones).  Contiguous rows
    as a training step (which rides), gathered rows as forward + backward; then one eval_step record on a fresh engine.
    MEASURED on MI355X (256 CUs): gradients at most 8.7e-7 (heads on their own, gathered, split), records and sums 1.6e-7, eval_step
    records 1.6e-7; z beyond rtol 1e-5 by at most 2.2e-6 (heads on their own, native; 8.4e-7 behind the 128-wide layer) of the
    4.9e-6 allowed.
    float32 torch-CPU run of the same steps against the oracle: gradients at most 4.5e-7, loss / reconstruction / KL 1.4e-7, z beyond
    rtol 1e-5 by at most 1.9e-6 (heads on their own), 9.1e-7 behind the 128-wide layer."""
    from deep_cartograph_amd import hip

    name, rows, form, beta = ab.vae_cases(_ncu())[which]
    c = _vae_case(name, rows, form, beta)
    L, d = len(c["dims"]) - 1, c["d"]
    what = f"vae {name} d={d} {rows} rows {form} beta={beta} {mode}"
    with gemm_mode(mode):
        hip.gemm_log_reset()
        vs._layer_step(c, form == "row0", what, vs.Z_ATOL_W)
        log = hip.gemm_log()
        eng = vs._engine(c, rows)
        eng.eval_step(torch.from_numpy(c["Xn"]).cuda(), **vs._kw(c))
        assert eng.last_path() == 0 and eng.noise_position() == rows
        wr = vs._check_record(eng.read_log()[0], c["o"], rows, beta, what + " eval_step")
        eng.close()
    print(f"{what}: product plans {_plan(log)}; eval_step record deviation {wr:.2e}")
    assert all(e.split == (mode == "split") for e in log), log
    assert _nt(log) == (L - 1 if c["rides"] else L), log   # the heads (2 d columns) in the epilogue of the 128-wide layer, or alone
    first_dec = [e for e in log if e.mode == "nt"][c["latent"] - (1 if c["rides"] else 0)]
    assert first_dec.vec == (d % 4 == 0) and first_dec.form == "single", log   # reads z: K = d
    assert _has(log, form="single", mode="tn", tn=32) and _has(log, form="single", mode="nn", tn=32), log   # latent_backward_layer: alone, N = d
    assert _has(log, form="pair", mode="tn") and _has(log, form="pair", mode="nn"), log
    assert log[0].gather == (form == "idx") and (log[0].tail_split >= 2) == (form == "row0"), log
    assert _has(log, form="ride", mode="tn", splits=cut) == (form == "row0"), log


# ------------------------------------------------------------------------------------------------ E: inference
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["A1", "narrow"])
def test_inference_on_block_engines_matches_float64(which, mode):
    """Group E: infer() over every row of the matrix (more than the engine's row capacity: chunk seams) on A1's engine and a Group B
    engine (d = 5: the encoder ends on the fused head), contiguous and through a view with stride(0) > F, after one step.  Every
    element against the float64 encoder within the element-wise float32 product bound of forward_layers_against_float64, carried
    through the layers (ae_block_oracle.encoder_with_bound); want_minmax exactly the extrema of the returned rows; dropout_step(),
    the log and the parameters untouched.
    MEASURED on MI355X (256 CUs): no element beyond the bound; worst error 0.0012 of it on A1's encoder, 0.011 on the Group B one,
    in both flavours, the strided view the same.  (The bound is loose for a whole encoder: each layer adds its 1e-6 absolute term
    times the next layers' |W|; what it catches is a lost product term or a wrong row at a chunk seam, not a rounding mode.)"""
    if which == "A1":
        k, c, rows = _step_case("A1")
        form = k["form"]
    else:
        dims = [260, 128, 5, 128, 260]
        c = ab.ae_case(dims, ab._acts(dims, "tanh", 2), 2, ab.matrix_rows(ab.NARROW_ROWS), 12)
        rows, form = ab.rows_of(c, ab.NARROW_ROWS, "row0", 12), "row0"
    F, lat = c["dims"][0], c["latent"]
    ref, bound = ab.encoder_with_bound(c["Xn"], c["Ws"], c["bs"], c["acts"], lat)
    with gemm_mode(mode):
        eng = _engine(c, len(rows))
        Xd = torch.from_numpy(c["Xn"]).cuda()
        assert Xd.shape[0] > eng.rows_cap
        eng.forward(Xd, **_kw(rows, form))
        eng.backward(Xd, **_kw(rows, form))
        before = (eng.dropout_step(), eng.read_log().copy(), eng.params_view().clone())
        wide = torch.zeros(Xd.shape[0], F + 4, device="cuda")
        wide[:, :F] = Xd
        view = wide[:, :F]
        assert view.stride(0) > F
        for what, X in (("contiguous", Xd), ("strided view", view)):
            out, mm = eng.infer(X, want_minmax=True)
            assert out.shape == (Xd.shape[0], c["dims"][lat])
            assert torch.equal(mm[0], out.min(dim=0).values) and torch.equal(mm[1], out.max(dim=0).values), f"{what}: min / max"
            assert_within(f"infer {which} {mode} {what}", out.cpu().numpy().astype(np.float64), ref, bound)
        assert eng.dropout_step() == before[0] and np.array_equal(eng.read_log(), before[1]) and torch.equal(eng.params_view(), before[2])
        eng.close()
