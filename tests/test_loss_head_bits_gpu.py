"""The loss head of the MLP engine -- batch statistics, the d x d Deep-TICA head, the loss gradient and the fused backward of
a narrow last layer (csrc/mlp_heads.hip), the tails of the fused small-network kernels (snet.hip, snet_dt.hip) and the pieces
they share (loss_head.h) -- bit for bit against digests recorded on the MI355X (tests/golden/loss_head_bits.json, written by
tests/golden/make_golden_loss_head_bits.py from the commit named in that file).  The float64 oracles of test_mlp_gpu.py,
test_snet_dt_gpu.py and test_vae_gpu.py allow rounding-level drift; a change that only moves code must allow none.

The switches that choose the engine are read once per process, so each environment is one test that starts one fresh child
(this file run as a script) which prints the digests of its cases as one JSON object.  Per case two digests:
  records  every column of read_log() and, after every step, stats_view(): independent of the CU count by construction (the
           rows per statistics block and the tile counts follow from the batch alone);
  params   get_linears() after the case's steps: these can depend on the launch plans of the block engine, so the case's
           gemm_log() is stored beside the digest and compared first -- another plan fails with the difference, never skips.
last_path() after every step is stored and compared too, so that a case cannot quietly move to another path.

Every case runs: two train_steps; one forward + backward pair (the unfused head: loss_record's own launch); one eval_step;
eval_steps with 3 batches from a non-zero log counter; a one-rank data_parallel_step for training and for evaluation.  The
shapes are the smallest that reach each copy of the arithmetic (named per case below).  Two shapes differ from the round
numbers one would first write down:
  * the fused Deep-TICA forward has 512 threads, so its last arriver sums in G = 512 / 40 = 12 groups and the eight-in-flight
    loop runs a second iteration from 8 * 12 + 1 = 97 tiles on: batch 777 at 16-row tiles (98 tiles), not ~400 pairs;
  * the 66-batch validation pass runs for the autoencoder [33, 12, 3, 12, 33] (second-ticket counter move across two
    launches) and for the Deep-TICA network [33, 12, 3].
Run on the GPU box: python -m pytest tests -m gpu"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "loss_head_bits.json")

ENVIRONMENTS = {
    "default": {},
    "no_snet": {"DCV_NO_SNET": "1"},
    "no_snet_no_head_fusion": {"DCV_NO_SNET": "1", "DCV_NO_HEAD_FUSION": "1"},
}


def dt(name, dims, batch, gather, what, **kw):
    return dict(name=name, model="deep_tica", dims=dims, batch=batch, gather=gather, what=what, **kw)


def ae(name, dims, batch, what, **kw):
    return dict(name=name, model="ae", dims=dims, batch=batch, gather=True, what=what, **kw)


def vae(name, batch, what, **kw):
    from tests.test_vae_gpu import REF_DIMS

    return dict(name=name, model="vae", dims=list(REF_DIMS), batch=batch, gather=True, what=what, **kw)


def cases_of(env):
    """contiguous rows share the rows of the two halves (lag_off = lag); a gathered batch has them apart (lag_off = B)"""
    out = []
    if env == "default":   # the fused small-network kernels
        for D in (1, 2, 3, 4):
            for gather in (False, True):
                out.append(dt(f"dt-54-16-8-{D}-b131-{'gather' if gather else 'rows'}", [54, 16, 8, D], 131, gather,
                              "snet_dt_fwd / bwd_kernel<16>, the wave head at D, a ragged last tile", path=2))
        out.append(dt("dt-54-16-8-4-b777-rows", [54, 16, 8, 4], 777, False, "98 tiles > 8 * (512 / 40): second eight-in-flight iteration", path=2,
                      tile_rows=16, tiles_over=8 * (512 // 40)))
        out.append(ae("ae-54-16-2-16-54-b77", [54, 16, 2, 16, 54], 77, "snet_ae_kernel<16, false> tail, ae_log_kernel behind the one-rank exchange", path=1))
        out.append(vae("vae-ref-b77", 77, "snet_ae_kernel<16, true> tail, its batched pass behind the advance kernel", path=1))
        out.append(ae("ae-33-12-3-12-33-b77-nb66", [33, 12, 3, 12, 33], 77, "66 batches: two launches, the second ticket moves the counter", path=1, nb_long=66))
        out.append(dt("dt-33-12-3-b77-nb66", [33, 12, 3], 77, True, "66 batches of the fused Deep-TICA forward: two launches", path=2, nb_long=66))
    elif env == "no_snet":   # the layer-by-layer engine
        for D in (1, 2, 3, 4):
            for gather in (False, True):
                out.append(dt(f"dt-54-16-8-{D}-b131-{'gather' if gather else 'rows'}", [54, 16, 8, D], 131, gather,
                              "tica_stats_rows_kernel<D> + fused head, tica_stats_rows_group_kernel<D>, head_backward_kernel<D>, tica_grad_wave_kernel<D>"))
        out.append(dt("dt-54-16-8-4-b12545-gather", [54, 16, 8, 4], 12545, True, "50 statistics blocks > 48 = 8 * (256 / 40)"))
        for D in (5, 6, 7, 8):
            out.append(dt(f"dt-40-16-{D}-b100-rows", [40, 16, D], 100, False, "tica_stats_kernel, tica_grad_kernel<5 | 6 | 0>, head_backward_kernel<D>"))
        for D in (9, 16):
            out.append(dt(f"dt-40-16-{D}-b100-gather", [40, 16, D], 100, True, "tica_grad_kernel<0>, tica_dF_kernel: the head is not fusable"))
        out.append(dt("dt-40-5-b100-rows", [40, 5], 100, False, "a single Linear: tica_dF_kernel"))
        out.append(dt("dt-40-15-3-b100-gather", [40, 15, 3], 100, True, "K = 15 is no multiple of 4: tica_dF_kernel"))
        out.append(dt("dt-54-16-8-4-b131-drop-prev", [54, 16, 8, 4], 131, False, "drop_prev of head_backward_kernel", dropout=[0.0, 0.25, 0.0], seed=11))
        out.append(dt("dt-54-16-8-4-b131-drop-out", [54, 16, 8, 4], 131, True, "the output mask of tica_dF_kernel", dropout=[0.0, 0.0, 0.25], seed=11))
        out.append(ae("ae-128-64-2-64-128-b2100", [128, 64, 2, 64, 128], 2100, "66 squared-error blocks: the one-wave sum loops twice", sse_blocks=66))
        out.append(ae("ae-54-16-2-16-54-b77", [54, 16, 2, 16, 54], 77, "ae_sse_kernel with its record, ae_log_kernel, launch_sum_partials"))
        out.append(vae("vae-ref-b77", 77, "ae_sse_kernel's KL sum, the two launch_sum_partials calls, the VAE record of ae_log_kernel"))
    else:
        out.append(dt("dt-54-16-8-4-b131-rows", [54, 16, 8, 4], 131, False, "tica_dF_kernel at d <= 4"))
        out.append(ae("ae-54-16-2-16-54-b77", [54, 16, 2, 16, 54], 77, "the unfused engine's autoencoder head"))
    for c in out:
        c.setdefault("path", 0)
    return out


_inputs = {}


def inputs(n, F):
    """normalised AR features (seed 17), computed once per shape"""
    from tests.test_mlp_gpu import ar_features, normalized

    if (n, F) not in _inputs:
        _inputs[(n, F)] = normalized(ar_features(n, F, 17))
    return _inputs[(n, F)]


def run_case(c):
    """the case's steps -> its digests, product plans and paths"""
    import torch

    from deep_cartograph_amd import hip
    from tests.test_mlp_gpu import push_params
    from tests.test_snet_dt_gpu import _TwoRanksInOneProcess, tile_rows

    class OneRank(_TwoRanksInOneProcess):
        @staticmethod
        def all_reduce(t, op=None, group=None, async_op=False):
            return None

    model, dims, B = c["model"], c["dims"], c["batch"]
    lag, nb_long = 1, c.get("nb_long", 0)
    nbig = max(3, nb_long)
    n = nbig * B + 64
    Xn, _, r = inputs(n, dims[0])
    Xd = torch.from_numpy(Xn).cuda()
    L = len(dims) - 1
    kw = dict(max_batch=B, lr=1e-3)
    if "dropout" in c:
        kw.update(dropout=c["dropout"], seed=c["seed"])
    steps = 9 + nb_long
    if model == "deep_tica":
        eng = hip.Mlp("deep_tica", dims, ["tanh"] * (L - 1) + [None], lag=lag, tica_reg=1e-6, **kw)
        torch.manual_seed(3)
        push_params(eng, [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(L)])
    elif model == "ae":
        eng = hip.Mlp("ae", dims, (["tanh"] * (L // 2 - 1) + [None]) * 2, latent_layer=L // 2, **kw)
        eng.set_feature_range(r)
        torch.manual_seed(3)
        push_params(eng, [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(L)])
    else:
        from tests.test_vae_gpu import REF_ACTS, _init

        eng = hip.Mlp("vae", dims, REF_ACTS, latent_layer=3, **kw)
        eng.set_feature_range(r)
        eng.set_linears(_init(dims, 3, 3))
        eng.set_kl_beta(0.1)
        eng.set_noise(torch.randn(steps * B, dims[3] // 2, generator=torch.Generator().manual_seed(19)).cuda())
    idx = torch.randperm(n - lag, generator=torch.Generator().manual_seed(7))[:nbig * B].contiguous().cuda() if c["gather"] else None

    def rows(j, row0):   # batch j of the index list, or the B rows from row0 on
        return dict(idx=idx[j * B:(j + 1) * B]) if c["gather"] else dict(row0=row0, batch=B)

    h, paths = hashlib.sha256(), []

    def done():
        torch.cuda.synchronize()
        paths.append(eng.last_path())
        h.update(np.ascontiguousarray(eng.stats_view().cpu().numpy()).tobytes())

    hip.gemm_log_reset()
    eng.reset_log(steps)
    eng.train_step(Xd, **rows(0, 5))
    done()
    if "tile_rows" in c:
        assert tile_rows(eng) == c["tile_rows"] and -(-B // (c["tile_rows"] // 2)) > c["tiles_over"], c["name"]
    eng.train_step(Xd, **rows(1, 9))
    done()
    eng.forward(Xd, **rows(0, 5))
    done()
    eng.backward(Xd, **rows(0, 5))
    done()
    eng.eval_step(Xd, **rows(2, 11))
    done()
    eng.eval_steps(Xd, B, 3, idx=idx, row0=7)
    done()
    eng.data_parallel_step(Xd, OneRank, B, train=True, **rows(1, 13))
    done()
    eng.data_parallel_step(Xd, OneRank, B, train=False, **rows(2, 13))
    done()
    if nb_long:
        eng.eval_steps(Xd, B, nb_long, idx=idx, row0=3)
        done()
    assert paths[0] == paths[1] == c["path"], (c["name"], paths)   # the training steps ran on the engine the case is there for
    rec = eng.read_log()
    assert rec.shape == (steps, eng.log_width) and np.isfinite(rec).all(), (c["name"], rec.shape)
    h.update(np.ascontiguousarray(rec).tobytes())
    p = hashlib.sha256()
    for w, b in eng.get_linears():
        p.update(np.ascontiguousarray(w).tobytes())
        p.update(np.ascontiguousarray(b).tobytes())
    plan = [" ".join(str(v if isinstance(v, str) else int(v)) for v in tuple(g)) for g in hip.gemm_log()]   # "single nt 128 64 1 1 0 3 0"
    eng.close()
    return dict(records=h.hexdigest(), params=p.hexdigest(), plan=plan, paths=paths)


def compute(env):
    """{"sha256": {case:records | case:params: digest}, "plan": {case: product plans}, "paths": {case: last_path per step}}"""
    out = dict(sha256={}, plan={}, paths={})
    for c in cases_of(env):
        got = run_case(c)
        out["sha256"][c["name"] + ":records"] = got["records"]
        out["sha256"][c["name"] + ":params"] = got["params"]
        out["plan"][c["name"]] = got["plan"]
        out["paths"][c["name"]] = got["paths"]
    return out


def run_child(env):
    """one fresh process with the environment's switches; its last output line is the JSON object"""
    e = dict(os.environ)
    for k in ("DCV_NO_SNET", "DCV_NO_HEAD_FUSION"):
        e.pop(k, None)
    e.update(ENVIRONMENTS[env])
    res = subprocess.run([sys.executable, os.path.abspath(__file__), env], env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("env", list(ENVIRONMENTS))
def test_loss_head_bit_equal_to_the_recorded_commit(env):
    with open(GOLDEN) as f:
        golden = json.load(f)
    want, got = golden["envs"][env], run_child(env)
    assert sorted(got["sha256"]) == sorted(want["sha256"])
    assert got["paths"] == want["paths"], {k: (got["paths"][k], want["paths"][k]) for k in got["paths"] if got["paths"][k] != want["paths"][k]}
    # parameters follow the launch plans of the block engine: those first, by name
    plans = {k: [(i, a, b) for i, (a, b) in enumerate(zip(got["plan"][k], want["plan"][k])) if a != b] or (len(got["plan"][k]), len(want["plan"][k]))
             for k in got["plan"] if got["plan"][k] != want["plan"][k]}
    assert not plans, f"other product plans than on {golden['device']} ({golden['multi_processor_count']} CUs): {plans}"
    differ = [k for k in sorted(got["sha256"]) if got["sha256"][k] != want["sha256"][k]]
    print(f"{env}: {len(got['sha256'])} digests against commit {golden['commit']}: {len(differ)} differ {differ}")
    assert not differ


if __name__ == "__main__":
    print(json.dumps(compute(sys.argv[1])))
