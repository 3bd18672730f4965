"""The block engine's grouped validation pass (mlp_passes.hip: eval_group; gemm_kernels.h: gemm_group_kernel): dcv_mlp_eval_steps
evaluates the batches of a pass side by side, one launch per layer with a member per batch, and must append the records
dcv_mlp_eval_step appends one call at a time -- BIT FOR BIT.  No tolerance appears in this file: every comparison is
np.array_equal / torch.equal on what the two paths leave behind.  dcv_mlp_last_eval_group() says which path a call took."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_mlp_gpu import ar_features, normalized, push_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = [512, 256, 128, 4]   # the bench's network: layer 1 carries the 128 -> 4 head in its epilogue
WIDE_HEAD = [256, 512, 128]     # + [d]: too wide for the fused small-network kernels, head fused into layer 1
WIDE_PLAIN = [256, 512, 256]    # + [d]: the narrow last layer is a launch of its own (256 columns do not fit one column tile)


def group_of(eng):
    return int(eng.lib.dcv_mlp_last_eval_group(eng.h))


def make_engine(dims, batch, lag, init_seed=1, act="leaky_relu", **kw):
    from deep_cartograph_amd import hip

    torch.manual_seed(init_seed)
    eng = hip.Mlp("deep_tica", dims, [act] * (len(dims) - 2) + [None], max_batch=batch, lag=lag, tica_reg=1e-6, lr=1e-3, **kw)
    push_params(eng, [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)])
    return eng


def features(rows, F, seed=5):
    Xn, _, _ = normalized(ar_features(rows, F, seed))
    return torch.from_numpy(Xn).cuda()


def batch_kw(idx, row0, batch, j):
    return dict(idx=idx[j * batch:(j + 1) * batch]) if idx is not None else dict(row0=row0 + j * batch, batch=batch)


def stepped(eng, Xd, batch, nb, idx, row0, lead=1):
    """`lead` records first (the counter the pass starts from), then nb single steps."""
    eng.reset_log(nb + lead)
    for _ in range(lead):
        eng.eval_step(Xd, **batch_kw(idx, row0, batch, 0))
    for j in range(nb):
        eng.eval_step(Xd, **batch_kw(idx, row0, batch, j))
    return eng.read_log()


def passed(eng, Xd, batch, nb, idx, row0, lead=1):
    """The same through one dcv_mlp_eval_steps call; returns (records, members of its first grouped launch)."""
    eng.reset_log(nb + lead)
    for _ in range(lead):
        eng.eval_step(Xd, **batch_kw(idx, row0, batch, 0))
    eng.eval_steps(Xd, batch, nb, idx=idx, row0=0 if idx is not None else row0)
    return eng.read_log(), group_of(eng)


def check_pass(eng, Xd, batch, nb, idx, row0, want_group):
    a = stepped(eng, Xd, batch, nb, idx, row0)
    b, grp = passed(eng, Xd, batch, nb, idx, row0)
    print(f"nb={nb} group={grp} records equal: {np.array_equal(a, b)} (differing records: {int((a != b).any(axis=1).sum()) if a.shape == b.shape else -1})")
    assert a.shape == b.shape == (nb + 1, eng.log_width)
    assert np.isfinite(a).all() and len(np.unique(a[1:, 0])) == nb   # the batches do differ
    assert grp == want_group, (grp, want_group)
    assert np.array_equal(a, b)
    assert eng.last_path() == 0
    return a


@pytest.mark.parametrize("mode", ["split", "native"])
@pytest.mark.parametrize("gather", [False, True])
def test_headline_shape(mode, gather):
    """512-256-128-4, 8192 pairs, lag 10: 8202 shared rows from row0 = 37 (the ragged last row tile of both products is cut along
    the contraction, in the single launch and in every member alike) / 16 384 rows gathered through a random index."""
    from deep_cartograph_amd import hip

    batch, lag, nb, row0 = 8192, 10, 5, 37
    Xd = features(row0 + batch * nb + lag + 8, HEADLINE[0])
    idx = torch.randperm(batch * nb + 8)[:batch * nb].contiguous().cuda() if gather else None
    before = hip.get_gemm_mode()
    hip.set_gemm_mode(mode)
    try:
        eng = make_engine(HEADLINE, batch, lag)
        check_pass(eng, Xd, batch, nb, idx, row0, want_group=nb)
        check_pass(eng, Xd, batch, 2, idx, row0, want_group=2)
    finally:
        hip.set_gemm_mode(before)


def test_headline_shape_full_group():
    """The groups of the bench's pass: as many 8202-row members as the workspace budget holds take 128 x 128 tiles in both
    products (one batch takes 64 x 64 and 32 x 128), the ragged tile of every member still cut as the single launch cuts it;
    one batch beyond the group goes through dcv_mlp_eval_step."""
    from deep_cartograph_amd import hip

    batch, lag, row0, many = 8192, 10, 37, 20
    Xd = features(row0 + batch * many + lag + 8, HEADLINE[0])
    before = hip.get_gemm_mode()
    try:
        for mode in ("split", "native"):
            hip.set_gemm_mode(mode)
            eng = make_engine(HEADLINE, batch, lag)
            eng.reset_log(many)
            eng.eval_steps(Xd, batch, many, row0=row0)
            cap = group_of(eng)
            print(f"{mode}: group capacity {cap}")
            assert 16 <= cap < many   # (the budget is chosen for >= 16 members of this shape)
            check_pass(eng, Xd, batch, cap + 1, None, row0, want_group=cap)
    finally:
        hip.set_gemm_mode(before)


@pytest.mark.parametrize("mode", ["split", "native"])
@pytest.mark.parametrize("dims,gather", [
    (WIDE_HEAD + [3], False), (WIDE_HEAD + [3], True), (WIDE_PLAIN + [3], False), (WIDE_PLAIN + [2], True),
    (WIDE_HEAD + [1], False), (WIDE_HEAD + [2], False), (WIDE_PLAIN + [1], True), (WIDE_HEAD + [4], True),
])
def test_ragged_batches_many_members(mode, dims, gather):
    """1000 pairs, lag 7 (1007 rows: no multiple of any tile height) on networks too wide for the fused kernels, outputs of
    1 - 4 columns: 2 and 5 batches, a full group and one batch left over (dcv_mlp_eval_step), a full group and a group of three;
    the log counter starts at 1 everywhere."""
    from deep_cartograph_amd import hip

    batch, lag, row0, many = 1000, 7, 3, 72
    Xd = features(row0 + batch * many + lag + 8, dims[0], seed=7)
    idx = torch.randperm(batch * many + 8)[:batch * many].contiguous().cuda() if gather else None
    before = hip.get_gemm_mode()
    hip.set_gemm_mode(mode)
    try:
        eng = make_engine(dims, batch, lag, init_seed=2)
        eng.reset_log(many)
        eng.eval_steps(Xd, batch, many, idx=idx, row0=0 if gather else row0)
        cap = group_of(eng)   # a pass longer than any group: its first launch is a full one
        print(f"group capacity {cap}")
        assert 2 <= cap <= many - 3
        for nb in (2, 5, cap + 1, cap + 3):
            check_pass(eng, Xd, batch, nb, idx, row0, want_group=min(nb, cap))
    finally:
        hip.set_gemm_mode(before)


def test_short_log_keeps_the_records_that_fit():
    batch, lag, nb, row0 = 1000, 7, 5, 3
    dims = WIDE_HEAD + [3]
    Xd = features(row0 + batch * nb + lag + 8, dims[0], seed=7)
    a = stepped(make_engine(dims, batch, lag, init_seed=2), Xd, batch, nb, None, row0, lead=0)
    eng = make_engine(dims, batch, lag, init_seed=2)   # (the host wrapper reads back as many records as its largest log held)
    eng.reset_log(3)
    eng.eval_steps(Xd, batch, nb, row0=row0)
    assert group_of(eng) == nb
    c = eng.read_log()
    assert c.shape == (3, eng.log_width) and np.array_equal(c, a[:3])
    # the counter moved past the end like five single steps move it: nothing more is recorded
    eng.eval_step(Xd, row0=row0, batch=batch)
    assert np.array_equal(eng.read_log(), a[:3])


SCRIPT = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from tests.test_eval_group_gpu import WIDE_HEAD, features, group_of, make_engine, passed
batch, lag, nb, row0 = 1000, 7, 5, 3
dims = WIDE_HEAD + [3]
Xd = features(row0 + batch * nb + lag + 8, dims[0], seed=7)
eng = make_engine(dims, batch, lag, init_seed=2)
rec, grp = passed(eng, Xd, batch, nb, None, row0)
np.savez(sys.argv[2], rec=rec, grp=grp)
"""


def test_switched_off_in_a_fresh_process(tmp_path):
    """DCV_EVAL_GROUP=0 (read once per process): the same records, batch by batch."""
    script = tmp_path / "pass.py"
    script.write_text(SCRIPT)
    got = {}
    for val in ("0", None):
        env = dict(os.environ)
        env.pop("DCV_EVAL_GROUP", None)
        if val is not None:
            env["DCV_EVAL_GROUP"] = val
        out = tmp_path / f"rec_{val}.npz"
        res = subprocess.run([sys.executable, str(script), ROOT, str(out)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr[-2000:]
        got[val] = np.load(out)
    assert int(got["0"]["grp"]) == 0 and int(got[None]["grp"]) == 5
    assert got["0"]["rec"].shape == (6, 2 + 2 * 9 + 3) and np.array_equal(got["0"]["rec"], got[None]["rec"])


@pytest.mark.parametrize("dims,batch,lag,gather", [(HEADLINE, 8192, 10, False), (WIDE_PLAIN + [3], 1000, 7, True)])
def test_training_step_after_a_grouped_pass(dims, batch, lag, gather):
    """A grouped pass touches nothing a training step reads: two training steps with a pass in between leave the parameters
    and the training records of two training steps without it."""
    nb, row0 = 4, 5
    Xd = features(row0 + batch * nb + lag + 8, dims[0], seed=9)
    idx = torch.randperm(batch * nb + 8)[:batch * nb].contiguous().cuda() if gather else None
    res = []
    for with_pass in (False, True):
        eng = make_engine(dims, batch, lag, init_seed=3)
        eng.reset_log(2 + nb)
        eng.train_step(Xd, **batch_kw(idx, row0, batch, 0))
        if with_pass:
            eng.eval_steps(Xd, batch, nb, idx=idx, row0=0 if gather else row0)
            assert group_of(eng) == nb
        eng.train_step(Xd, **batch_kw(idx, row0, batch, 1))
        rec = eng.read_log()
        res.append((eng.params_view().clone(), rec[[0, -1]], eng.grads_view().clone()))
    assert np.isfinite(res[0][1]).all()
    assert np.array_equal(res[0][1], res[1][1])
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][2], res[1][2])


@pytest.mark.parametrize("what", ["dropout", "batchnorm", "five_outputs"])
def test_engines_that_keep_stepping(what):
    """Dropout, batch normalisation and more than 4 outputs stay on the batch-by-batch path behind the same call."""
    batch, lag, nb, row0 = 1000, 7, 4, 3
    dims = WIDE_HEAD + [5 if what == "five_outputs" else 3]
    kw = {"dropout": dict(dropout=[0.25, 0.0, 0.0], seed=5), "batchnorm": dict(batchnorm=[1, 0, 0]), "five_outputs": {}}[what]
    Xd = features(row0 + batch * nb + lag + 8, dims[0], seed=7)
    eng = make_engine(dims, batch, lag, init_seed=2, **kw)
    check_pass(eng, Xd, batch, nb, None, row0, want_group=0)
