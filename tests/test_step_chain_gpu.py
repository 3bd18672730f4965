"""One-GPU training steps of the block engine: every gradient but layer 0's weights is reduced and updated by extra workgroups
of the layer-0 weight-gradient launch (csrc/ride.hip, mlp_opt.hip: ride_upper); the final reduction holds the W0 item alone.
Items, arithmetic and update arguments are those of the single reduction, so DCV_NO_REDUCE_RIDE=1 (the single reduction) must
leave every bit alone: statistics, loss records, gradients, parameters and the optimiser's state after three steps.  The switch is
read once per process, so each comparison runs the two settings in fresh child processes, both at once.
dcv_mlp_last_ride() says which path a step took."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import hashlib, sys
import numpy as np, torch
sys.path.insert(0, {root!r})
from deep_cartograph_amd import hip
case = sys.argv[1]
F, d, lag, hidden = 64, 3, 10, [128, 128]
batches, kw, bn, gathered, dp = [300, 300, 300], {{}}, None, False, False
if case == "nadam":
    kw = dict(optimizer="NAdam", opt_params=[4e-3, 0.0])
elif case == "asgd":            # host-side state that advances with the step count (eta)
    kw = dict(optimizer="ASGD", opt_params=[1e-4, 0.75])
elif case == "amsgrad":         # an optimiser with auxiliary state
    kw = dict(optimizer="Adam", amsgrad=True)
elif case == "batchnorm":       # the normalisation's weight / bias ride along
    bn = [False, True, False]
elif case == "two_layers":      # only the biases and one upper layer ride
    hidden = [128]
elif case == "d1":
    d = 1
elif case == "d4_sizes":        # 16 + 1 bias partials, then fewer, then as many again: item tables of different lengths on one engine
    d, batches = 4, [512, 300, 512]
elif case == "tiny":            # one row tile, one weight-gradient chunk
    batches, lag = [20, 20, 20], 3
elif case == "big_tiles":       # 8 output tiles x 64 chunks of the layer-0 weight gradient: the 128 x 128 tile family (from 16 129 rows), while
    F, hidden, batches = 512, [256, 128], [16300, 16300, 16300]   # the last layer's 510 partials still take the flat-grid reduction (<= 512)
elif case == "gathered":        # index lists: the gathering loader is not wrapped, the single reduction stays
    gathered = True
elif case == "data_parallel":   # world 1: gradients are all-reduced between reduction and update, nothing rides
    dp = True
else:
    assert case == "adam", case
dims = [F] + hidden + [d]
acts = ["leaky_relu"] * len(hidden) + [None]
if bn is not None:
    bn = bn[: len(dims) - 1]
n = max(batches) + 3 * 37 + 64
rng = np.random.Generator(np.random.PCG64(11))
X = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32).cumsum(0) * 0.02 + rng.standard_normal((n, F)).astype(np.float32)).cuda()
eng = hip.Mlp("deep_tica", dims, acts, max_batch=max(batches), lag=lag, tica_reg=1e-6, lr=1e-3, batchnorm=bn, **kw)
torch.manual_seed(3)
lins = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]
eng.set_linears([(l.weight.detach().numpy(), l.bias.detach().numpy()) for l in lins])
eng.reset_log(16)
comm = hip.RcclComm(None) if dp else None
h = hashlib.sha256()
rides = []
for i, b in enumerate(batches):
    if gathered:
        idx = torch.from_numpy(rng.permutation(n - lag)[:b].astype(np.int64)).cuda()
        eng.train_step(X, idx=idx)
    elif dp:
        eng.data_parallel_step(X, comm, b, row0=37 * i, batch=b, train=True)
    else:
        eng.train_step(X, row0=37 * i, batch=b)
    assert eng.last_path() == 0, eng.last_path()
    rides.append(eng.last_ride())
    torch.cuda.synchronize()
    views = [eng.stats_view(), eng.grads_view(), eng.params_view(), eng.opt_state_view(0), eng.opt_state_view(1), eng.opt_state_view(2)]
    for v in views:
        if v is not None:
            h.update(v.cpu().numpy().tobytes())
h.update(np.ascontiguousarray(eng.read_log()).tobytes())
assert np.isfinite(eng.read_log()).all() and len(eng.read_log()) == len(batches)
assert (eng.opt_state_view(2) is not None) == (case == "amsgrad")
print("RIDES", rides)
print("HASH", h.hexdigest())
"""

# True: the upper gradients must ride; False: the single reduction must stay
_CASES = {"adam": True, "nadam": True, "asgd": True, "amsgrad": True, "batchnorm": True, "two_layers": True, "d1": True, "d4_sizes": True,
          "tiny": True, "big_tiles": True, "gathered": False, "data_parallel": False}


def _run_pair(script, case):
    procs = []
    for ride_off in ("0", "1"):
        env = dict(os.environ)
        env["DCV_NO_SNET"] = "1"          # the block engine, whatever the network's size
        env["DCV_NO_REDUCE_RIDE"] = ride_off
        procs.append(subprocess.Popen([sys.executable, str(script), case], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            out, err = p.communicate(timeout=180)
            assert p.returncode == 0, err[-2000:]
            outs.append(out)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    pick = lambda out, key: [l for l in out.splitlines() if l.startswith(key)][-1]
    return [(pick(o, "HASH"), eval(pick(o, "RIDES")[len("RIDES "):])) for o in outs]


@pytest.mark.parametrize("case", sorted(_CASES))
def test_reduction_ride_leaves_the_bits_alone(case, tmp_path):
    script = tmp_path / "ride_run.py"
    script.write_text(_CHILD.format(root=ROOT))
    (h_on, rides_on), (h_off, rides_off) = _run_pair(script, case)
    print(case, "rides", rides_on, "switched off", rides_off)
    assert rides_off == [0, 0, 0], rides_off
    if _CASES[case]:
        assert all(r > 0 for r in rides_on), rides_on
    else:
        assert rides_on == [0, 0, 0], rides_on
    assert h_on == h_off, (case, h_on, h_off)
