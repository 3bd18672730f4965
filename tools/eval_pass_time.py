"""Times a validation pass of the headline Deep-TICA engine by itself: 512-256-128-4, 244 batches of 8192
pairs (lag 10) behind the training rows of a resident matrix, 50 training steps first, then dcv_mlp_eval_steps between HIP
events, five repetitions; prints the median per validation batch as one JSON line.

    python tools/eval_pass_time.py [frames]            (DCV_EVAL_GROUP=0: the batch-by-batch pass)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deep_cartograph_amd import hip


def main():
    n, F, batch, lag, nval = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000, 512, 8192, 10, 244
    n_train = n - nval * batch - lag - 8
    assert n_train >= 50 * batch, "too few frames for 50 training steps in front of the validation rows"
    torch.manual_seed(0)
    Xn = torch.randn(n, F, device="cuda")
    dims = [F, 256, 128, 4]
    eng = hip.Mlp("deep_tica", dims, ["leaky_relu", "leaky_relu", None], max_batch=batch, lag=lag, tica_reg=1e-6, lr=1e-3)
    eng.set_linears([(l.weight.detach().numpy(), l.bias.detach().numpy()) for l in [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(3)]])
    eng.reset_log(64 + 8 * nval)
    eng.train_steps(Xn, batch, 50, row0=0)
    eng.eval_steps(Xn, batch, nval, row0=n_train)   # the first pass allocates the group workspace
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        eng.train_steps(Xn, batch, 10, row0=0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.eval_steps(Xn, batch, nval, row0=n_train)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / nval)
    times.sort()
    print(json.dumps({"us_per_validation_batch_median": round(times[2], 2), "all": [round(t, 2) for t in times],
                      "group": int(eng.lib.dcv_mlp_last_eval_group(eng.h)), "frames": n}))


if __name__ == "__main__":
    main()
