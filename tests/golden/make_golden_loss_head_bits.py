"""Generate tests/golden/loss_head_bits.json: per environment of tests/test_loss_head_bits_gpu.py the SHA-256 of every
case's loss records + batch statistics and of its parameters, the block-engine product plans the parameters were computed
with and the path every step took, as the library built from ONE commit computes them on an MI355X -- together with that
commit, the device name and its CU count.

Run on the GPU box, from a checkout of the commit the digests are to be pinned to, with libdcv.so built from it:

    python tests/golden/make_golden_loss_head_bits.py [--commit HASH] [--out FILE]

--commit names the commit where the tree is not a git checkout (default: git rev-parse HEAD).  Every environment runs twice,
each time in a fresh process (the switches are read once per process); nothing is written when the two runs differ.  A change
that is meant to leave the loss head's results alone records nothing: it passes against the file as it stands.

What is stored is data: seeded inputs (test_mlp_gpu.ar_features, torch.manual_seed) go through the library, and only digests,
plans and path numbers are kept.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "loss_head_bits.json"))
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()

    import torch

    from tests.test_loss_head_bits_gpu import ENVIRONMENTS, run_child

    envs = {}
    for env in ENVIRONMENTS:
        first, second = run_child(env), run_child(env)
        assert first == second, f"{env} is not deterministic: " + str([k for k in first["sha256"] if first["sha256"][k] != second["sha256"][k]])
        envs[env] = first
        print(f"{env}: {len(first['sha256'])} digests", flush=True)
    prop = torch.cuda.get_device_properties(0)
    with open(args.out, "w") as f:
        json.dump({"commit": commit, "device": prop.name, "multi_processor_count": prop.multi_processor_count, "envs": envs}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {sum(len(e['sha256']) for e in envs.values())} digests from commit {commit}")


if __name__ == "__main__":
    main()
