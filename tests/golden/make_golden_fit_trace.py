"""Generate tests/golden/fit_trace.json: per case of tests/fit_trace.py everything NonLinear.train() did against the recording
stand-in engine -- the ordered engine calls, return value, score, metrics, chosen checkpoint, try count, generator digest --
as the host driver of ONE commit does it, together with that commit and torch.__version__.  Runs on the CPU:

    python tests/golden/make_golden_fit_trace.py [--commit HASH] [--out FILE]

--commit names the commit where the tree is not a git checkout (default: git rev-parse HEAD).  Every case runs twice; nothing
is written when the two runs differ.  A change that is meant to leave the driver's decisions alone records nothing: it passes
against the file as it stands.

What is stored is data: seeded inputs go through the driver, and only call names, scalars and digests are kept.
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
    ap.add_argument("--out", default=os.path.join(HERE, "fit_trace.json"))
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()

    import torch

    from tests import fit_trace

    cases = {}
    for name in sorted(fit_trace.CASES):
        first, second = fit_trace.run_case(name), fit_trace.run_case(name)
        assert first == second, f"{name} is not deterministic: {fit_trace.first_difference(first, second, name)}"
        cases[name] = first
        print(f"{name}: {len(first['trace'])} calls, return {first['return']}, chosen {first['chosen']}", flush=True)
    with open(args.out, "w") as f:
        json.dump({"commit": commit, "torch": torch.__version__, "cases": cases}, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(cases)} cases from commit {commit}")


if __name__ == "__main__":
    main()
