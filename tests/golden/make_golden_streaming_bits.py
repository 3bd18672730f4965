"""Generate tests/golden/streaming_bits.json: the SHA-256 of every output of tests/test_streaming_bits_gpu.py's cases, as
the library built from ONE commit computes them on an MI355X, together with that commit.

Run on the GPU box, from a checkout of the commit the digests are to be pinned to, with libdcv.so built from it:

    python tests/golden/make_golden_streaming_bits.py [--commit HASH] [--out FILE]

--commit names the commit where the tree is not a git checkout (default: git rev-parse HEAD).  A change that is meant to
leave the streaming kernels' results alone records nothing: it passes against the file as it stands.  A change that is
meant to move them records the file anew from its own commit and says so.

What is stored is data: seeded inputs (np.random.PCG64, test_streaming_gpu.rand_matrix) go through the library, and
only digests of the results are kept.
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
    ap.add_argument("--out", default=os.path.join(HERE, "streaming_bits.json"))
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()

    import torch

    from tests.test_streaming_bits_gpu import compute_digests

    first, second = compute_digests(), compute_digests()
    assert first == second, "not deterministic: " + str([k for k in first if first[k] != second[k]])
    with open(args.out, "w") as f:
        json.dump({"commit": commit, "device": torch.cuda.get_device_name(0), "sha256": first}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(first)} digests from commit {commit}")


if __name__ == "__main__":
    main()
