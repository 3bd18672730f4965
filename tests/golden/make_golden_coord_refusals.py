"""Generate tests/golden/coord_refusals.json: the return code and the dcv_last_error() text of every refusal that
tests/test_coord_entries_cpu.py's REFUSALS table provokes in the seven coordinate entries, as the library built from ONE
commit answers them, together with that commit.

Run on a machine WITHOUT a GPU (the device addresses of the cases are made up; the validation under test runs before the
first HIP call), from a checkout of the commit the texts are to be pinned to, with libdcv.so built from it:

    python tests/golden/make_golden_coord_refusals.py [--commit HASH] [--out FILE]

--commit names the commit where the tree is not a git checkout (default: git rev-parse HEAD).  Error texts are part of
the interface: a change that only moves the validation code records nothing and passes against the file as it stands.
Recorded from 98ea609 (the parent of the commit that introduced csrc/coords.h).
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
    ap.add_argument("--out", default=os.path.join(HERE, "coord_refusals.json"))
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()

    from tests.test_coord_entries_cpu import EINVAL, ENOMEM, compute_refusals

    first, second = compute_refusals(), compute_refusals()
    assert first == second, "not deterministic: " + str([k for k in first if first[k] != second[k]])
    stray = {k: v for k, v in first.items() if v["code"] not in (EINVAL, ENOMEM)}
    assert not stray, f"not refused by the validation: {stray}"
    with open(args.out, "w") as f:
        json.dump({"commit": commit, "refusals": first}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(first)} refusals from commit {commit}")


if __name__ == "__main__":
    main()
