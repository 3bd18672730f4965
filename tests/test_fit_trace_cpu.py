"""The neural-CV training driver (NonLinear.train) pinned on the CPU: with a recording stand-in for the HIP engine
(tests/fit_trace.py) every case's ordered engine calls, return value, score, metrics, chosen checkpoint, try count and final
generator state must equal tests/golden/fit_trace.json, recorded at the commit named there.  No GPU."""
import json
import os

import pytest
import torch

from tests import fit_trace
from tests.conftest import GOLDEN

with open(os.path.join(GOLDEN, "fit_trace.json")) as _f:
    RECORDED = json.load(_f)


def test_golden_covers_the_cases():
    assert sorted(RECORDED["cases"]) == sorted(fit_trace.CASES)


@pytest.mark.parametrize("name", sorted(fit_trace.CASES))
def test_fit_trace(name):
    assert torch.__version__ == RECORDED["torch"], (
        f"tests/golden/fit_trace.json was recorded with torch {RECORDED['torch']}, this is {torch.__version__}: initialisation and "
        f"permutations may differ -- re-record it with tests/golden/make_golden_fit_trace.py from commit {RECORDED['commit']}")
    got, want = fit_trace.run_case(name), dict(RECORDED["cases"][name])
    if name in fit_trace.NO_RNG_DIGEST:
        got.pop("rng"), want.pop("rng")
    assert got == want, fit_trace.first_difference(got, want, name)


def test_case_outcomes():
    """What the cases were chosen to reach, read from the recorded results."""
    c = RECORDED["cases"]
    calls = lambda name: {e[0] for e in c[name]["trace"]}
    for name in ("deep_tica", "ae", "vae"):
        assert c[name]["return"] is True and c[name]["tries"] == 2
        assert c[name]["metrics"]["epoch"] == [0, 1, 2, 3, 4]                  # early stop: patience 2 after the minimum at epoch 2
        assert calls(name) >= {"train_steps", "train_step", "eval_steps", "eval_step"}   # many-steps call + ragged last batch
    assert c["ae"]["chosen"] == {"engine": 2, "reads": 3}                    # second try, checkpoint of epoch 2
    assert c["ae_last"]["chosen"] == {"engine": 2, "reads": 4} and c["ae_last"]["cv_score"] == c["ae_last"]["metrics"]["valid_loss"][-1]
    assert not calls("deep_tica_one_batch") & {"train_steps", "eval_steps"}
    assert "train_steps" not in calls("ae_one_cycle") and "eval_steps" in calls("ae_one_cycle")
    assert c["ae_nan"]["return"] is False and c["ae_nan"]["chosen"] is None
    assert calls("ae_two_ranks") & {"train_step", "eval_step", "train_steps", "eval_steps"} == set()
    assert all(e[1]["global_batch"] == 2 * e[1]["n"] for e in c["ae_two_ranks"]["trace"] if e[0] == "data_parallel_step")
    assert c["ae_two_ranks_batchnorm"]["return"] is False and "data_parallel_step" not in calls("ae_two_ranks_batchnorm")
    assert any(e[1]["X"] == "val" for e in c["deep_tica_separate_val"]["trace"] if e[0].startswith("eval"))


def test_generator_restored_after_failed_epoch():
    """A try that ends in an epoch with the next epoch's permutation already drawn (non-finite loss in epoch 1 of 6) leaves
    torch's global generator where the same failure leaves it when nothing was prefetched (epoch 1 of 2).  Fails before the
    prefetch was given its try / finally: the generator stayed one randperm ahead on every exit but the early stop."""
    states = []
    for max_epochs in (6, 2):
        result = fit_trace.run_case("ae_nan", general={"max_epochs": max_epochs})
        assert result["return"] is False
        states.append(result["rng"])
    assert states[0] == states[1]
