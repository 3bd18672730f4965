"""tests/ae_block_oracle.py against float64 autograd of oracle.nn.AEModel, and the case tables of tests/test_ae_block_gpu.py:
every case well conditioned, every arithmetic claim of the tables counted at 256 CUs."""
import copy

import numpy as np
import pytest
import torch

from tests import ae_block_oracle as ab
from tests.test_mlp_gpu import linears_of

N_CU = 256


@pytest.mark.parametrize("acts", [
    ["tanh", None, "elu", None],
    ["leaky_relu", "tanh", "relu", "tanh"],
])
def test_ae_step_matches_float64_autograd(acts):
    """A ragged batch of 37 gathered rows through 33-12-3-7-33: the loss and every gradient tensor of ae_step in float64 against
    autograd of AEModel(...).double().step, to 1e-12 relative (the bound of tests/test_vae_oracle_cpu.py)."""
    c = ab.ae_case([33, 12, 3, 7, 33], acts, 2, 50, 4)
    rows = np.random.Generator(np.random.PCG64(1)).permutation(50)[:37]
    o = ab.ae_step(torch.from_numpy(c["Xn"])[rows], c["Ws"], c["bs"], acts, c["range"])
    ref64 = copy.deepcopy(c["ref"]).double()
    loss, _ = ref64.step(torch.from_numpy(c["Xn"]).double()[rows] * torch.from_numpy(c["range"]).double())
    loss.backward()
    worst = abs(o["loss"] - loss.item()) / abs(loss.item())
    assert abs(o["sse"] / (37 * 33) - o["loss"]) <= 1e-14 * o["loss"]
    for l, lin in enumerate(linears_of(ref64.encoder) + linears_of(ref64.decoder)):
        assert o["gw"][l].shape == tuple(lin.weight.shape) and o["gb"][l].shape == tuple(lin.bias.shape)
        worst = max(worst, ab.rel_dev(o["gw"][l], lin.weight.grad.numpy()), ab.rel_dev(o["gb"][l], lin.bias.grad.numpy()))
    print(f"{acts}: worst deviation from float64 autograd {worst:.2e}")
    assert worst < 1e-12
    # a fixed slope pattern equal to the layer's own changes nothing; a flipped one does
    kinks = ab.kink_layers(acts)
    if kinks:
        same = ab.ae_step(torch.from_numpy(c["Xn"])[rows], c["Ws"], c["bs"], acts, c["range"], patterns=dict(o["own"]))
        assert same["loss"] == o["loss"] and all(np.array_equal(a, b) for a, b in zip(same["gw"], o["gw"]))
        flipped = ab.ae_step(torch.from_numpy(c["Xn"])[rows], c["Ws"], c["bs"], acts, c["range"], patterns={kinks[0]: ~o["own"][kinks[0]]})
        assert flipped["loss"] != o["loss"]


def _conditioning(c, rows, what):
    """float32 ae_step against float64 ae_step on the same rows (slope pattern of the float64 run held fixed): a quarter of
    the GPU bounds, so that a correct float32 kernel has room"""
    x = torch.from_numpy(c["Xn"])[rows]
    o64 = ab.ae_step(x, c["Ws"], c["bs"], c["acts"], c["range"])
    o32 = ab.ae_step(x, c["Ws"], c["bs"], c["acts"], c["range"], patterns=dict(o64["own"]), dtype=torch.float32)
    g, lo = ab.step_deviation(o32, o64)
    print(f"{what}: float32 oracle vs float64: worst gradient tensor {g:.2e}, loss {lo:.2e}")
    for l, (gw, gb) in enumerate(zip(o64["gw"], o64["gb"])):
        assert np.max(np.abs(gw)) > 1e-8 and np.max(np.abs(gb)) > 1e-8, f"{what}: layer {l} has no gradient to compare with"
    assert g <= ab.GRAD_TOL / 4, f"{what}: gradient {g:.2e}"
    assert lo <= ab.REC_TOL / 4, f"{what}: loss {lo:.2e}"


@pytest.mark.parametrize("name", [k for k, v in ab.step_cases(N_CU).items() if v["rows"] <= 8300])
def test_step_cases_are_well_conditioned(name):
    """Group A cases of at most 8 300 rows at 256 CUs (the larger ones: once by hand, figures in the GPU test's docstring)."""
    k = ab.step_cases(N_CU)[name]
    c = ab.ae_case(k["dims"], k["acts"], k["latent"], ab.matrix_rows(k["rows"]), k["seed"])
    _conditioning(c, ab.rows_of(c, k["rows"], k["form"], k["seed"]), name)


def test_narrow_loss_and_colsum_cases_are_well_conditioned():
    """Groups B and C: every network once, at its largest row count of at most 8 300."""
    seen = set()
    for name, dims, acts, latent, form, mode, rides, vec in ab.narrow_cases():
        if (tuple(dims), tuple(acts)) in seen:
            continue
        seen.add((tuple(dims), tuple(acts)))
        c = ab.ae_case(dims, acts, latent, ab.matrix_rows(ab.NARROW_ROWS), 12)
        _conditioning(c, ab.rows_of(c, ab.NARROW_ROWS, form, 12), name)
    for rows, _ in ab.loss_rows(N_CU):
        if rows <= 8300:
            c = ab.ae_case(ab.LOSS_DIMS, ab._acts(ab.LOSS_DIMS, "tanh", 2), 2, ab.matrix_rows(rows), 13)
            _conditioning(c, ab.rows_of(c, rows, "row0", 13), f"loss network, {rows} rows")
    for dims, out_act in ab.COLSUM_NETS:
        for rows in ab.COLSUM_ROWS:
            c = ab.ae_case(dims, ab._acts(dims, "tanh", 2, None, out_act), 2, ab.matrix_rows(rows), 14)
            _conditioning(c, ab.rows_of(c, rows, "idx", 14), f"{dims} {rows} rows")


def test_case_tables_reach_what_they_claim():
    n = N_CU
    cases = ab.step_cases(n)
    # every case is off the fused kernel
    for name, k in cases.items():
        assert ab.off_the_fused_kernel(k["dims"], k["rows"]), name
        assert k["dims"][0] == k["dims"][-1] and len(k["acts"]) == len(k["dims"]) - 1
    for name, dims, acts, latent, form, mode, rides, vec in ab.narrow_cases():
        assert ab.off_the_fused_kernel(dims, ab.NARROW_ROWS), name
        d = dims[latent]
        assert rides == ("head4" if d <= 4 and dims[latent - 1] <= 128 else "head8" if d <= 8 and dims[latent - 1] <= 128 else None)
        assert vec == (d % 4 == 0)
    narrow = [k for k in ab.narrow_cases() if k[1][1] == 128]
    assert {k[1][2] for k in narrow} == {1, 2, 3, 4, 5, 8, 9}
    for d in (1, 2, 3, 4, 5, 8, 9):
        assert {k[5] for k in narrow if k[1][2] == d} == {"split", "native"}, d
    assert {k[2][1] for k in narrow if k[1][2] == 3} == {None, "tanh"}
    assert {k[4] for k in narrow} == {"idx", "row0"}
    assert any(k[1][1] == 256 and k[6] is None for k in ab.narrow_cases())
    assert ab.off_the_fused_kernel(ab.LOSS_DIMS, 1)
    for dims, _ in ab.COLSUM_NETS:
        assert ab.off_the_fused_kernel(dims, 77) and dims[-1] > 256
    assert ab.COLSUM_NETS[0][0][-1] % 256 != 0 and ab.COLSUM_NETS[0][0][-1] % 4 == 0 and ab.COLSUM_NETS[1][0][-1] % 4 != 0
    # A1 / A2: the contract shape, ragged and whole
    assert cases["A1"]["rows"] == 8202 and cases["A1"]["rows"] % 64 != 0 and cases["A2"]["rows"] == 8192 and cases["A2"]["form"] == "idx"
    # A4a: the first row count with 2 n tiles of 128 x 128 over four column tiles (pick_cfg: cdiv(M, 128) * cdiv(N, 128) >= 2 n); A4b: 2 n
    # such tiles over two column tiles and 2 n tiles of 64 x 128 over one; a ragged last tile in each
    R = cases["A4a"]["rows"]
    assert ab.cdiv(R, 128) * 4 >= 2 * n > ab.cdiv(R - 1, 128) * 4 and R % 128 != 0
    R = cases["A4b"]["rows"]
    assert ab.cdiv(R, 128) * 2 >= 2 * n and ab.cdiv(R, 64) >= 2 * n > ab.cdiv(R, 128) and R % 128 != 0 and R % 64 != 0
    # A5: more bias partials than the flat-grid reduction takes, on a wide last layer
    assert ab.bias_partials(cases["A5"]["rows"]) > 1024 and cases["A5"]["dims"][-1] > 256 and cases["A5"]["sgd"]
    # every other step case stays within it (so the training steps of A1 can ride)
    assert all(ab.bias_partials(k["rows"]) <= 1024 for name, k in cases.items() if name != "A5")
    # Group C: each row count in the regime it names, at both sides of every edge; the clamp at the two smallest
    F = ab.LOSS_DIMS[0]
    rows = [r for r, _ in ab.loss_rows(n)]
    for R, regime in ab.LOSS_REGIMES.items():
        assert R in rows and ab.ae_sse_plan(R, F)[0] == regime, (R, ab.ae_sse_plan(R, F))
    assert [ab.ae_sse_plan(R, F)[0] for R in (1024, 1025, 4096, 4097, 16384, 16385)] == \
        ["16/thread", "floor128", "floor128", "64/thread", "64/thread", "cap512"]
    # at F = 512 the 16-elements-per-thread regime asks for 8 rows per block, so the kSseRows clamp decides the whole of it and
    # the floor regime up to 1 920 rows: 1 920 / 1 921 are the clamp's last row count and the first that is free of it
    assert all(ab.ae_sse_plan(R, F)[3] for R in (1, 17, 1024, 1025, 1920)) and not any(ab.ae_sse_plan(R, F)[3] for R in (1921, 4096, 4097, 16384, 16385))
    assert 1920 in rows and 1921 in rows and ab.ae_sse_plan(1920, F)[1:3] == (16, 120) and ab.ae_sse_plan(1921, F)[1:3] == (16, 121)
    assert ab.ae_sse_plan(17, F)[1:3] == (16, 2) and ab.ae_sse_plan(16385, F)[1:3] == (33, 497) and ab.ae_sse_plan(4096, F)[2] == 128
    # the block plan never asks for more blocks than the partial buffer holds (cdiv(rows_cap, kSseRows), dcv_mlp_create)
    for R in rows:
        assert ab.ae_sse_plan(R, F)[2] <= ab.cdiv(R, ab.K_SSE_ROWS)
    # the grid-stride case: first row count of a second trip
    g = 8 * n + 1
    assert g in rows and g * F > 16 * n * 256 >= (g - 1) * F and ab.dY_trips(g, F, n) == 2 and ab.dY_trips(g - 1, F, n) == 1
    assert sum(1 for _, whole in ab.loss_rows(n) if whole) == 2 and dict(ab.loss_rows(n))[g]
    # Group D
    for name, dims, latent, d, rides in ab.VAE_NETS:
        assert dims[latent] == 2 * d and max(dims) > 256
        assert rides == (None if dims[latent - 1] > 128 else "head4" if 2 * d <= 4 else "head8")
        assert {b for k, _, _, b in ab.vae_cases(n) if k == name} == {0.3, 4.0}
        assert {f for k, _, f, _ in ab.vae_cases(n) if k == name} == {"row0", "idx"}
