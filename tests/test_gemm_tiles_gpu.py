"""The block engine's two most tuned tile families -- 128 x 128 (CfgBigT) and 64 x 64 (CfgQuarterT) -- as bare products against
a float64 product, in both arithmetic flavours.  tests/test_kernels_gpu.py's product tests never reach them: at their sizes the
tile choice (gemm_kernels.h: pick_cfg) sends NT / NN products to the narrow and 64 x 128 tiles and TN products to the narrow
and 64 x 64 ones.  The choice depends on the CU count, so every shape here follows it, and every test asserts from the
launch-plan log (hip.gemm_log) that the family, loader and flavour it is about were the ones launched.
Method: operands are integers in [-4, 4] (exact in fp32 and bf16, every partial sum exact), B is asymmetric, so the result
must equal the exact product bit for bit whatever the tile, loader or summation order; one random-normal case per family and
mode holds the fp32 bound of test_gemm_random_fp32.  Run on the GPU box: python -m pytest tests -m gpu"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLAVOURS = ["split", "native"]
# contraction lengths (a stage is 32 deep): whole stages, ring loop only | ring loop + register-staged remainder |
# K % 4 != 0 and less than one stage: the scalar loader of contraction-contiguous operands | a short contraction
KS = [64, 100, 30, 7]


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def family_shape(family, N=None):
    """(M, N, (TM, TN)) of a row-parallel (NT / NN) product that takes the family.  128 x 128: 2 * CUs workgroups at two
    column tiles, the last row tile ragged (68 of 128 rows).  64 x 64: CUs + 4 workgroups at four column tiles of 128 -- between
    one and two 64 x 128 workgroups per CU -- the last row tile ragged (36 of 64 rows)."""
    if family == "big":
        return 128 * ncu() - 60, (256 if N is None else N), (128, 128)
    return 64 * (ncu() // 4) + 36, (512 if N is None else N), (64, 64)


def int_operands(M, N, K, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    A = rng.integers(-4, 5, size=(M, K)).astype(np.float32)
    B = rng.integers(-4, 5, size=(K, N)).astype(np.float32)
    return A, B


def as_view(a, kind):
    """a (NumPy, 2-D) on the device as a view of a larger buffer.  'strided': row stride 8 floats beyond the extent (a multiple
    of 4 when the extent is, base 16-byte aligned: the 16-byte loaders stay legal); 'offset': the view starts one float into
    its buffer (misaligned base: scalar loaders)."""
    r, c = a.shape
    if kind == "contiguous":
        return torch.from_numpy(a).cuda()
    if kind == "strided":
        buf = torch.full((r, c + 8), 3.0, dtype=torch.float32, device="cuda")   # a loader that ignored the stride would read the 3s
        v = buf[:, :c]
    else:
        flat = torch.full((r * (c + 8) + 1,), 3.0, dtype=torch.float32, device="cuda")
        v = flat[1:].view(r, c + 8)[:, :c]
        assert v.data_ptr() % 16 == 4
    v.copy_(torch.from_numpy(a))
    return v


def product(hip, mode, A, B, view="contiguous"):
    """op(A) . op(B) of host A [M, K], B [K, N] through hip.gemm; returns (result on the host, launch log)"""
    if mode == "nt":
        a, b = as_view(A, view), as_view(np.ascontiguousarray(B.T), view)
    elif mode == "nn":
        a, b = as_view(A, view), as_view(B, view)
    else:
        a, b = as_view(np.ascontiguousarray(A.T), view), as_view(B, view)
    hip.gemm_log_reset()
    out = hip.gemm(mode, a, b)
    log = hip.gemm_log()
    return out.cpu().numpy(), log, (a, b)


def vec_expected(mode, a, b, K):
    """16-byte loaders: aligned bases, row strides that are multiples of 4, and K % 4 == 0 for contraction-contiguous operands"""
    ok = all(t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 for t in (a, b))
    if mode in ("nt", "nn"):
        ok = ok and K % 4 == 0
    return ok


def check_plan(log, mode, tile, flavour, vec, splits=1):
    assert len(log) == 1, log
    e = log[0]
    print("plan:", tuple(e))
    assert e.form == "single" and e.mode == mode, e
    assert (e.tm, e.tn) == tile, f"{e}: expected the {tile[0]} x {tile[1]} family"
    assert e.split == (flavour == "split"), e
    assert e.vec == vec and e.gather == (not vec), e   # scalar loads take the gather-capable kernel form
    assert e.splits == splits and e.tail_split == 0, e


class Flavour:
    def __init__(self, flavour):
        self.flavour = flavour

    def __enter__(self):
        from deep_cartograph_amd import hip

        self.start = hip.get_gemm_mode()
        hip.set_gemm_mode(self.flavour)
        return hip

    def __exit__(self, *exc):
        from deep_cartograph_amd import hip

        hip.set_gemm_mode(self.start)


# N = 200: a ragged column tile that still takes 16-byte loads; N = 131 (NN): B's and C's leading dimension is odd -- scalar
# loaders, scalar stores
ROW_PARALLEL = ([("nt", "big", N) for N in (256, 200)] + [("nn", "big", N) for N in (256, 200, 131)] +
                [("nt", "quarter", 512), ("nn", "quarter", 512)])


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("mode,family,N", ROW_PARALLEL)
def test_row_parallel_tiles_exact_on_integers(mode, family, N, K, flavour):
    M, N, tile = family_shape(family, N)
    A, B = int_operands(M, N, K, M + 3 * N + 7 * K)
    ref = (A.astype(np.float64) @ B.astype(np.float64)).astype(np.float32)   # exact
    with Flavour(flavour) as hip:
        out, log, (a, b) = product(hip, mode, A, B)
    check_plan(log, mode, tile, flavour, vec_expected(mode, a, b, K))
    np.testing.assert_array_equal(out, ref)


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("view", ["strided", "offset"])
@pytest.mark.parametrize("mode", ["nt", "nn"])
@pytest.mark.parametrize("family", ["big", "quarter"])
def test_operand_views_exact_on_integers(family, mode, view, flavour):
    """hip.gemm takes any row stride with unit column stride: operands that are views of a larger matrix."""
    M, N, tile = family_shape(family)
    K = 100
    A, B = int_operands(M, N, K, M + N + K + len(view))
    ref = (A.astype(np.float64) @ B.astype(np.float64)).astype(np.float32)
    with Flavour(flavour) as hip:
        out, log, (a, b) = product(hip, mode, A, B, view)
    assert not a.is_contiguous() and not b.is_contiguous()
    check_plan(log, mode, tile, flavour, vec=(view == "strided"))
    np.testing.assert_array_equal(out, ref)


def tn_single_shape():
    """TN, one split, 128 x 128: more tiles than CUs / 2 (12 x 13 on 256 CUs), N ragged"""
    t = int(np.ceil(np.sqrt(ncu() / 2)))
    return 128 * t, 128 * t + 4, 70


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_tn_single_split_big_exact_on_integers(flavour):
    M, N, K = tn_single_shape()
    A, B = int_operands(M, N, K, 17)
    ref = (A.astype(np.float64) @ B.astype(np.float64)).astype(np.float32)
    with Flavour(flavour) as hip:
        out, log, _ = product(hip, "tn", A, B)
    check_plan(log, "tn", (128, 128), flavour, vec=True)
    np.testing.assert_array_equal(out, ref)


def tn_split_case(name):
    """(M, N, k_chunk, K, tile): CUs / 8 + 8 slabs of four (or 2 x 2 ragged) 128 x 128 tiles exceed CUs / 2 workgroups; the
    64 x 64 case is test_short_slab_is_refused_not_overrun's shape with a ragged last chunk.  The last chunk is ragged in all."""
    slabs = ncu() // 8 + 8
    return {"big": (256, 256, 96, slabs * 96 - 17, (128, 128)),
            "big-ragged": (250, 196, 96, slabs * 96 - 17, (128, 128)),          # M % 4 != 0: scalar loaders
            "big-ragged-vec": (252, 196, 96, slabs * 96 - 17, (128, 128)),      # ragged tiles under 16-byte loaders
            "quarter": (96, 160, 512, 4096 - 5, (64, 64))}[name]


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("case", ["big", "big-ragged", "big-ragged-vec", "quarter"])
def test_tn_split_k_every_slab_exact_on_integers(case, flavour):
    """hip.gemm_tn_split, slab by slab: slab z must be A[z kc:(z+1) kc]^T B[z kc:(z+1) kc] exactly -- a row attributed to the
    wrong chunk is invisible in the sum of the slabs -- and the guard slab behind the capacity untouched."""
    M, N, kc, K, tile = tn_split_case(case)
    A, B = int_operands(M, N, K, 23 + M)
    At = np.ascontiguousarray(A.T)   # [K, M]
    nslab = -(-K // kc)
    with Flavour(flavour) as hip:
        a, b = torch.from_numpy(At).cuda(), torch.from_numpy(B).cuda()
        hip.gemm_log_reset()
        slabs = hip.gemm_tn_split(a, b, k_chunk=kc, slab_cap=nslab)
        log = hip.gemm_log()
    check_plan(log, "tn", tile, flavour, vec=(M % 4 == 0 and N % 4 == 0), splits=nslab)
    assert slabs.shape == (nslab + 1, M, N)
    assert torch.isnan(slabs[nslab]).all()   # guard slab untouched
    got = slabs[:nslab].cpu().numpy()
    for z in range(nslab):
        ref = (At[z * kc:(z + 1) * kc].astype(np.float64).T @ B[z * kc:(z + 1) * kc].astype(np.float64)).astype(np.float32)
        np.testing.assert_array_equal(got[z], ref, err_msg=f"slab {z}")


def random_case(family, mode):
    if mode != "tn":
        return family_shape(family) + (100,)
    if family == "big":
        M, N, K = tn_single_shape()
        return M, N, (128, 128), K
    return 96, 160, (64, 64), 300   # two tiles, one split: at most CUs / 2 workgroups of 128 x 128


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("mode", ["nt", "nn", "tn"])
@pytest.mark.parametrize("family", ["big", "quarter"])
def test_tiles_random_fp32(family, mode, flavour):
    """random-normal operands: the bound of test_gemm_random_fp32 (fp32 fma chain: error <= ~1.5e-7 * sum|a||b|)"""
    M, N, tile, K = random_case(family, mode)
    rng = np.random.Generator(np.random.PCG64(5))
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((K, N)).astype(np.float32)
    ref = A.astype(np.float64) @ B.astype(np.float64)
    with Flavour(flavour) as hip:
        out, log, _ = product(hip, mode, A, B)
    check_plan(log, mode, tile, flavour, vec=True)
    bound = 4e-7 * (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64))
    err = np.abs(out - ref)
    print(f"worst error / bound: {np.max(err / (bound + 1e-6)):.3f}")
    assert np.all(err <= bound + 1e-6)


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("gather", [False, True])
def test_grouped_launch_is_logged(gather, flavour):
    """The grouped launcher (gemm_group_kernel: the batches of a validation pass as members of one launch) notes its plan
    too: form 'group', NT, 16-byte loaders (scalar loads do not qualify for it), the gathering kernel form exactly when the
    batches come through an index, and the tail cut of the single launch of the same layer, which it must impose."""
    dims, batch, lag, nb, row0 = [256, 512, 128, 3], 1000, 10, 4, 5
    g = torch.Generator().manual_seed(3)
    X = torch.randn(row0 + batch * nb + lag + 8, dims[0], generator=g).cuda()
    idx = torch.randperm(batch * nb, generator=g).contiguous().cuda() if gather else None
    with Flavour(flavour) as hip:
        torch.manual_seed(1)
        eng = hip.Mlp("deep_tica", dims, ["leaky_relu", "leaky_relu", None], max_batch=batch, lag=lag, tica_reg=1e-6)
        eng.set_linears([(l.weight.detach().numpy(), l.bias.detach().numpy()) for l in
                         (torch.nn.Linear(dims[i], dims[i + 1]) for i in range(3))])
        eng.reset_log(nb + 1)
        hip.gemm_log_reset()
        eng.eval_step(X, **(dict(idx=idx[:batch]) if gather else dict(row0=row0, batch=batch)))
        single = [e for e in hip.gemm_log() if e.mode == "nt"]
        hip.gemm_log_reset()
        eng.eval_steps(X, batch, nb, idx=idx, row0=0 if gather else row0)
        log = hip.gemm_log()
        members = int(eng.lib.dcv_mlp_last_eval_group(eng.h))
        assert eng.last_path() == 0
        eng.close()
    print("single:", [tuple(e) for e in single], "pass:", [tuple(e) for e in log])
    assert members == nb, members
    assert [e.form for e in single] == ["single", "single"], single   # layer 0, layer 1 with the head fused
    group = [e for e in log if e.form == "group"]
    assert len(group) == 2 and len(log) == 2, log
    for e, one, gath in zip(group, single, (gather, False)):   # only layer 0 reads the caller's rows
        assert e.mode == "nt" and e.vec and e.splits == 1 and e.split == (flavour == "split"), e
        assert e.gather == gath and one.gather == gath, (e, one)
        assert e.tail_split == one.tail_split, (e, one)
