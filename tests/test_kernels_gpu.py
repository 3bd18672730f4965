"""Parity of the HIP kernels (through the C-ABI) against the CPU oracle / float64 NumPy.
Run on the GPU box: python -m pytest tests -m gpu"""
import numpy as np
import pytest
import torch

from oracle import cluster as oc
from oracle import linear as ol
from tests import kmeans_oracle as ko

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.as_tensor(a).cuda()


def rand_matrix(n, F, seed, scramble=True):
    rng = np.random.Generator(np.random.PCG64(seed))
    X = rng.standard_normal((n, F)).astype(np.float32)
    if scramble:
        X = X * rng.uniform(0.1, 10, F).astype(np.float32) + rng.uniform(-5, 5, F).astype(np.float32)
    return X


@pytest.mark.parametrize("n,F", [(164, 54), (10000, 128), (5000, 512), (3001, 1024), (700, 2048), (1, 8), (5, 3)])
def test_col_stats(n, F):
    from deep_cartograph_amd import hip

    X = rand_matrix(n, F, 1)
    raw = hip.col_stats_raw(dev(X)).cpu().numpy()
    X64 = X.astype(np.float64)
    np.testing.assert_allclose(raw[0], X64.sum(0), rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(raw[1], (X64 * X64).sum(0), rtol=1e-12)
    np.testing.assert_array_equal(raw[2], X64.min(0))
    np.testing.assert_array_equal(raw[3], X64.max(0))
    if n > 1:
        st = hip.finalize_stats(torch.from_numpy(raw), n)
        ref = ol.feature_stats(X)
        # tolerance: pandas accumulates in float32, the kernel in float64
        np.testing.assert_allclose(st["mean"], ref["mean"], rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(st["std"], ref["std"], rtol=2e-5)
        np.testing.assert_array_equal(st["min"], ref["min"])
        np.testing.assert_array_equal(st["max"], ref["max"])


@pytest.mark.parametrize("n,F", [(164, 54), (4096, 256), (1000, 100)])
def test_normalize_bit_exact(n, F):
    from deep_cartograph_amd import hip

    X = rand_matrix(n, F, 2)
    st = ol.feature_stats(X)
    m, r = ol.prepare_normalization(st, "mean_std")
    ref = ol.normalize(X, m, r)
    Xd = dev(X)
    out = hip.normalize(Xd, dev(m.astype(np.float32)), dev(r.astype(np.float32)))
    np.testing.assert_array_equal(out.cpu().numpy(), ref)
    hip.normalize(Xd, dev(m.astype(np.float32)), dev(r.astype(np.float32)), out=Xd)  # in place, as the reference
    np.testing.assert_array_equal(Xd.cpu().numpy(), ref)


GEMM_SHAPES = [(128, 128, 64), (300, 200, 100), (64, 4, 128), (4, 128, 1000), (257, 33, 31), (1000, 256, 512),
               (129, 130, 33), (32, 32, 2), (512, 2, 7), (2, 512, 40)]


# every product kind in both arithmetic modes; the split case (the library's default mode, the one this test ran in
# before it had the parameter) keeps the id it always had
GEMM_KIND_MODES = [pytest.param(kind, gm, id=kind if gm == "split" else kind + "-" + gm)
                   for kind in ("nt", "nn", "tn") for gm in ("native", "split")]


@pytest.mark.parametrize("mode,gemm_mode", GEMM_KIND_MODES)
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_exact_on_integers(mode, M, N, K, gemm_mode):
    """Small-integer operands make every fp32 product and partial sum exact, so the MFMA
    engine must agree bit for bit with an int64 product whatever the tile / k-slot order;
    B is asymmetric, so a transposed C write cannot pass.  Operands in [-4, 4] are exact
    in bf16 as well, so the same holds for the split flavour: every ragged shape is
    checked in both arithmetic modes."""
    from deep_cartograph_amd import hip

    rng = np.random.Generator(np.random.PCG64(M * 7 + N * 3 + K))
    A = rng.integers(-4, 5, size=(M, K))
    B = rng.integers(-4, 5, size=(K, N))
    ref = (A @ B).astype(np.float32)
    Af = A.astype(np.float32)
    Bf = B.astype(np.float32)
    start = hip.get_gemm_mode()
    try:
        hip.set_gemm_mode(gemm_mode)
        if mode == "nt":
            out = hip.gemm("nt", dev(Af), dev(np.ascontiguousarray(Bf.T)))
        elif mode == "nn":
            out = hip.gemm("nn", dev(Af), dev(Bf))
        else:
            out = hip.gemm("tn", dev(np.ascontiguousarray(Af.T)), dev(Bf))
        out = out.cpu().numpy()
    finally:
        hip.set_gemm_mode(start)
    np.testing.assert_array_equal(out, ref)


@pytest.mark.parametrize("mode", ["nt", "nn", "tn"])
def test_gemm_random_fp32(mode):
    from deep_cartograph_amd import hip

    rng = np.random.Generator(np.random.PCG64(5))
    M, N, K = 384, 256, 640
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((K, N)).astype(np.float32)
    ref = A.astype(np.float64) @ B.astype(np.float64)
    if mode == "nt":
        out = hip.gemm("nt", dev(A), dev(np.ascontiguousarray(B.T)))
    elif mode == "nn":
        out = hip.gemm("nn", dev(A), dev(B))
    else:
        out = hip.gemm("tn", dev(np.ascontiguousarray(A.T)), dev(B))
    # fp32 fma chain: error <= ~1.5e-7 * sum|a||b| (guide: FP32-input MFMA numerics)
    bound = 4e-7 * (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64))
    assert np.all(np.abs(out.cpu().numpy() - ref) <= bound + 1e-6)


def test_gemm_modes_split_vs_native():
    """The two arithmetic flavours of the product engine (dcv_set_gemm_mode): FP32-input MFMA and FP32-accurate split
    products on the BF16 pipe.  Both meet the fp32 error bound against float64 on zero-mean data; on a long same-sign
    accumulation (K = 8192) the BF16 pipe's truncating accumulator shows its bias -- bounded here at 4e-5 relative,
    which is why the covariance kernels never use it -- while the native path stays unbiased."""
    from deep_cartograph_amd import hip

    start = hip.get_gemm_mode()
    try:
        rng = np.random.Generator(np.random.PCG64(8))
        A = rng.standard_normal((256, 512)).astype(np.float32)
        B = rng.standard_normal((192, 512)).astype(np.float32)
        ref = A.astype(np.float64) @ B.astype(np.float64).T
        bound = 4e-7 * (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T)
        outs = {}
        for mode in ("native", "split"):
            hip.set_gemm_mode(mode)
            assert hip.get_gemm_mode() == mode
            outs[mode] = hip.gemm("nt", dev(A), dev(B)).cpu().numpy()
            assert np.all(np.abs(outs[mode] - ref) <= bound + 1e-6), mode
        assert not np.array_equal(outs["native"], outs["split"])       # the switch does switch
        Ap = (rng.random((8192, 128)) + 0.1).astype(np.float32)        # K = 8192 rows of positive numbers (TN form)
        Bp = (rng.random((8192, 128)) + 0.1).astype(np.float32)
        refp = Ap.astype(np.float64).T @ Bp.astype(np.float64)
        rel = {}
        for mode in ("native", "split"):
            hip.set_gemm_mode(mode)
            got = hip.gemm("tn", dev(Ap), dev(Bp)).cpu().numpy()
            rel[mode] = (got - refp) / refp
        assert np.max(np.abs(rel["native"])) < 2e-5 and abs(rel["native"].mean()) < 2e-6
        assert np.max(np.abs(rel["split"])) < 4e-5
    finally:
        hip.set_gemm_mode(start)


@pytest.mark.parametrize("n,F,lag,shift", [(5000, 64, 3, False), (3000, 54, 1, True), (40000, 256, 10, False),
                                           (20000, 128, 0, True), (1500, 300, 7, True), (40, 8, 39, False)])
def test_lagged_cov_vs_float64(n, F, lag, shift):
    from deep_cartograph_amd import hip

    X = rand_matrix(n, F, 3, scramble=shift)
    P = n - lag
    sh = X.mean(0).astype(np.float32) if shift else None
    raw = hip.lagged_cov_raw(dev(X), P, lag, dev(sh) if shift else None).cpu().numpy()
    Z = X.astype(np.float32) - (sh if shift else 0)
    Z = Z.astype(np.float64)  # the kernel subtracts in fp32
    zt, zl = Z[:P], Z[lag:lag + P]
    a, b = zt.sum(0), zl.sum(0)
    A = zt.T @ zt
    B = zt.T @ zl
    scale = np.sqrt(np.outer(np.diag(A), np.diag(A)))
    np.testing.assert_allclose(raw[:F], a, rtol=1e-9, atol=1e-6 * P)
    if lag:
        np.testing.assert_allclose(raw[F:2 * F], b, rtol=1e-9, atol=1e-6 * P)
    got_A = raw[2 * F:2 * F + F * F].reshape(F, F)
    got_B = raw[2 * F + F * F:].reshape(F, F)
    # fp32 products and chunked fp32 accumulation: relative to the diagonal scale
    assert np.max(np.abs(got_A - A) / scale) < 3e-6
    if lag:
        assert np.max(np.abs(got_B - B) / scale) < 3e-6
    else:
        assert np.all(got_B == 0)
    # deterministic
    raw2 = hip.lagged_cov_raw(dev(X), P, lag, dev(sh) if shift else None).cpu().numpy()
    np.testing.assert_array_equal(raw, raw2)


@pytest.mark.parametrize("n,F,d", [(164, 54, 2), (10000, 256, 4), (3000, 512, 3), (777, 100, 8), (5000, 1024, 16), (100, 64, 1)])
def test_project_linear(n, F, d):
    from deep_cartograph_amd import hip

    X = rand_matrix(n, F, 4)
    st = ol.feature_stats(X)
    m, r = ol.prepare_normalization(st, "mean_std")
    rng = np.random.Generator(np.random.PCG64(9))
    W = (rng.standard_normal((F, d)) / np.sqrt(F)).astype(np.float32)
    Xn = ol.normalize(X, m, r)
    cm, cr = ol.linear_cv_norm(Xn, W)
    ref = ol.project_linear(X, W, cm, cr, m, r)
    out, mm = hip.project_linear(dev(X), dev(W), fmean=dev(m.astype(np.float32)), frange=dev(r.astype(np.float32)),
                                 cvmean=dev(cm.astype(np.float32)), cvrange=dev(cr.astype(np.float32)), want_minmax=True)
    out = out.cpu().numpy()
    np.testing.assert_allclose(out, ref, atol=2e-5)  # |out| <= 1 after min-max normalisation
    np.testing.assert_allclose(mm.cpu().numpy(), np.stack([out.min(0), out.max(0)]), atol=0)
    # raw projection of already-normalised data + extrema only (normalize_cv path)
    _, mm2 = hip.project_linear(dev(Xn), dev(W), want_out=False, want_minmax=True)
    Praw = Xn.astype(np.float64) @ W.astype(np.float64)
    np.testing.assert_allclose(mm2.cpu().numpy(), np.stack([Praw.min(0), Praw.max(0)]), rtol=1e-5, atol=1e-5)


def test_kmeans_step_and_nearest(golden_cluster):
    from deep_cartograph_amd import hip

    for tag in ("syn_a", "syn_b", "syn_c"):
        P = golden_cluster[f"{tag}.points"]
        C = golden_cluster[f"{tag}.init"]
        mean = P.mean(0)
        Pd = dev(P)
        labels = torch.full((P.shape[0],), -1, dtype=torch.int32, device="cuda")
        acc, md = hip.kmeans_step(Pd, dev(C - mean), labels, offset=dev(mean), want_mindist=True)
        acc = acc.cpu().numpy()
        Xc = P - mean
        Cc = C - mean
        pw = (Cc * Cc).sum(1)[None, :] - 2.0 * (Xc @ Cc.T)
        ref_lab = pw.argmin(1)
        np.testing.assert_array_equal(labels.cpu().numpy(), ref_lab)
        k, d = C.shape
        sums = np.zeros((k, d))
        np.add.at(sums, ref_lab, Xc)
        np.testing.assert_allclose(acc[:k * d].reshape(k, d), sums, rtol=1e-12, atol=1e-9)
        np.testing.assert_array_equal(acc[k * d:k * d + k], np.bincount(ref_lab, minlength=k))
        ref_in = ((Xc - Cc[ref_lab]) ** 2).sum()
        np.testing.assert_allclose(acc[k * d + k], ref_in, rtol=1e-12)
        assert acc[k * d + k + 1] == P.shape[0]
        np.testing.assert_allclose(md.cpu().numpy(), ((Xc - Cc[ref_lab]) ** 2).sum(1), rtol=1e-12, atol=1e-15)
        # nearest sample of every centroid: bit-exact row indices vs np.linalg.norm / np.argmin
        cents = golden_cluster[f"{tag}.pp_centroids"]
        _, rows = hip.nearest_rows(Pd, dev(cents))
        np.testing.assert_array_equal(rows.cpu().numpy(), oc.find_centroid_rows(P, cents))
        # 1-NN label transfer
        sup = P[::37] + 1e-3
        nn = hip.nearest_point(Pd, dev(sup)).cpu().numpy()
        d2 = ((sup[:, None, :] - P[None, :, :]) ** 2).sum(-1)
        np.testing.assert_array_equal(nn, d2.argmin(1))


@pytest.mark.parametrize("d,k,n", [(4, 6, 200_003), (2, 3, 70_001), (4, 8, 63), (2, 1, 5_000), (4, 9, 30_000)])
def test_kmeans_pass_through_the_lds_ring(d, k, n):
    """The plain Lloyd pass (no per-point distances asked for) streams d = 2 / 4 points through the per-wave LDS-DMA ring
    (kmeans.hip: ring_stream): labels bit-exact against the sklearn formula in NumPy (first minimum wins), sums / counts /
    inertia / changed against NumPy, the same answers as the register pass (which reports the distances), ragged tails (n not
    a multiple of 64, fewer points than one chunk), an offset, k = 9 (the register kernel: more than 8 clusters)."""
    from deep_cartograph_amd import hip

    rng = np.random.Generator(np.random.PCG64(1000 + 10 * d + k))
    cent = rng.uniform(-1, 1, (k, d))
    P = np.round(cent[rng.integers(0, k, n)] + 0.15 * rng.standard_normal((n, d)), 4)
    C = P[rng.choice(n, k, replace=False)] + 1e-3
    mean = P.mean(0)
    Pd = dev(P)
    lab_ring = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    lab_reg = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    acc_ring, none = hip.kmeans_step(Pd, dev(C - mean), lab_ring, offset=dev(mean))
    acc_reg, md = hip.kmeans_step(Pd, dev(C - mean), lab_reg, offset=dev(mean), want_mindist=True)
    assert none is None
    Xc, Cc = P - mean, C - mean
    ref_lab = ((Cc * Cc).sum(1)[None, :] - 2.0 * (Xc @ Cc.T)).argmin(1)
    np.testing.assert_array_equal(lab_ring.cpu().numpy(), ref_lab)
    np.testing.assert_array_equal(lab_reg.cpu().numpy(), ref_lab)
    sums = np.zeros((k, d))
    np.add.at(sums, ref_lab, Xc)
    for acc in (acc_ring.cpu().numpy(), acc_reg.cpu().numpy()):
        np.testing.assert_allclose(acc[:k * d].reshape(k, d), sums, rtol=1e-12, atol=1e-9)
        np.testing.assert_array_equal(acc[k * d:k * d + k], np.bincount(ref_lab, minlength=k))
        np.testing.assert_allclose(acc[k * d + k], ((Xc - Cc[ref_lab]) ** 2).sum(), rtol=1e-12)
        assert acc[k * d + k + 1] == n
    again, _ = hip.kmeans_step(Pd, dev(C - mean), lab_ring, offset=dev(mean))      # idempotent, bit for bit
    again = again.cpu().numpy()
    assert again[k * d + k + 1] == 0
    np.testing.assert_array_equal(again[:k * d + k + 1], acc_ring.cpu().numpy()[:k * d + k + 1])


def test_nearest_rows_wide_d():
    """numpy's pairwise summation changes form at d >= 8."""
    from deep_cartograph_amd import hip

    rng = np.random.Generator(np.random.PCG64(3))
    for d in (8, 11, 16):
        P = np.round(rng.uniform(-1, 1, (4000, d)), 4)
        C = np.round(rng.uniform(-1, 1, (5, d)), 3)
        _, rows = hip.nearest_rows(dev(P), dev(C))
        np.testing.assert_array_equal(rows.cpu().numpy(), oc.find_centroid_rows(P, C))


@pytest.mark.parametrize("d,k", [(1, 3), (2, 6), (3, 11), (4, 6), (4, 17)])
def test_nearest_rows_one_pass_narrow_d(d, k):
    """d <= 4: ONE pass over the points for every chunk of 8 centroids (nearest_rows_multi_kernel).  Rows bit-exact against
    np.linalg.norm / argmin incl. exact ties (duplicated points: the first index wins) and centroids that ARE points; the
    per-centroid kernel (DCV_NEAREST_PER_CENTROID=1 in a fresh process would select it) is covered by the wide-d test."""
    from deep_cartograph_amd import hip

    rng = np.random.Generator(np.random.PCG64(100 + 10 * d + k))
    P = np.round(rng.uniform(-1, 1, (150_001, d)), 4)      # %.4f CSV values, as the pipeline hands them over
    P[70_000:70_050] = P[10_000:10_050]                   # exact duplicates: ties in every distance
    C = np.round(rng.uniform(-1, 1, (k, d)), 3)
    C[0] = P[70_010]                                       # distance 0, reached at two rows: row 10 010 must win
    dist, rows = hip.nearest_rows(dev(P), dev(C))
    ref = oc.find_centroid_rows(P, C)
    np.testing.assert_array_equal(rows.cpu().numpy(), ref)
    assert rows[0].item() == 10_010
    np.testing.assert_array_equal(dist.cpu().numpy(), np.linalg.norm(P[ref] - C, axis=1))
    # a row offset (frame-sharded callers) shifts the reported rows only
    _, rows_o = hip.nearest_rows(dev(P), dev(C), row_offset=1_000_000)
    np.testing.assert_array_equal(rows_o.cpu().numpy(), ref + 1_000_000)


def _lloyd_case(d, k, n):
    """Points, start centres and mean of a Lloyd-pass case whose argmin does not hang on the last bit: for every point the
    two smallest |c|^2 - 2 x.c are more than 1e-9 apart and the argmin is the same whether the dot product is summed by BLAS,
    sequentially, or sequentially with fused multiply-adds (where Python has math.fma) -- checked here, on the CPU."""
    import math

    rng = np.random.Generator(np.random.PCG64(2000 + 10 * d + k))
    cent = rng.uniform(-1, 1, (k, d))
    P = np.round(cent[rng.integers(0, k, n)] + 0.15 * rng.standard_normal((n, d)), 4)
    C = P[rng.choice(n, k, replace=False)] + 1e-3
    mean = P.mean(0)
    Xc, Cc = P - mean, C - mean
    cn = (Cc * Cc).sum(1)
    pw = cn[None, :] - 2.0 * (Xc @ Cc.T)
    ref_lab = pw.argmin(1)
    two = np.sort(pw, axis=1)[:, :2]
    assert (two[:, 1] - two[:, 0]).min() > 1e-9
    dot = np.zeros((n, k))
    for c in range(d):
        dot = dot + Xc[:, c, None] * Cc[None, :, c]
    np.testing.assert_array_equal((cn[None, :] - 2.0 * dot).argmin(1), ref_lab)
    if hasattr(math, "fma"):
        dotf = np.zeros((n, k))
        for i in range(n):
            for j in range(k):
                s = 0.0
                for c in range(d):
                    s = math.fma(Xc[i, c], Cc[j, c], s)
                dotf[i, j] = s
        np.testing.assert_array_equal((cn[None, :] - 2.0 * dotf).argmin(1), ref_lab)
    return P, C, mean, ref_lab


@pytest.mark.parametrize("d,k,n", [(1, 2, 1_025), (3, 17, 777), (5, 3, 1_000), (8, 9, 300), (16, 64, 2_049)])
def test_kmeans_step_general_kernel_and_odd_d(d, k, n):
    """The Lloyd pass outside d = 2 / 4: the general kernel with per-wave LDS accumulators (k > 16 or d > 4, even and odd d:
    the 16-byte and the scalar point load) and the register kernel at d = 1.  Labels bit-exact against the sklearn formula in
    NumPy, counts exact, sums / inertia / per-point distances against NumPy, every label changed on the first call and none
    on the second."""
    from deep_cartograph_amd import hip

    P, C, mean, ref_lab = _lloyd_case(d, k, n)
    Xc, Cc = P - mean, C - mean
    Pd = dev(P)
    labels = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    acc, md = hip.kmeans_step(Pd, dev(Cc), labels, offset=dev(mean), want_mindist=True)
    acc = acc.cpu().numpy()
    np.testing.assert_array_equal(labels.cpu().numpy(), ref_lab)
    sums = np.zeros((k, d))
    np.add.at(sums, ref_lab, Xc)
    np.testing.assert_allclose(acc[:k * d].reshape(k, d), sums, rtol=1e-12, atol=1e-9)
    np.testing.assert_array_equal(acc[k * d:k * d + k], np.bincount(ref_lab, minlength=k))
    np.testing.assert_allclose(acc[k * d + k], ((Xc - Cc[ref_lab]) ** 2).sum(), rtol=1e-12)
    np.testing.assert_allclose(md.cpu().numpy(), ((Xc - Cc[ref_lab]) ** 2).sum(1), rtol=1e-12, atol=1e-15)
    assert acc[k * d + k + 1] == n
    again, _ = hip.kmeans_step(Pd, dev(Cc), labels, offset=dev(mean), want_mindist=True)
    assert again.cpu().numpy()[k * d + k + 1] == 0
    np.testing.assert_array_equal(labels.cpu().numpy(), ref_lab)


@pytest.mark.parametrize("d", [1, 2, 5, 8, 16])
def test_kmeanspp_passes_even_and_odd_d(d):
    """k-means++ seeding passes with an offset: closest = max(0, -2 x.c + |c|^2 + |x|^2) for the first centre, its running
    minimum for a second one, the potential each update returns, and the potentials of three candidates.  The centres are
    drawn independently of the points: at a centre that IS a point the three terms cancel to rounding noise of one ulp of
    |x|^2 (1.8e-15 at d = 16, measured on the first run of this test), which depends on the order of summation and lies
    outside atol = 1e-15; away from the points rtol covers that ulp."""
    from deep_cartograph_amd import hip

    n = 1_537
    rng = np.random.Generator(np.random.PCG64(3000 + d))
    P = np.round(rng.uniform(-1, 1, (n, d)), 4)
    mean = P.mean(0)
    X = P - mean

    def dist(c):
        return np.maximum(0.0, -2.0 * (X @ c) + (c * c).sum() + (X * X).sum(1))

    c0, c1 = rng.uniform(-1, 1, d) - mean, rng.uniform(-1, 1, d) - mean
    cand = rng.uniform(-1, 1, (3, d)) - mean
    Pd, off = dev(P), dev(mean)
    closest = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    pot = hip.kmeanspp_update(Pd, dev(c0), closest, True, offset=off)
    ref = dist(c0)
    np.testing.assert_allclose(closest.cpu().numpy(), ref, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(pot.cpu().numpy(), [ref.sum()], rtol=1e-12)
    pots = hip.kmeanspp_potentials(Pd, dev(cand), closest, offset=off)
    np.testing.assert_allclose(pots.cpu().numpy(), [np.minimum(ref, dist(c)).sum() for c in cand], rtol=1e-12)
    pot = hip.kmeanspp_update(Pd, dev(c1), closest, False, offset=off)
    ref = np.minimum(ref, dist(c1))
    np.testing.assert_allclose(closest.cpu().numpy(), ref, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(pot.cpu().numpy(), [ref.sum()], rtol=1e-12)


_REG_STREAM_NEAREST = [(4, 6, 70_001), (2, 3, 5_000), (4, 17, 63)] + [(d, k, ko.NEAREST_STEADY_N) for d, k in ko.OTHER_STREAM_NEAREST_DK]
_REG_STREAM_LLOYD = [(4, 6, 70_001)] + [(d, k, ko.LLOYD_STEADY_N) for d, k in ko.OTHER_STREAM_LLOYD_DK]
_REG_STREAM_CHILD_SECONDS = 5   # measured: see test_register_stream_matches_ring_and_numpy


def _reg_stream_inputs():
    """The point sets of the register-stream test, with duplicated rows (exact ties) and a centroid that IS a point, as
    test_nearest_rows_one_pass_narrow_d builds them; the same in the parent and the child process.  The steady-state sizes
    (tests/kmeans_oracle.py: more than 1024 points per workgroup, so that the register stream alternates its batches) come
    from the oracle module's recipes and seeds.  Lloyd cases are (P, C, mean); the first one runs without an offset."""
    cases = []
    for d, k, n in _REG_STREAM_NEAREST:
        if n == ko.NEAREST_STEADY_N:
            cases.append(ko.nearest_case(d, k, n, ko.nearest_seed(d, k, n))[:2])
            continue
        rng = np.random.Generator(np.random.PCG64(4000 + 10 * d + k))
        P = np.round(rng.uniform(-1, 1, (n, d)), 4)
        m = min(50, n // 4)
        P[n // 2:n // 2 + m] = P[n // 8:n // 8 + m]
        C = np.round(rng.uniform(-1, 1, (k, d)), 3)
        C[0] = P[n // 2 + m // 5]
        cases.append((P, C))
    lloyd = []
    for d, k, n in _REG_STREAM_LLOYD:
        if n == ko.LLOYD_STEADY_N:
            lloyd.append(ko.lloyd_case(d, k, n, ko.lloyd_seed(d, k, n)))
            continue
        rng = np.random.Generator(np.random.PCG64(4500))
        cent = rng.uniform(-1, 1, (k, d))
        P = np.round(cent[rng.integers(0, k, n)] + 0.15 * rng.standard_normal((n, d)), 4)
        P[n // 2:n // 2 + 50] = P[n // 8:n // 8 + 50]
        C = P[rng.choice(n, k, replace=False)] + 1e-3
        lloyd.append((P, C, None))
    return cases, lloyd


def _reg_stream_run(inputs=None):
    """rows / distances of every nearest-rows case and labels / acc of every Lloyd case, through whichever stream the
    process's DCV_KM_RING selects."""
    from deep_cartograph_amd import hip

    cases, lloyd = inputs or _reg_stream_inputs()
    out = {}
    for q, (Pn, Cn) in enumerate(cases):
        dist, rows = hip.nearest_rows(dev(Pn), dev(Cn))
        out[f"dist{q}"], out[f"rows{q}"] = dist.cpu().numpy(), rows.cpu().numpy()
    for q, (P, C, mean) in enumerate(lloyd):
        labels = torch.full((P.shape[0],), -1, dtype=torch.int32, device="cuda")
        if mean is None:
            acc, _ = hip.kmeans_step(dev(P), dev(C), labels)
        else:
            acc, _ = hip.kmeans_step(dev(P), dev(C - mean), labels, offset=dev(mean))
        sfx = "" if q == 0 else str(q)
        out["labels" + sfx], out["acc" + sfx] = labels.cpu().numpy(), acc.cpu().numpy()
    return out


_REG_STREAM_SCRIPT = """
import importlib.util
import sys
import time
sys.path.insert(0, sys.argv[1])
import numpy as np
spec = importlib.util.spec_from_file_location("kernels_gpu_cases", sys.argv[3])
tk = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tk)
np.savez(sys.argv[2], **tk._reg_stream_run())
print("child seconds %.1f" % (time.time() - float(sys.argv[4])))
"""


def test_register_stream_matches_ring_and_numpy(tmp_path):
    """DCV_KM_RING=0 in a fresh process selects the register stream (kmeans.hip: reg_stream) where this process takes the
    LDS-DMA ring: nearest_rows (four points per thread and batch) at d = 4 (the lane-pair path; 17 centroids in three chunks
    on fewer points than one 64-point chunk) and d = 2, and the Lloyd pass at d = 4 (two points, the labels travel along).
    Rows and distances bit-equal to np.linalg.norm / argmin and to the ring's, labels equal to the ring's.

    The steady-state sizes besides: nearest_rows at n = 4 300 003 (five batches per thread: ba, bb, ba, bb, ba, the planted
    duplicates in the last) and the plain Lloyd pass at n = 2 400 011 (five batches of two points).  Labels, counts, sums
    and inertia of BOTH processes against tests/kmeans_oracle.py (sums within the summation-tree bound L 2^-53 S derived
    in tests/test_kmeans_streams_gpu.py).  One child, started once; this process computes the references while it runs.
    The child took 5.0 s from its launch to the end of its work, measured on an MI355X machine (it prints the figure);
    its limit is four times that."""
    import os
    import subprocess
    import sys
    import time

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.environ.get("DCV_KM_RING", "1") != "0"
    inputs = _reg_stream_inputs()
    cases, lloyd = inputs
    ring = _reg_stream_run(inputs)
    script = tmp_path / "reg_stream.py"
    script.write_text(_REG_STREAM_SCRIPT)
    env = dict(os.environ)
    env["DCV_KM_RING"] = "0"
    out = tmp_path / "reg.npz"
    started = time.time()
    child = subprocess.Popen([sys.executable, str(script), root, str(out), os.path.abspath(__file__), repr(started)], env=env, cwd=root,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        near_refs = [oc.find_centroid_rows(P, C) for P, C in cases]
        lloyd_refs = [ko.lloyd_reference(P, C, np.zeros(P.shape[1]) if mean is None else mean) for P, C, mean in lloyd]
        stdout, stderr = child.communicate(timeout=max(1.0, 4 * _REG_STREAM_CHILD_SECONDS - (time.time() - started)))
    except BaseException:
        child.kill()
        child.communicate()
        raise
    assert child.returncode == 0, stderr[-2000:]
    print(stdout.strip())
    reg = np.load(out)
    for q, (P, C) in enumerate(cases):
        ref = near_refs[q]
        ref_dist = np.linalg.norm(P[ref] - C, axis=1)
        for got in (reg, ring):
            np.testing.assert_array_equal(got[f"rows{q}"], ref)
            np.testing.assert_array_equal(got[f"dist{q}"], ref_dist)
        assert reg[f"dist{q}"].tobytes() == ring[f"dist{q}"].tobytes()
    np.testing.assert_array_equal(reg["labels"], ring["labels"])
    assert reg["labels"].min() >= 0
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    for q, (P, C, mean) in enumerate(lloyd):
        n, d = P.shape
        k = C.shape[0]
        ref = lloyd_refs[q]
        assert ref.margin > 1e-9   # every label decided whatever the order of a dot product
        L = ko.lloyd_chain(n, cus)
        sfx = "" if q == 0 else str(q)
        for got in (reg, ring):
            np.testing.assert_array_equal(got["labels" + sfx], ref.labels)
            acc = got["acc" + sfx]
            np.testing.assert_array_equal(acc[k * d:k * d + k], ref.counts)
            assert acc[k * d + k + 1] == n
            ok, err = ko.within_sum_bound(acc[:k * d].reshape(k, d), ref.sums, ref.abs_sums, L)
            assert ok, (L, err)
            ok, err = ko.within_sum_bound(acc[k * d + k], ref.inertia, ref.inertia, L)
            assert ok, (L, err)


@pytest.mark.parametrize("d,bins,blocks", [(1, 150, 1), (2, 100, 1), (2, 64, 4), (1, 5000, 1)])
def test_fes_binned_kde_matches_oracle(d, bins, blocks):
    """f4, FES half: dcv_linear_binning + statistics.compute_fes against the NumPy restatement of the same binned KDE
    (oracle/fes.py): node weights to 1e-9 (64-bit fixed-point accumulation, 2^-36 per contribution), FES to 1e-6 kJ/mol;
    identical grids from two runs (integer atomics commute)."""
    from deep_cartograph_amd import hip, statistics
    from oracle import fes as ofes

    rng = np.random.Generator(np.random.PCG64(11))
    X = np.concatenate([rng.normal(-0.4, 0.12, (40_000, d)), rng.normal(0.45, 0.2, (60_000, d))]).clip(-1.2, 1.2)
    lo, hi = [-1.0] * d, [1.0] * d
    P = torch.from_numpy(X).cuda()
    w1, out1 = hip.linear_binning(P, list(range(d)), lo, hi, bins)
    w2, _ = hip.linear_binning(P, list(range(d)), lo, hi, bins)
    assert torch.equal(w1, w2)
    exp = ofes.linear_binning(X, lo, hi, bins)
    assert out1 == int(np.sum(np.any((X < -1.0) | (X > 1.0), axis=1)))
    np.testing.assert_allclose(w1.cpu().numpy(), exp, atol=1e-9 * X.shape[0])
    fes, grid, bounds, err = statistics.compute_fes(X, 300.0, 0.05, bins, blocks=blocks, bounds=list(zip(lo, hi)))
    assert fes.shape == (bins,) * d and err.shape == fes.shape and abs(fes.min()) < 1e-12
    if blocks == 1:
        ref = ofes.binned_fes(X, 300.0, 0.05, bins, lo, hi)
        np.testing.assert_allclose(fes, ref, atol=1e-6)
    else:
        assert np.all(err >= 0) and np.isfinite(err).all()
