"""The four streaming kernels every calculator goes through before a model is fitted -- dcv_col_stats, dcv_normalize
(csrc/stats.hip), dcv_lagged_cov (cov.hip) and dcv_project_linear (project.hip) -- against float64 NumPy, on the inputs
tests/test_kernels_gpu.py never hands them: row-major VIEWS of a wider matrix (row stride != width, misaligned base), the
dispatch paths that test reaches zero or one time, and the run-time switches.
Method: a view lives inside a parent buffer whose every other element is NaN (View).  A column or row outside the view
that reaches a stored result shows as NaN; after the call every element outside the view must still be NaN, so a store
outside the view is caught without any fault -- it lands in memory the test owns.  Each case is the smallest shape that
reaches the path it is named for; the path is proved from the launch-plan log (hip.gemm_log), or from the dispatch
condition restated on the tensors at hand (*_path below) and, where the CU count enters, asserted from it.
Tolerances are the project's own (test_kernels_gpu.py) or derived (project_bound); the tests print the figures they
assert.  Run on the GPU box: python -m pytest tests -m gpu"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev(a):
    return torch.as_tensor(a).cuda()


def rand_matrix(n, F, seed, scramble=True):
    """test_kernels_gpu.rand_matrix: per-column scale 0.1..10 and offset -5..5 when scrambled"""
    rng = np.random.Generator(np.random.PCG64(seed))
    X = rng.standard_normal((n, F)).astype(np.float32)
    if scramble:
        X = X * rng.uniform(0.1, 10, F).astype(np.float32) + rng.uniform(-5, 5, F).astype(np.float32)
    return X


# ------------------------------------------------------------------------------------------------ guard-banded views
VIEW_KINDS = ("contiguous", "wide", "wide4", "offset", "oddld")


class View:
    """An [n, F] float32 matrix on the device inside a NaN-filled parent of n + guard_rows rows:
      contiguous  parent width F: row stride F, 16-byte aligned base, guard rows behind the last row only
      wide        parent width F + 8: aligned base, a row stride that is a multiple of 4 when F is
      wide4       F % 4 != 0, parent width roundup(F, 4) + 4: aligned base, stride % 4 == 0 around a ragged width
      offset      as wide, but the parent starts one float into its buffer: data_ptr() % 16 == 4
      oddld       F % 4 == 0, parent width F + 3: aligned base, odd row stride
    `a` = None leaves the view itself NaN as well (an output).  .t is the view, guard_intact() whether every element
    outside it is still NaN."""

    def __init__(self, a, kind, n=None, F=None, guard_rows=3):
        if a is not None:
            n, F = a.shape
        if kind == "contiguous":
            W = F
        elif kind in ("wide", "offset"):
            W = F + 8
        elif kind == "wide4":
            assert F % 4 != 0
            W = (F + 3) // 4 * 4 + 4
        elif kind == "oddld":
            assert F % 4 == 0
            W = F + 3
        else:
            raise ValueError(kind)
        self.kind, self.rows, self.off = kind, n + guard_rows, 1 if kind == "offset" else 0
        self.flat = torch.full((self.off + self.rows * W,), NAN, dtype=torch.float32, device="cuda")
        self.t = self._carve(self.flat, n, F, W)
        self.inside = torch.zeros(self.flat.shape, dtype=torch.bool, device="cuda")
        self._carve(self.inside, n, F, W).fill_(True)
        assert self.t.stride() == (W, 1) and self.t.data_ptr() % 16 == 4 * self.off
        assert n == 1 or self.t.is_contiguous() == (kind == "contiguous")
        if a is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        assert int(self.inside.sum()) == n * F and self.guard_intact()

    def _carve(self, flat, n, F, W):
        return flat[self.off:].view(self.rows, W)[:n, :F]

    def guard_intact(self):
        return bool(torch.isnan(self.flat[~self.inside]).all())

    def host(self):
        return self.t.cpu().numpy()


def quad_loads(t, F=None):
    """The kernels' condition for 16-byte accesses to a matrix: width and row stride multiples of 4, base aligned"""
    F = t.shape[1] if F is None else F
    return F % 4 == 0 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0


def test_view_kinds_are_what_they_are_named_for():
    X = rand_matrix(5, 12, 0)
    for kind, want in (("contiguous", True), ("wide", True), ("offset", False), ("oddld", False)):
        v = View(X, kind)
        assert quad_loads(v.t) == want, kind
        np.testing.assert_array_equal(v.host(), X)
    v = View(rand_matrix(5, 10, 0), "wide4")
    assert v.t.stride(0) == 16 and v.t.data_ptr() % 16 == 0 and not quad_loads(v.t)
    v.flat[3] = 1.0   # the view's first row ends at element 9; 10..15 are guard
    assert v.guard_intact()
    v.flat[11] = 1.0
    assert not v.guard_intact()


# ------------------------------------------------------------------------------------------------ col_stats
# (n, F, view, 16-byte loads, what the shape reaches).  stats.hip: ng = F / VEC column groups, cpb = min(ng, 256) of them
# per pass, rpp = 256 / cpb row lanes, blocks = min(ceil(n / 64), 2048)
COL_STATS = [
    (1000, 100, "contiguous", True, "VEC=4, ng = 25 does not divide 256: 6 idle threads"),
    (1000, 100, "wide", True, "the same at ld = 108"),
    (130, 1028, "contiguous", True, "VEC=4, ng = 257: ragged second column pass"),
    (130, 1028, "wide", True, "the same at ld = 1036"),
    (200, 300, "contiguous", True, "VEC=4, ng = 75"),
    (200, 300, "offset", False, "VEC=1 because of the pointer, F > 256: ragged second column pass"),
    (200, 257, "contiguous", False, "VEC=1 because of F, second column pass of one column"),
    (500, 64, "contiguous", True, "VEC=4, ng = 16"),
    (500, 64, "oddld", False, "VEC=1 because of ld = 67"),
    (200, 2048, "contiguous", True, "rpp = 1, 50 rows per block: 48 in the 4-row unroll, 2 in the tail loop"),
    (131073, 4, "contiguous", True, "2048 blocks of 65 rows: blocks 2017.. hold no row; ng = 1, 256 row lanes"),
    (131073, 8, "contiguous", True, "the same at ng = 2"),
    (1, 12, "contiguous", True, "one row"), (1, 12, "wide", True, "one row"),
    (2, 12, "contiguous", True, "two rows"), (2, 12, "wide", True, "two rows"),
    (3, 12, "contiguous", True, "three rows"), (3, 12, "wide", True, "three rows"),
]


@pytest.mark.parametrize("n,F,kind,vec,what", COL_STATS, ids=[f"{c[0]}x{c[1]}-{c[2]}" for c in COL_STATS])
def test_col_stats_views_and_paths(n, F, kind, vec, what):
    from deep_cartograph_amd import hip

    X = rand_matrix(n, F, 11)
    v = View(X, kind)
    assert quad_loads(v.t) == vec, what
    raw = hip.col_stats_raw(v.t).cpu().numpy()
    X64 = X.astype(np.float64)
    s, q = X64.sum(0), (X64 * X64).sum(0)
    print(f"col_stats {n} x {F} {kind}: sum {np.max(np.abs(raw[0] - s) / (1e-9 + 1e-12 * np.abs(s))):.1e} of atol 1e-9 + rtol 1e-12, "
          f"sum of squares {np.max(np.abs(raw[1] - q) / q):.1e} relative (rtol 1e-12)")
    np.testing.assert_allclose(raw[0], s, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(raw[1], q, rtol=1e-12)
    np.testing.assert_array_equal(raw[2], X64.min(0))
    np.testing.assert_array_equal(raw[3], X64.max(0))
    assert v.guard_intact()
    np.testing.assert_array_equal(v.host(), X)   # an input


# ------------------------------------------------------------------------------------------------ normalize
def normalize_path(X, out, mean, rng):
    """dcv_normalize's dispatch (stats.hip), restated: 'rows' (normalize_rows_kernel), 'flat4' / 'flat1' (normalize_kernel)"""
    F = X.shape[1]
    if not (quad_loads(X) and quad_loads(out) and mean.data_ptr() % 16 == 0 and rng.data_ptr() % 16 == 0):
        return "flat1"
    ng = F // 4
    if os.environ.get("DCV_NORMALIZE_FLAT", "")[:1] == "1":
        return "flat4"
    return "rows" if ng <= 256 and 256 % ng == 0 else "flat4"


def rows_per_block(F):
    """normalize_rows_kernel: 256 / ng row lanes, four rounds of eight rows each.  A store a row lane should have masked
    lands less than half a block behind the last row: with this many guard rows behind an output it stays in the parent."""
    return 32 * max(1, 256 // max(F // 4, 1))


def norm_inputs(n, F, seed=12):
    X = rand_matrix(n, F, seed)
    m = X.mean(0, dtype=np.float64).astype(np.float32)
    r = (X.std(0, dtype=np.float64) + 0.25).astype(np.float32)
    return X, m, r, ((X - m) / r).astype(np.float32)   # NumPy float32: IEEE round-to-nearest subtraction and division


ARRANGEMENTS = ("wide-to-contiguous", "contiguous-to-wide", "inplace-wide", "inplace-contiguous")


def run_normalize(X, m, r, arrangement, path=None):
    """one call in the named arrangement of input and output; (result, every guard band intact)"""
    from deep_cartograph_amd import hip

    n, F = X.shape
    g = rows_per_block(F)
    md, rd = dev(m), dev(r)
    if arrangement == "wide-to-contiguous":
        x, o = View(X, "wide"), View(None, "contiguous", n, F, guard_rows=g)
    elif arrangement == "contiguous-to-wide":
        x, o = View(X, "contiguous"), View(None, "wide", n, F, guard_rows=g)
    else:
        x = View(X, "wide" if arrangement == "inplace-wide" else "contiguous", guard_rows=g)
        o = x
    if path is not None:
        assert normalize_path(x.t, o.t, md, rd) == path
    ret = hip.normalize(x.t, md, rd, out=o.t)
    assert ret is o.t
    ok = x.guard_intact() and o.guard_intact()
    if o is not x:
        ok = ok and bool(torch.equal(x.t.cpu(), torch.from_numpy(X)))
    return o.host(), ok


# (F, n, path): rows kernel at ng = 1 (8192 rows per block: fewer rows than row lanes; one row into a second block),
# ng = 16 (512 rows per block: a ragged only block; one row into a second), ng = 256 (one row lane, 32 rows per block);
# the flat kernels at ng = 25 (256 % ng != 0) and ng = 512 (> 256) and at a width that is no multiple of 4
NORMALIZE = [(4, 100, "rows"), (4, 8193, "rows"), (64, 259, "rows"), (64, 513, "rows"), (1024, 7, "rows"), (1024, 33, "rows"),
             (100, 37, "flat4"), (2048, 37, "flat4"), (54, 37, "flat1")]


@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
@pytest.mark.parametrize("F,n,path", NORMALIZE, ids=[f"{c[1]}x{c[0]}" for c in NORMALIZE])
def test_normalize_bit_equal_on_views(F, n, path, arrangement):
    assert os.environ.get("DCV_NORMALIZE_FLAT", "")[:1] != "1" and os.environ.get("DCV_NORMALIZE_RPB") is None
    X, m, r, ref = norm_inputs(n, F)
    got, guards = run_normalize(X, m, r, arrangement, path)
    np.testing.assert_array_equal(got, ref)
    assert guards


@pytest.mark.parametrize("why", ["offset-X", "oddld-out", "misaligned-mean", "misaligned-range"])
def test_normalize_scalar_form_because_of_an_operand(why):
    """F = 64 qualifies for the rows kernel; one operand that does not allow 16-byte accesses sends the call to the scalar
    flat kernel (a 16-byte access at such an address faults or, worse, reads the neighbouring quad)."""
    from deep_cartograph_amd import hip

    n, F = 300, 64
    X, m, r, ref = norm_inputs(n, F)
    x = View(X, "offset" if why == "offset-X" else "contiguous")
    o = View(None, "oddld" if why == "oddld-out" else "contiguous", n, F, guard_rows=rows_per_block(F))
    md, rd = dev(m), dev(r)
    if why == "misaligned-mean":
        buf = torch.full((F + 2,), NAN, dtype=torch.float32, device="cuda")
        md = buf[1:F + 1]
        md.copy_(torch.from_numpy(m))
    if why == "misaligned-range":
        buf = torch.full((F + 2,), NAN, dtype=torch.float32, device="cuda")
        rd = buf[1:F + 1]
        rd.copy_(torch.from_numpy(r))
    assert normalize_path(x.t, o.t, md, rd) == "flat1"
    assert normalize_path(View(X, "contiguous").t, View(None, "contiguous", n, F).t, dev(m), dev(r)) == "rows"
    hip.normalize(x.t, md, rd, out=o.t)
    np.testing.assert_array_equal(o.host(), ref)
    assert x.guard_intact() and o.guard_intact()


# ------------------------------------------------------------------------------------------------ lagged_cov
def cov_inputs(P, F, lag, shift, seed=13):
    """test_lagged_cov_vs_float64's data: scrambled columns with their float32 mean as the shift, plain normals without"""
    X = rand_matrix(P + lag, F, seed, scramble=shift)
    sh = X.mean(0).astype(np.float32) if shift else None
    return X, sh


def cov_check(raw, X, sh, P, lag, tag=""):
    """test_lagged_cov_vs_float64's oracle: the shift subtracted in float32, everything after it in float64; a, b to
    rtol 1e-9 / atol 1e-6 P, A and B to 3e-6 of sqrt(A_ii A_jj), B == 0 exactly at lag 0.  Returns the worst scaled error."""
    F = X.shape[1]
    Z = (X - (sh if sh is not None else 0)).astype(np.float32).astype(np.float64)
    zt, zl = Z[:P], Z[lag:lag + P]
    A, B = zt.T @ zt, zt.T @ zl
    scale = np.sqrt(np.outer(np.diag(A), np.diag(A)))
    got_A = raw[2 * F:2 * F + F * F].reshape(F, F)
    got_B = raw[2 * F + F * F:].reshape(F, F)
    eA = np.max(np.abs(got_A - A) / scale)
    eB = np.max(np.abs(got_B - B) / scale) if lag else 0.0
    ea = np.max(np.abs(raw[:F] - zt.sum(0)))
    eb = np.max(np.abs(raw[F:2 * F] - zl.sum(0))) if lag else 0.0
    print(f"lagged_cov {tag} P={P} F={F} lag={lag}: A {eA:.2e} B {eB:.2e} of sqrt(A_ii A_jj) (bound 3e-6); "
          f"a {ea:.2e} b {eb:.2e} absolute (atol {1e-6 * P:.1e})")
    assert np.isfinite(raw).all()
    np.testing.assert_allclose(raw[:F], zt.sum(0), rtol=1e-9, atol=1e-6 * P)
    if lag:
        np.testing.assert_allclose(raw[F:2 * F], zl.sum(0), rtol=1e-9, atol=1e-6 * P)
        assert eB < 3e-6
    else:
        assert np.all(raw[F:2 * F] == 0) and np.all(got_B == 0)
    assert eA < 3e-6
    return max(eA, eB)


def run_cov(X, sh, P, lag, kind):
    """(raw sums, launch log, view): the view has exactly P + lag rows, the guard rows follow them"""
    from deep_cartograph_amd import hip

    v = View(X, kind)
    shd = dev(sh) if sh is not None else None
    hip.gemm_log_reset()
    raw = hip.lagged_cov_raw(v.t, P, lag, shd)
    log = hip.gemm_log()
    raw2 = hip.lagged_cov_raw(v.t, P, lag, shd)
    assert torch.equal(raw, raw2)   # deterministic, bit for bit
    assert v.guard_intact()
    assert torch.equal(v.t.cpu(), torch.from_numpy(X))
    return raw.cpu().numpy(), log, v


# (P, F, lag, shift, view, property of the one logged launch)
LAGGED_COV = [
    # F = 130 at ld = 136, aligned: 16-byte loads whose last quad straddles column F and pulls the guard band's NaNs into the
    # out-of-range part of the second column tile; 2 x 2 tiles; two chunks, the last 5 rows long (under one stage)
    (2053, 130, 3, True, "wide4", lambda e: e.vec and e.splits == 2),
    (2053, 130, 3, True, "contiguous", lambda e: not e.vec and e.splits == 2),     # ld = 130: the scalar form of the same
    # eight chunks of 1280 rows, the last 40: the XCD-aware map; no shift: the float64 statistics pass gives a and b
    (9000, 64, 5, False, "wide", lambda e: e.vec and e.splits % 8 == 0 and e.splits > 0),
    (4100, 128, 16, True, "offset", lambda e: not e.vec),     # one dense tile, shift subtracted at store time
    (4100, 128, 16, True, "contiguous", lambda e: e.vec),     # one dense tile, shift subtracted on the DMA path's fragments
    (3000, 132, 0, True, "wide", lambda e: e.vec),            # lag 0 on a view: one product, B == 0
    (70, 1, 2, True, "contiguous", lambda e: not e.vec and e.splits == 1),         # one column
]


@pytest.mark.parametrize("P,F,lag,shift,kind,named", LAGGED_COV, ids=[f"{c[0]}x{c[1]}-lag{c[2]}-{c[4]}" for c in LAGGED_COV])
def test_lagged_cov_views_and_plans(P, F, lag, shift, kind, named):
    X, sh = cov_inputs(P, F, lag, shift)
    raw, log, v = run_cov(X, sh, P, lag, kind)
    assert len(log) == 1, log
    e = log[0]
    print("plan:", tuple(e))
    assert e.form == "single" and e.mode == "tn" and (e.tm, e.tn) == (128, 128) and not e.split, e
    assert named(e), e
    cov_check(raw, X, sh, P, lag, kind)


@pytest.mark.parametrize("shift", [True, False], ids=["shift", "noshift"])
@pytest.mark.parametrize("P,F,lag", [(100, 8, 200), (1000, 12, 4000)])
def test_lagged_cov_lag_longer_than_the_pairs(P, F, lag, shift):
    """A short trajectory at a long lag: the statistics passes over the `lag` head and tail rows take more blocks than the
    pass over the pairs (4 against 2 at 100 pairs, lag 200), and all three share one workspace."""
    X, sh = cov_inputs(P, F, lag, shift)
    raw, log, _ = run_cov(X, sh, P, lag, "contiguous")
    assert len(log) == 1 and log[0].splits == 1, log
    cov_check(raw, X, sh, P, lag, "long lag")


# ------------------------------------------------------------------------------------------------ project_linear
def project_inputs(n, F, d, seed=14):
    rng = np.random.Generator(np.random.PCG64(seed + 7 * F + d))
    X = rand_matrix(n, F, seed)
    W = (rng.standard_normal((F, d)) / np.sqrt(F)).astype(np.float32)
    fm = X.mean(0, dtype=np.float64).astype(np.float32)
    fr = (X.std(0, dtype=np.float64) + 0.25).astype(np.float32)
    bias = rng.uniform(-1, 1, d).astype(np.float32)
    cm = rng.uniform(-0.5, 0.5, d).astype(np.float32)
    cr = rng.uniform(0.5, 3.0, d).astype(np.float32)
    return X, W, fm, fr, bias, cm, cr


def project_ref(X, W, fm=None, fr=None, bias=None, cm=None, cr=None):
    """(ref, bound) in float64.  xn is the float32 IEEE-normalised input the kernel forms (bit for bit: see normalize),
    y = xn @ W + bias, ref = (y - cvmean) / cvrange.  The kernel's float32 chain of products errs by at most
    4e-7 * S, S = |xn| @ |W| + |bias| (test_gemm_random_fp32's bound for an fp32 fma chain); the subtraction of cvmean
    rounds once (1.2e-7 = 2^-23 of its larger operand, itself known to that error), the division scales both and rounds
    once more."""
    xn = ((X - fm) / fr).astype(np.float32) if fm is not None else X
    xn, W64 = xn.astype(np.float64), W.astype(np.float64)
    b = bias.astype(np.float64) if bias is not None else np.zeros(W.shape[1])
    m = cm.astype(np.float64) if cm is not None else np.zeros(W.shape[1])
    r = cr.astype(np.float64) if cr is not None else np.ones(W.shape[1])
    y = xn @ W64 + b
    S = np.abs(xn) @ np.abs(W64) + np.abs(b)
    ref = (y - m) / r
    bound = (4e-7 * S + 1.2e-7 * (np.abs(y) + np.abs(m))) / np.abs(r) + 1.2e-7 * np.abs(ref)
    return ref, bound


def project_check(out, mm, ref, bound, tag):
    ratio = np.max(np.abs(out - ref) / bound)
    print(f"project_linear {tag}: worst error / bound {ratio:.3f}, worst error {np.max(np.abs(out - ref)):.2e}")
    assert np.all(np.abs(out - ref) <= bound)
    if mm is not None:
        np.testing.assert_array_equal(mm, np.stack([out.min(0), out.max(0)]))
    return ratio


def gpu_vectors(**kw):
    return {k: (dev(v) if v is not None else None) for k, v in kw.items()}


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("d", [1, 3, 5, 9, 15])
def test_project_linear_every_width_with_bias(d, norm):
    """d below the compiled width D = 2, 4, 8, 16 of every instantiation, with a bias; with and without the two normalisations"""
    from deep_cartograph_amd import hip

    n, F = 77, 64
    X, W, fm, fr, bias, cm, cr = project_inputs(n, F, d)
    if not norm:
        fm = fr = cm = cr = None
    ref, bound = project_ref(X, W, fm, fr, bias, cm, cr)
    out, mm = hip.project_linear(dev(X), dev(W), want_minmax=True, **gpu_vectors(fmean=fm, frange=fr, bias=bias, cvmean=cm, cvrange=cr))
    project_check(out.cpu().numpy(), mm.cpu().numpy(), ref, bound, f"{n} x {F} d={d} norm={norm}")


@pytest.mark.parametrize("F,kind,vec", [(64, "wide", True), (64, "offset", False), (64, "oddld", False), (54, "wide4", False),
                                        (64, "contiguous", True)])
def test_project_linear_views(F, kind, vec):
    from deep_cartograph_amd import hip

    n, d = 333, 4
    X, W, fm, fr, bias, cm, cr = project_inputs(n, F, d)
    ref, bound = project_ref(X, W, fm, fr, bias, cm, cr)
    v = View(X, kind)
    assert quad_loads(v.t) == vec
    out, mm = hip.project_linear(v.t, dev(W), want_minmax=True, **gpu_vectors(fmean=fm, frange=fr, bias=bias, cvmean=cm, cvrange=cr))
    project_check(out.cpu().numpy(), mm.cpu().numpy(), ref, bound, f"{n} x {F} d={d} {kind}")
    assert v.guard_intact()
    np.testing.assert_array_equal(v.host(), X)


@pytest.mark.parametrize("kind", ["contiguous", "offset"])
@pytest.mark.parametrize("n", [1, 15, 65, 129])
def test_project_linear_rows_past_the_end(n, kind):
    """a block iteration takes 64 rows, four in flight per 16-lane group: n = 1 and 15 leave rows past the end in every
    in-flight slot, 65 and 129 one row into the next iteration"""
    from deep_cartograph_amd import hip

    F, d = 16, 2
    X, W, fm, fr, bias, cm, cr = project_inputs(n, F, d)
    ref, bound = project_ref(X, W, fm, fr, bias, cm, cr)
    v = View(X, kind)
    out, mm = hip.project_linear(v.t, dev(W), want_minmax=True, **gpu_vectors(fmean=fm, frange=fr, bias=bias, cvmean=cm, cvrange=cr))
    assert out.shape == (n, d)
    project_check(out.cpu().numpy(), mm.cpu().numpy(), ref, bound, f"{n} x {F} d={d} {kind}")
    assert v.guard_intact()


def test_project_linear_grid_stride_loop():
    from deep_cartograph_amd import hip

    n, F, d = 131137, 8, 1
    n_iter = -(-n // 64)
    blocks = min(8 * ncu(), 4096)   # project.hip: proj_blocks
    assert n_iter == 2050 and n_iter > blocks, f"{blocks} blocks take {n_iter} iterations in one pass: the loop is not reached"
    X, W, fm, fr, bias, cm, cr = project_inputs(n, F, d)
    ref, bound = project_ref(X, W, fm, fr, bias, cm, cr)
    out, mm = hip.project_linear(dev(X), dev(W), want_minmax=True, **gpu_vectors(fmean=fm, frange=fr, bias=bias, cvmean=cm, cvrange=cr))
    project_check(out.cpu().numpy(), mm.cpu().numpy(), ref, bound, f"{n} x {F} d={d}")


@pytest.mark.parametrize("F,vec,lds", [(1026, False, 74016), (1024, True, 73728)])
def test_project_linear_above_64k_of_lds(F, vec, lds):
    """weights, means and ranges of d = 16 components in LDS: (16 + 2) x roundup(F, 4) floats, above the 64 KiB a kernel gets
    without asking, in the scalar and the 16-byte instantiation"""
    from deep_cartograph_amd import hip

    n, d = 50, 16
    assert (16 + 2) * ((F + 3) // 4 * 4) * 4 == lds and lds > 64 * 1024
    X, W, fm, fr, bias, cm, cr = project_inputs(n, F, d)
    ref, bound = project_ref(X, W, fm, fr, bias, cm, cr)
    Xd = dev(X)
    assert quad_loads(Xd) == vec
    out, mm = hip.project_linear(Xd, dev(W), want_minmax=True, **gpu_vectors(fmean=fm, frange=fr, bias=bias, cvmean=cm, cvrange=cr))
    project_check(out.cpu().numpy(), mm.cpu().numpy(), ref, bound, f"{n} x {F} d={d}")


def test_project_linear_refuses_what_lds_cannot_hold():
    from deep_cartograph_amd import hip

    n, F, d = 10, 2400, 16
    assert (16 + 2) * F * 4 == 172800 > 160 * 1024
    X, W, fm, fr, bias, cm, cr = project_inputs(n, F, d)
    with pytest.raises(hip.DcvError, match="LDS"):
        hip.project_linear(dev(X), dev(W), want_minmax=True, **gpu_vectors(fmean=fm, frange=fr))
    torch.cuda.synchronize()   # nothing was launched, nothing is pending
    out, _ = hip.project_linear(dev(X[:, :64].copy()), dev(W[:64].copy()))
    ref, bound = project_ref(X[:, :64], W[:64])
    project_check(out.cpu().numpy(), None, ref, bound, "after the refusal")


def test_project_linear_out_or_extrema_alone():
    from deep_cartograph_amd import hip

    n, F, d = 333, 64, 4
    X, W, fm, fr, bias, cm, cr = project_inputs(n, F, d)
    ref, bound = project_ref(X, W, fm, fr, bias, cm, cr)
    kw = gpu_vectors(fmean=fm, frange=fr, bias=bias, cvmean=cm, cvrange=cr)
    Xd, Wd = dev(X), dev(W)
    out, mm = hip.project_linear(Xd, Wd, want_minmax=True, **kw)
    none, mm_alone = hip.project_linear(Xd, Wd, want_out=False, want_minmax=True, **kw)
    out_alone, none2 = hip.project_linear(Xd, Wd, want_out=True, want_minmax=False, **kw)
    assert none is None and none2 is None
    project_check(out.cpu().numpy(), mm.cpu().numpy(), ref, bound, "out and extrema")
    assert torch.equal(out_alone, out)
    np.testing.assert_array_equal(mm_alone.cpu().numpy(), np.stack([out.cpu().numpy().min(0), out.cpu().numpy().max(0)]))


# ------------------------------------------------------------------------------------------------ run-time switches
SWITCH_NORM = (513, 64)
SWITCH_COV = (2053, 130, 3)


def switched_run():
    """What a child process with a switch set computes: the rows-kernel normalise case 513 x 64 in every arrangement and the
    covariance case 2053 x 130 with a shift, through 16-byte loads (wide4) and scalar ones."""
    out = {"env": np.array([os.environ.get(k, "") for k in ("DCV_NORMALIZE_NT", "DCV_NORMALIZE_FLAT", "DCV_COV_FUSED_SUMS")])}
    n, F = SWITCH_NORM
    X, m, r, _ = norm_inputs(n, F)
    for arr in ARRANGEMENTS:
        out["norm_" + arr], out["norm_guards_" + arr] = run_normalize(X, m, r, arr)
    P, F, lag = SWITCH_COV
    X, sh = cov_inputs(P, F, lag, True)
    for kind in ("wide4", "contiguous"):
        raw, log, _ = run_cov(X, sh, P, lag, kind)
        out["cov_" + kind], out["cov_vec_" + kind] = raw, np.array([len(log), int(log[0].vec), log[0].splits])
    return out


SWITCH_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_streaming_gpu import switched_run
np.savez(sys.argv[2], **switched_run())
"""


@pytest.mark.parametrize("switch", ["DCV_NORMALIZE_NT=0", "DCV_NORMALIZE_FLAT=1", "DCV_COV_FUSED_SUMS=0"])
def test_switch_in_a_fresh_process(switch, tmp_path):
    """The switches are read once per process.  DCV_NORMALIZE_NT=0: the rows kernel with plain loads and stores;
    DCV_NORMALIZE_FLAT=1: the flat 16-byte kernel where the rows kernel would run; DCV_COV_FUSED_SUMS=0: the column sums of
    a shifted covariance from the float64 statistics pass and cov_sums_kernel's shift term.  Each child is held to the
    oracle, not to another setting."""
    name, val = switch.split("=")
    script = tmp_path / "switched.py"
    script.write_text(SWITCH_SCRIPT)
    env = dict(os.environ)
    for k in ("DCV_NORMALIZE_NT", "DCV_NORMALIZE_FLAT", "DCV_COV_FUSED_SUMS", "DCV_NORMALIZE_RPB", "DCV_COV_CHUNK"):
        env.pop(k, None)
    env[name] = val
    res_path = tmp_path / "switched.npz"
    res = subprocess.run([sys.executable, str(script), ROOT, str(res_path)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    got = np.load(res_path)
    assert dict(zip(("DCV_NORMALIZE_NT", "DCV_NORMALIZE_FLAT", "DCV_COV_FUSED_SUMS"), got["env"]))[name] == val
    n, F = SWITCH_NORM
    _, _, _, ref = norm_inputs(n, F)
    for arr in ARRANGEMENTS:
        np.testing.assert_array_equal(got["norm_" + arr], ref, err_msg=arr)
        assert bool(got["norm_guards_" + arr]), arr
    P, F, lag = SWITCH_COV
    X, sh = cov_inputs(P, F, lag, True)
    for kind, vec in (("wide4", 1), ("contiguous", 0)):
        assert list(got["cov_vec_" + kind]) == [1, vec, 2], kind
        cov_check(got["cov_" + kind], X, sh, P, lag, f"{switch} {kind}")


# ------------------------------------------------------------------------------------------------ argument validation
def bad_vector(length, how):
    if how == "float64":
        return torch.ones(length, dtype=torch.float64, device="cuda")
    if how == "short":
        return torch.ones(length - 1, dtype=torch.float32, device="cuda")
    v = torch.ones(2 * length, dtype=torch.float32, device="cuda")[::2]
    assert v.shape == (length,) and not v.is_contiguous()
    return v


VECTORS = ["mean", "rng", "fmean", "frange", "bias", "cvmean", "cvrange", "shift"]


@pytest.mark.parametrize("how", ["float64", "short", "strided"])
@pytest.mark.parametrize("name", VECTORS)
def test_wrappers_refuse_a_wrong_vector(name, how):
    """The kernels read F (or d) consecutive float32 values from each vector's base address: a float64 vector (NumPy's
    default) would be read as float32 pairs, a short one past its end.  The wrappers raise before anything is launched."""
    from deep_cartograph_amd import hip

    n, F, d = 20, 8, 4
    X = torch.zeros(n, F, device="cuda")
    W = torch.zeros(F, d, device="cuda")
    good = {"mean": torch.zeros(F, device="cuda"), "rng": torch.ones(F, device="cuda"), "fmean": torch.zeros(F, device="cuda"),
            "frange": torch.ones(F, device="cuda"), "bias": torch.zeros(d, device="cuda"), "cvmean": torch.zeros(d, device="cuda"),
            "cvrange": torch.ones(d, device="cuda"), "shift": torch.zeros(F, device="cuda")}
    bad = dict(good)
    bad[name] = bad_vector(good[name].shape[0], how)

    def call(v):
        if name in ("mean", "rng"):
            return hip.normalize(X, v["mean"], v["rng"])
        if name == "shift":
            return hip.lagged_cov_raw(X, n - 2, 2, v["shift"])
        return hip.project_linear(X, W, **{k: v[k] for k in ("fmean", "frange", "bias", "cvmean", "cvrange")})

    call(good)
    with pytest.raises(hip.DcvError, match=name if name != "rng" else "range"):
        call(bad)


@pytest.mark.parametrize("shape", [(19, 8), (20, 12), (20, 4), (21, 8)])
def test_normalize_refuses_an_out_of_another_shape(shape):
    from deep_cartograph_amd import hip

    X = torch.zeros(20, 8, device="cuda")
    with pytest.raises(hip.DcvError, match="out"):
        hip.normalize(X, torch.zeros(8, device="cuda"), torch.ones(8, device="cuda"), out=torch.empty(*shape, device="cuda"))
