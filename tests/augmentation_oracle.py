"""Oracle of the frame interpolation (csrc/interp.hip, hip.interpolate; test infrastructure, not a test module).

`scipy_interpolate` calls the classes the reference calls -- scipy.interpolate.PchipInterpolator(x, y, axis=0) and
Akima1DInterpolator(x, y, axis=0, method="makima") -- on the float32 data with knot k at time k.  `restated` is the
NumPy float64 restatement of the formulas in include/dcv.h (the contract of the kernel), kept beside scipy so that a
CPU test can hold one against the other.  `tolerance` is the derived bound of the GPU tests, `makima_margin` the
condition on their inputs."""
import numpy as np

KIND_OF_METHOD = {"pchip": "pchip", "akima": "makima"}


def scipy_interpolate(y, t, kind, extrapolate=True):
    """float64 (len(t), ...) values of scipy's interpolant through y (n_knots, ...) at the times t."""
    from scipy.interpolate import Akima1DInterpolator, PchipInterpolator

    y = np.asarray(y)
    x = np.arange(y.shape[0], dtype=np.float64)
    if kind == "pchip":
        f = PchipInterpolator(x, y, axis=0, extrapolate=bool(extrapolate))
    elif kind == "makima":
        f = Akima1DInterpolator(x, y, axis=0, method="makima", extrapolate=bool(extrapolate))
    else:
        raise ValueError(kind)
    return np.asarray(f(np.asarray(t, dtype=np.float64)), dtype=np.float64)


def _sign_differs(a, b):
    return np.sign(a) != np.sign(b)   # NaN != NaN: true, as in scipy


def _pchip_end(m0, m1):
    e = (3.0 * m0 - m1) / 2.0
    zero = _sign_differs(e, m0)
    clip = ~zero & _sign_differs(m0, m1) & (np.abs(e) > 3.0 * np.abs(m0))
    return np.where(zero, 0.0, np.where(clip, 3.0 * m0, e))


def pchip_derivatives(y):
    y = np.asarray(y, dtype=np.float64)
    m = y[1:] - y[:-1]
    d = np.zeros_like(y)
    if y.shape[0] == 2:
        d[0] = d[1] = m[0]
        return d
    with np.errstate(divide="ignore", invalid="ignore"):
        inner = 1.0 / ((3.0 / m[:-1] + 3.0 / m[1:]) / 6.0)
    d[1:-1] = np.where(_sign_differs(m[:-1], m[1:]) | (m[:-1] == 0) | (m[1:] == 0), 0.0, inner)
    d[0] = _pchip_end(m[0], m[1])
    d[-1] = _pchip_end(m[-1], m[-2])
    return d


def makima_weights(y):
    """(M, f1, f2): the padded slopes (n + 3 rows) and the two weights of every knot (n rows each)."""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    if n < 3:
        raise ValueError("makima needs at least 3 knots")
    M = np.empty((n + 3,) + y.shape[1:])
    M[2:-2] = y[1:] - y[:-1]
    M[1] = 2.0 * M[2] - M[3]
    M[0] = 2.0 * M[1] - M[2]
    M[-2] = 2.0 * M[-3] - M[-4]
    M[-1] = 2.0 * M[-2] - M[-3]
    f1 = np.abs(M[3:] - M[2:-1]) + 0.5 * np.abs(M[3:] + M[2:-1])
    f2 = np.abs(M[1:-2] - M[:-3]) + 0.5 * np.abs(M[1:-2] + M[:-3])
    return M, f1, f2


def makima_threshold(y):
    """1e-9 G with G the largest finite f1 + f2 of the whole array."""
    _, f1, f2 = makima_weights(y)
    f12 = f1 + f2
    finite = f12[np.isfinite(f12)]
    return 1e-9 * (finite.max() if finite.size else -np.inf)


def makima_derivatives(y):
    M, f1, f2 = makima_weights(y)
    f12 = f1 + f2
    with np.errstate(divide="ignore", invalid="ignore"):
        weighted = (f1 * M[1:-2] + f2 * M[2:-1]) / f12
    return np.where(f12 > makima_threshold(y), weighted, 0.5 * (M[3:] + M[:-3]))


def makima_margin(y):
    """The condition on makima inputs: no f1 + f2 within a factor of 2 of the threshold 1e-9 G, so that a flip of the
    branch cannot pass for rounding.  Returns (threshold, smallest value above it, largest value below it)."""
    _, f1, f2 = makima_weights(y)
    f12 = (f1 + f2)[np.isfinite(f1 + f2)]
    thr = makima_threshold(y)
    near = (f12 > 0.5 * thr) & (f12 < 2.0 * thr)
    assert not near.any(), f"{int(near.sum())} values of f1 + f2 lie within a factor of 2 of the threshold {thr:.3e}"
    above, below = f12[f12 > thr], f12[f12 <= thr]
    return thr, (above.min() if above.size else np.inf), (below.max() if below.size else 0.0)


def restated(y, t, kind, extrapolate=True):
    """The header's formulas in NumPy float64: y (n_knots, ...) float32, t (n_out,) -> (n_out, ...) float64."""
    y = np.asarray(y, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    n = y.shape[0]
    d = pchip_derivatives(y) if kind == "pchip" else makima_derivatives(y)
    K = np.clip(np.floor(t), 0, n - 2).astype(np.int64)
    s = (t - K).reshape((-1,) + (1,) * (y.ndim - 1))
    m = y[K + 1] - y[K]
    T = d[K] + d[K + 1] - 2.0 * m
    p = y[K] + d[K] * s + ((m - d[K]) - T) * (s * s) + T * (s * s * s)
    if not extrapolate:
        p[(t < 0) | (t > n - 1)] = np.nan
    return p


def tolerance(ref, y_sel):
    """|out - ref| <= spacing(float32(|ref|)) + 2^-43 Ymax per element: one rounding to float32, plus the float64
    evaluation of the same cubic on both sides (a few dozen roundings on magnitudes of at most about 8 Ymax).  `ref`
    is (n_out, n_sel, 3), `y_sel` the knots of the same columns (n_knots, n_sel, 3)."""
    ymax = np.abs(np.asarray(y_sel, dtype=np.float64)).max(axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 2.0 ** -43 * ymax[None]


def assert_close(out, ref, y_sel, what=""):
    """Every finite element within `tolerance`, NaN exactly where the reference has NaN.  Returns the largest error in
    units of the bound."""
    out = np.asarray(out, dtype=np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(out), nan), f"{what}: NaN positions differ ({int(np.isnan(out).sum())} against {int(nan.sum())})"
    tol = tolerance(np.where(nan, 0.0, ref), y_sel)
    ratio = np.where(nan, 0.0, np.abs(out - np.where(nan, 0.0, ref)) / tol)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: max |out - ref| / bound = {worst:.3f} over {int((~nan).sum())} finite elements")
    assert worst <= 1.0, f"{what}: |out - ref| reaches {worst:.3f} of the bound"
    return worst


def crafted(n_knots, n_atoms, seed, special_atoms=()):
    """(n_knots, n_atoms, 3) float32 coordinates of about 130 A: a random walk per column, with the shapes that reach
    every branch written into the atoms `special_atoms` (first: a constant column, flat runs, a monotone column;
    second: signs alternating at both ends, a mirrored alternation, a decreasing column)."""
    rng = np.random.default_rng(seed)
    y = 100.0 + 30.0 * rng.random((1, n_atoms, 3)) + np.cumsum(rng.normal(0.0, 1.5, (n_knots, n_atoms, 3)), axis=0)
    k = np.arange(n_knots, dtype=np.float64)
    if len(special_atoms) > 0:
        a = special_atoms[0]
        y[:, a, 0] = 117.25
        y[:, a, 1] = 90.0 + np.floor(k / 3.0) * 1.5 * (1 + (k // 6) % 2)          # runs of three equal knots
        y[:, a, 2] = 50.0 + np.cumsum(np.abs(rng.normal(0.0, 2.0, n_knots)))
    if len(special_atoms) > 1:
        b = special_atoms[1]
        y[:, b, 0] = 10.0 + (-1.0) ** k * (1.0 + 0.5 * k)                          # end slopes of opposite signs, growing: both end masks
        y[:, b, 1] = 20.0 - (-1.0) ** k * (4.0 / (1.0 + k))
        y[:, b, 2] = 80.0 - np.cumsum(np.abs(rng.normal(0.0, 2.0, n_knots)))
    return y.astype(np.float32)
