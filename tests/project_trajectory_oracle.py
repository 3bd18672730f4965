"""Float64 NumPy oracle of dcv_featurize_project and the derived error bound of its tests.

The chain include/dcv.h documents: features_oracle.featurize (float64) -> float32 -> IEEE float32 normalisation ->
float64 product with W and the float64 tail (y + bias - cvmean) / cvrange.  Reads nothing but its arguments."""
import numpy as np

from tests import features_oracle as fo


def features(xyz, records, F, unit=0.1):
    """(n, F) float64: feature i of every frame from the (n_rec, 8) records [kind, a0..a3, feature0, feature1, 0]."""
    records = np.asarray(records).reshape(-1, 8)
    defs = np.concatenate([records[:, :5], 2 * np.arange(len(records))[:, None]], axis=1)
    pairs = fo.featurize(xyz, defs, unit=unit, n_cols=2 * len(records))
    out = np.full((xyz.shape[0], F), np.nan)
    for r, (f0, f1) in enumerate(records[:, 5:7]):
        if f0 >= 0:
            out[:, f0] = pairs[:, 2 * r]
        if f1 >= 0:
            out[:, f1] = pairs[:, 2 * r + 1]
    return out


def project(f32, W, fmean=None, frange=None, bias=None, cvmean=None, cvrange=None):
    """(ref, bound) in float64 from the float32 features.

    |out - ref| <= 2^-24 |ref| + (F 2^-53 S + 2^-22 T) / |cvrange|,  S = |xn| @ |W| + |bias| + |cvmean|,
    T = (|f| / |frange|) @ |W|: the one rounding of the result; a float64 sum of F exact products in any order; a
    feature one float32 ulp off the oracle's (the device's libm, as the featurize tests allow)."""
    assert f32.dtype == np.float32 and W.dtype == np.float32
    d = W.shape[1]
    xn = ((f32 - fmean) / frange).astype(np.float32) if fmean is not None else f32
    fr = np.abs(frange.astype(np.float64)) if frange is not None else np.ones(f32.shape[1])
    b = bias.astype(np.float64) if bias is not None else np.zeros(d)
    m = cvmean.astype(np.float64) if cvmean is not None else np.zeros(d)
    r = cvrange.astype(np.float64) if cvrange is not None else np.ones(d)
    xn64, W64 = xn.astype(np.float64), W.astype(np.float64)
    ref = (xn64 @ W64 + b - m) / r
    S = np.abs(xn64) @ np.abs(W64) + np.abs(b) + np.abs(m)
    T = (np.abs(f32.astype(np.float64)) / fr) @ np.abs(W64)
    bound = 2.0 ** -24 * np.abs(ref) + (f32.shape[1] * 2.0 ** -53 * S + 2.0 ** -22 * T) / np.abs(r)
    return ref, bound


def featurize_project(xyz, records, W, unit=0.1, **vectors):
    """(ref, bound, float32 features) of coordinates (n, A, 3) float32."""
    f32 = features(xyz, records, W.shape[0], unit).astype(np.float32)
    ref, bound = project(f32, W, **vectors)
    return ref, bound, f32


def two_step_bound(f32, W, fmean=None, frange=None, bias=None, cvmean=None, cvrange=None):
    """The bound of dcv_project_linear's float32 chain on the same features (tests/test_streaming_gpu.py's project_ref,
    restated): 4e-7 S' for the fp32 fma chain, S' = |xn| @ |W| + |bias|, one rounding (1.2e-7) of the subtraction of
    cvmean and one of the division."""
    d = W.shape[1]
    xn = (((f32 - fmean) / frange).astype(np.float32) if fmean is not None else f32).astype(np.float64)
    b = bias.astype(np.float64) if bias is not None else np.zeros(d)
    m = cvmean.astype(np.float64) if cvmean is not None else np.zeros(d)
    r = cvrange.astype(np.float64) if cvrange is not None else np.ones(d)
    y = xn @ W.astype(np.float64) + b
    S = np.abs(xn) @ np.abs(W.astype(np.float64)) + np.abs(b)
    ref = (y - m) / r
    return (4e-7 * S + 1.2e-7 * (np.abs(y) + np.abs(m))) / np.abs(r) + 1.2e-7 * np.abs(ref)
