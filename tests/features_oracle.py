"""Float64 NumPy oracle of dcv_featurize: distances and torsions of (n, A, 3) float32 coordinates, with the
arithmetic include/dcv.h documents -- p = float64(x) * unit, no fused multiply-adds, nothing rounded to float32.
Independent of the package: it reads nothing but the coordinate array and the records."""
import numpy as np

DISTANCE, TORSION_SINCOS, TORSION = 0, 1, 2
COLUMNS = {DISTANCE: 1, TORSION_SINCOS: 2, TORSION: 1}


def n_columns(defs):
    return max(int(r[5]) + COLUMNS[int(r[0])] for r in defs)


def torsion_xy(p0, p1, p2, p3):
    """(x, y) with angle = atan2(y, x); inputs (n, 3) float64."""
    b0, b1, b2 = p1 - p0, p2 - p1, p3 - p2

    def cross(u, v):
        return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                         u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)

    def dot(u, v):
        return u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2]

    n1, n2 = cross(b0, b1), cross(b1, b2)
    x = dot(n1, n2)
    l1 = np.sqrt(dot(b1, b1))
    q = dot(cross(n1, n2), b1)
    with np.errstate(invalid="ignore", divide="ignore"):
        y = np.where(l1 == 0.0, 0.0, q / np.where(l1 == 0.0, 1.0, l1))
    return x, y


def featurize(xyz, defs, unit=0.1, n_cols=None, fill=np.nan):
    """(n, F) float64.  Columns no record writes hold `fill`."""
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32 and xyz.ndim == 3 and xyz.shape[2] == 3
    P = xyz.astype(np.float64) * np.float64(unit)
    defs = np.asarray(defs).reshape(-1, 6)
    F = n_columns(defs) if n_cols is None else n_cols
    out = np.full((xyz.shape[0], F), fill, dtype=np.float64)
    for kind, a0, a1, a2, a3, col in defs:
        if kind == DISTANCE:
            b = P[:, a1] - P[:, a0]
            out[:, col] = np.sqrt(b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1] + b[:, 2] * b[:, 2])
            continue
        x, y = torsion_xy(P[:, a0], P[:, a1], P[:, a2], P[:, a3])
        if kind == TORSION:
            out[:, col] = np.arctan2(y, x)
        else:
            r = np.hypot(x, y)
            with np.errstate(invalid="ignore", divide="ignore"):
                safe = np.where(r == 0.0, 1.0, r)
                out[:, col] = np.where(r == 0.0, 0.0, y / safe)
                out[:, col + 1] = np.where(r == 0.0, 1.0, x / safe)
    return out


def ulp_distance_f32(a, b):
    """Distance in float32 units in the last place between two float32 arrays (finite values)."""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, np.int64(-2 ** 31) - a, a)   # map the sign-magnitude order onto the integers
    b = np.where(b < 0, np.int64(-2 ** 31) - b, b)
    return np.abs(a - b)
