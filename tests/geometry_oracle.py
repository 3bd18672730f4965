"""Float64 NumPy oracle of the geometry analysis: optimal superposition by Kabsch's SVD with the determinant correction
(not the quaternion form the kernel uses), and the RMSD / average structure / RMSF / dRMSD built on it as
deep_cartograph_amd.geometry documents them.  Row-vector convention: aligned = (x - c_mob) . R + c_ref."""
import numpy as np

from tests import features_oracle as fo


def kabsch(x, y, w=None):
    """(R, c_mob, c_ref) of one frame: the proper rotation minimising sum w |(x - c_mob) . R - (y - c_ref)|^2."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    w = np.ones(len(x)) if w is None else np.asarray(w, dtype=np.float64)
    c_mob, c_ref = (w[:, None] * x).sum(0) / w.sum(), (w[:, None] * y).sum(0) / w.sum()
    H = ((x - c_mob) * w[:, None]).T @ (y - c_ref)
    U, _, Vt = np.linalg.svd(H)
    d = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0
    return U @ np.diag([1.0, 1.0, d]) @ Vt, c_mob, c_ref


def superpose(xyz, fit, fit_ref, sel=None, sel_ref=None, w=None):
    """The outputs of hip.superpose for (n, A, 3) coordinates: transform [n, 16], rmsd [n, 2], aligned [n, n_sel, 3]
    (float64, not rounded) and moments [n_sel, 3, 2]."""
    xyz = np.asarray(xyz, dtype=np.float64)
    n = len(xyz)
    fit = np.asarray(fit)
    fit_ref = np.asarray(fit_ref, dtype=np.float64)
    wv = np.ones(len(fit)) if w is None else np.asarray(w, dtype=np.float64)
    n_sel = 0 if sel is None else len(sel)
    out = {"transform": np.zeros((n, 16)), "rmsd": np.zeros((n, 2)), "aligned": np.zeros((n, n_sel, 3)), "moments": np.zeros((n_sel, 3, 2))}
    for f in range(n):
        R, c_mob, c_ref = kabsch(xyz[f, fit], fit_ref, wv)
        res = (xyz[f, fit] - c_mob) @ R - (fit_ref - c_ref)
        fit_rmsd = np.sqrt((wv * (res ** 2).sum(1)).sum() / wv.sum())
        out["transform"][f] = np.concatenate([R.ravel(), c_mob, c_ref, [fit_rmsd]])
        out["rmsd"][f, 0] = fit_rmsd
        if n_sel:
            al = (xyz[f, sel] - c_mob) @ R + c_ref
            out["aligned"][f] = al
            if sel_ref is not None:
                d = al - np.asarray(sel_ref, dtype=np.float64)
                out["rmsd"][f, 1] = np.sqrt((d ** 2).sum() / n_sel)
                out["moments"][:, :, 0] += d
                out["moments"][:, :, 1] += d ** 2
    return out


def rmsd(xyz, fit, fit_ref, sel, sel_ref):
    return superpose(xyz, fit, fit_ref, sel, sel_ref)["rmsd"][:, 1]


def average_structure(xyz, fit):
    """Mean of the fit atoms after fitting every frame to frame 0 on them."""
    first = np.asarray(xyz[0, fit], dtype=np.float64)
    return superpose(xyz, fit, first, fit)["aligned"].mean(0)


def rmsf(xyz, fit, sel, resids):
    """(per-residue mean RMSF, residues ascending): frames fitted on `fit` to the average structure, ddof = 0."""
    aligned = superpose(xyz, fit, average_structure(xyz, fit), sel)["aligned"]
    per_atom = np.sqrt(aligned.var(axis=0).sum(axis=1))
    resids = np.asarray(resids)[np.asarray(sel)]
    residues = np.unique(resids)
    return np.asarray([per_atom[resids == r].mean() for r in residues]), residues


def drmsd(xyz, ref_positions, defs, unit=0.1):
    """sqrt(mean((d - d_ref)^2)) per frame over the distance records `defs`, in float64 from float64 distances."""
    d = fo.featurize(np.asarray(xyz, dtype=np.float32), defs, unit=unit)
    d_ref = fo.featurize(np.asarray(ref_positions, dtype=np.float32)[None], defs, unit=unit)[0]
    return np.sqrt(np.mean((d - d_ref) ** 2, axis=1))


def random_rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def synthetic(n, A, seed, sigma=20.0, noise=1.0, shift=300.0):
    """(xyz float32 [n, A, 3], reference float64 [A, 3]): a random reference of sigma Angstrom, per frame a random
    rotation, a translation of a few hundred Angstrom and `noise` Angstrom of noise, cast to float32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ref = rng.standard_normal((A, 3)) * sigma
    xyz = np.empty((n, A, 3), dtype=np.float32)
    for f in range(n):
        xyz[f] = ((ref + rng.standard_normal((A, 3)) * noise) @ random_rotation(rng) + rng.uniform(-shift, shift, 3)).astype(np.float32)
    return xyz, ref
