"""Thin torch-tensor front end of the C-ABI (include/dcv.h).

torch is plumbing here: it owns device memory and the current stream; every number is
produced by a HIP kernel of libdcv.so.  All functions require CUDA(HIP) tensors and raise
otherwise -- there is no CPU path.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import FEAT_DISTANCE, FEAT_TORSION, FEAT_TORSION_SINCOS, INTERP_MAKIMA, INTERP_PCHIP, DcvError, check


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise DcvError("deep_cartograph_amd kernels need tensors on an MI355X (cuda) device; got a CPU tensor")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _check_matrix(X: torch.Tensor, dtype=torch.float32):
    if X.dim() != 2 or X.dtype != dtype or X.stride(1) != 1:
        raise DcvError(f"expected a row-major 2-D {dtype} tensor, got shape {tuple(X.shape)} dtype {X.dtype} strides {X.stride()}")


def _check_vector(v: Optional[torch.Tensor], length: int, name: str, device=None):
    """The kernels read ``length`` consecutive float32 values from the vector's base address: anything else (a float64
    NumPy default, a shorter or strided vector, another device) would be read as garbage or past its end.  None passes."""
    if v is None:
        return
    if v.dim() != 1 or v.dtype != torch.float32 or v.shape[0] != length or not v.is_contiguous():
        raise DcvError(f"{name}: expected a contiguous float32 vector of {length} elements, got shape {tuple(v.shape)} "
                       f"dtype {v.dtype} strides {v.stride()}")
    if device is not None and v.device != device:
        raise DcvError(f"{name}: on {v.device}, the matrix is on {device}")


# ------------------------------------------------------------------------------- statistics
def col_stats_raw(X: torch.Tensor) -> torch.Tensor:
    """[4, F] float64: sum, sum of squares, min, max (dcv_col_stats)."""
    _require_gpu(X)
    _check_matrix(X)
    lib = _lib.load()
    n, F = X.shape
    out = torch.empty(4, F, dtype=torch.float64, device=X.device)
    ws = _ws(lib.dcv_col_stats_workspace(n, F), X.device)
    check(lib.dcv_col_stats(_ptr(X), n, F, X.stride(0), _ptr(out), _ptr(ws), ws.numel(), _stream()), "dcv_col_stats")
    return out


def finalize_stats(raw: torch.Tensor, n: int) -> dict:
    """mean / std(ddof=1) / min / max as float32 NumPy arrays from (all-reduced) raw sums."""
    r = raw.detach().cpu().numpy()
    mean = r[0] / n
    var = (r[1] - n * mean * mean) / max(n - 1, 1)
    std = np.sqrt(np.maximum(var, 0.0))
    return {"mean": mean.astype(np.float32), "std": std.astype(np.float32),
            "min": r[2].astype(np.float32), "max": r[3].astype(np.float32)}


def col_histogram(X: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
    """[F, bins] int64 counts of every column of X over its own bin edges ([F, bins + 1] float32), with
    np.histogram's semantics (dcv_col_histogram)."""
    _require_gpu(X, edges)
    _check_matrix(X)
    n, F = X.shape
    if edges.dim() != 2 or edges.shape[0] != F or edges.shape[1] < 2 or edges.dtype != torch.float32 or not edges.is_contiguous():
        raise DcvError(f"col_histogram: edges must be a contiguous float32 [F, bins + 1] tensor, got {tuple(edges.shape)} {edges.dtype}")
    lib = _lib.load()
    bins = edges.shape[1] - 1
    counts = torch.empty(F, bins, dtype=torch.int64, device=X.device)
    ws = _ws(lib.dcv_col_histogram_workspace(n, F, bins), X.device)
    check(lib.dcv_col_histogram(_ptr(X), n, F, X.stride(0), _ptr(edges), bins, _ptr(counts), _ptr(ws), ws.numel(), _stream()),
          "dcv_col_histogram")
    return counts


def dip_sorted_workspace_bytes(n: int, C: int) -> int:
    return int(_lib.load().dcv_dip_sorted_workspace(n, C))


def dip_sorted(Xs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dip [C] float64, lo [C] int32, hi [C] int32) of an n x C float32 matrix whose columns are each sorted
    ascending, e.g. torch.sort(X, dim=0).values (dcv_dip_sorted)."""
    _require_gpu(Xs)
    _check_matrix(Xs)
    n, C = Xs.shape
    if n == 0 or C == 0:
        raise DcvError("dip_sorted: empty matrix")
    # sorted columns: a NaN or an infinity can only sit in the first or the last row
    if not bool(torch.isfinite(Xs[0]).all() & torch.isfinite(Xs[-1]).all()):
        raise DcvError("dip_sorted: the matrix holds NaN or infinite values")
    lib = _lib.load()
    dip = torch.empty(C, dtype=torch.float64, device=Xs.device)
    lo = torch.empty(C, dtype=torch.int32, device=Xs.device)
    hi = torch.empty(C, dtype=torch.int32, device=Xs.device)
    ws = _ws(lib.dcv_dip_sorted_workspace(n, C), Xs.device)
    check(lib.dcv_dip_sorted(_ptr(Xs), n, C, Xs.stride(0), _ptr(dip), _ptr(lo), _ptr(hi), _ptr(ws), ws.numel(), _stream()),
          "dcv_dip_sorted")
    return dip, lo, hi


# ------------------------------------------------------------------------------- featurisation
_FEAT_COLUMNS = {FEAT_DISTANCE: 1, FEAT_TORSION_SINCOS: 2, FEAT_TORSION: 1}


def _coordinates(who: str, xyz: torch.Tensor, n_atoms: int, strides):
    """(n, base pointer, frame, atom and component stride) of the two coordinate forms the trajectory kernels accept."""
    if xyz.dtype != torch.float32:
        raise DcvError(f"{who}: coordinates must be float32, got {xyz.dtype}")
    if strides is None:
        if xyz.dim() != 3 or xyz.shape[1] != n_atoms or xyz.shape[2] != 3:
            raise DcvError(f"{who}: expected a (n, {n_atoms}, 3) tensor, got {tuple(xyz.shape)}")
        n = xyz.shape[0]
        fs, as_, cs = (int(s) for s in xyz.stride())
        return n, xyz.data_ptr(), fs, as_, cs
    n, offset, fs, as_, cs = (int(v) for v in strides)
    if xyz.dim() != 1 or not xyz.is_contiguous():
        raise DcvError(f"{who}: with explicit strides the coordinates must be a contiguous 1-D buffer")
    last = offset + max(n - 1, 0) * fs + (n_atoms - 1) * as_ + 2 * cs
    if n < 0 or offset < 0 or min(fs, as_, cs) < 0 or (n > 0 and last >= xyz.numel()):
        raise DcvError(f"{who}: layout {tuple(strides)} with {n_atoms} atoms reaches element {last} of a buffer of {xyz.numel()}")
    return n, xyz.data_ptr() + 4 * offset, fs, as_, cs


def featurize(xyz: torch.Tensor, defs, n_atoms: int, strides=None, unit: float = 0.1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[n, F] float32 distances / torsions of every frame (dcv_featurize).

    ``xyz``: float32 coordinates on the device.  With ``strides=None`` a (n, A, 3) tensor, read through its own
    strides.  Otherwise a 1-D buffer and ``strides = (n_frames, offset, frame_stride, atom_stride, comp_stride)`` in
    elements -- what ``trajectory.Trajectory.layout()`` returns: coordinate c of atom a of frame f is
    ``xyz[offset + f*frame_stride + a*atom_stride + c*comp_stride]``.
    ``defs``: (n_defs, 6) int32 records [kind, a0, a1, a2, a3, out_column] (FEAT_*), on the host.
    ``out``: optional row-major float32 [n, >= F] tensor; only the columns the records name are written."""
    _require_gpu(xyz, out)
    defs = np.ascontiguousarray(np.asarray(defs), dtype=np.int32)
    if defs.ndim != 2 or defs.shape[1] != 6 or defs.shape[0] == 0:
        raise DcvError(f"featurize: defs must be a non-empty (n_defs, 6) int32 array, got shape {defs.shape}")
    n_atoms = int(n_atoms)
    n, base, fs, as_, cs = _coordinates("featurize", xyz, n_atoms, strides)
    F = max(int(r[5]) + _FEAT_COLUMNS.get(int(r[0]), 1) for r in defs)
    if out is None:
        out = torch.empty(n, max(F, 1), dtype=torch.float32, device=xyz.device)
    else:
        _check_matrix(out)
        if out.shape[0] != n:
            raise DcvError(f"featurize: out has {out.shape[0]} rows for {n} frames")
        # the library checks columns against the row stride; a view may be narrower than that
        if F > out.shape[1] or int(defs[:, 5].min()) < 0:
            raise DcvError(f"featurize: the records write columns [{int(defs[:, 5].min())}, {F}), out has {out.shape[1]}")
    if n == 0:
        return out   # an empty tensor has no data pointer to hand to the library
    lib = _lib.load()
    ws = _ws(lib.dcv_featurize_workspace(n, n_atoms, defs.shape[0]), xyz.device)
    ldo = max(out.stride(0), out.shape[1])   # the stride of a one-row tensor is arbitrary
    check(lib.dcv_featurize(base, n, fs, as_, cs, n_atoms, defs.ctypes.data, defs.shape[0], float(unit), _ptr(out), ldo,
                            _ptr(ws), ws.numel(), _stream()), "dcv_featurize")
    return out


def featurize_project(xyz: torch.Tensor, records, n_atoms: int, F: int, W: torch.Tensor, strides=None, unit: float = 0.1, fmean=None,
                      frange=None, bias=None, cvmean=None, cvrange=None, want_minmax: bool = False, out: Optional[torch.Tensor] = None):
    """(out [n, d] float32, minmax [2, d] or None): ``featurize`` then ``project_linear`` in one launch, without the
    [n, F] matrix (dcv_featurize_project).

    ``xyz``, ``n_atoms``, ``strides`` and ``unit`` as in :func:`featurize`.  ``records``: (n_rec, 8) int32
    [kind, a0, a1, a2, a3, feature0, feature1, 0] on the host -- what ``trajectory.definitions_from_labels`` returns;
    every feature in [0, F) is the value of exactly one record.  ``W``: contiguous float32 [F, d], d <= 16; the five
    vectors as in :func:`project_linear`.  ``out``: optional float32 [n, d] tensor or view with unit column stride."""
    _require_gpu(xyz, W, fmean, frange, bias, cvmean, cvrange, out)
    records = np.ascontiguousarray(np.asarray(records), dtype=np.int32)
    if records.ndim != 2 or records.shape[1] != 8 or records.shape[0] == 0:
        raise DcvError(f"featurize_project: records must be a non-empty (n_rec, 8) int32 array, got shape {records.shape}")
    n_atoms, F = int(n_atoms), int(F)
    n, base, fs, as_, cs = _coordinates("featurize_project", xyz, n_atoms, strides)
    if W.dim() != 2 or W.shape[0] != F or not W.is_contiguous() or W.dtype != torch.float32 or W.device != xyz.device:
        raise DcvError(f"featurize_project: W must be a contiguous float32 {F} x d tensor on {xyz.device}")
    d = W.shape[1]
    for v, length, name in ((fmean, F, "fmean"), (frange, F, "frange"), (bias, d, "bias"), (cvmean, d, "cvmean"), (cvrange, d, "cvrange")):
        _check_vector(v, length, "featurize_project: " + name, xyz.device)
    if out is None:
        out = torch.empty(n, d, dtype=torch.float32, device=xyz.device)
    else:
        _check_matrix(out)
        if tuple(out.shape) != (n, d) or out.device != xyz.device:
            raise DcvError(f"featurize_project: out has shape {tuple(out.shape)} on {out.device}, expected ({n}, {d}) on {xyz.device}")
    mm = torch.empty(2, d, dtype=torch.float32, device=xyz.device) if want_minmax else None
    if n == 0:   # an empty tensor has no data pointer to hand to the library
        if mm is not None:
            mm[0], mm[1] = float("inf"), float("-inf")
        return out, mm
    lib = _lib.load()
    ws = _ws(lib.dcv_featurize_project_workspace(n, n_atoms, records.shape[0], F, d), xyz.device)
    ldo = max(out.stride(0), d)   # the stride of a one-row tensor is arbitrary
    check(lib.dcv_featurize_project(base, n, fs, as_, cs, n_atoms, records.ctypes.data, records.shape[0], F, float(unit), _ptr(fmean),
                                    _ptr(frange), _ptr(W), d, _ptr(bias), _ptr(cvmean), _ptr(cvrange), _ptr(out), ldo, _ptr(mm), _ptr(ws),
                                    ws.numel(), _stream()), "dcv_featurize_project")
    return out, mm


SUPERPOSE_OUTPUTS = ("transform", "rmsd", "aligned", "moments")


def superpose(xyz: torch.Tensor, n_atoms: int, fit, fit_ref, sel=None, sel_ref=None, fit_weights=None, strides=None,
              want=("rmsd",)) -> dict:
    """Optimal rigid superposition of every frame onto ``fit_ref`` on the atoms ``fit`` (dcv_superpose); Angstrom in,
    Angstrom out, float64 arithmetic.  Returns a dict with the outputs named in ``want``:

    ``transform`` [n, 16] float64: R row-major (row-vector convention), c_mob, c_ref, fit RMSD;
    ``rmsd``      [n, 2] float64: fit RMSD and the unweighted RMSD of ``sel`` to ``sel_ref``; without ``sel_ref`` there is
                  no second RMSD and the tensor is [n, 1] (the library's placeholder 0 is not handed out);
    ``aligned``   [n, n_sel, 3] float32: the aligned ``sel`` atoms;
    ``moments``   [n_sel, 3, 2] float64: per atom and component the sum over frames of d and d^2, d = aligned - sel_ref.

    ``xyz``, ``n_atoms`` and ``strides`` as in :func:`featurize`.  ``fit`` / ``sel``: atom indices; ``fit_ref`` (n_fit, 3)
    and ``sel_ref`` (n_sel, 3): float64 reference positions, on the host; ``fit_weights``: n_fit non-negative weights."""
    _require_gpu(xyz)
    want = tuple(want)
    unknown = [w for w in want if w not in SUPERPOSE_OUTPUTS]
    if unknown or not want:
        raise DcvError(f"superpose: want must name some of {SUPERPOSE_OUTPUTS}, got {want}")
    n_atoms = int(n_atoms)
    n, base, fs, as_, cs = _coordinates("superpose", xyz, n_atoms, strides)
    fit = np.ascontiguousarray(np.asarray(fit).reshape(-1), dtype=np.int32)
    fit_ref = np.ascontiguousarray(np.asarray(fit_ref, dtype=np.float64))
    if fit.size == 0 or fit_ref.shape != (fit.size, 3):
        raise DcvError(f"superpose: fit_ref must be ({fit.size}, 3) for {fit.size} fit atoms (at least one), got {fit_ref.shape}")
    if fit_weights is not None:
        fit_weights = np.ascontiguousarray(np.asarray(fit_weights, dtype=np.float64).reshape(-1))
        if fit_weights.size != fit.size:
            raise DcvError(f"superpose: {fit_weights.size} weights for {fit.size} fit atoms")
    n_sel = 0
    if sel is not None:
        sel = np.ascontiguousarray(np.asarray(sel).reshape(-1), dtype=np.int32)
        n_sel = int(sel.size)
    if sel_ref is not None:
        sel_ref = np.ascontiguousarray(np.asarray(sel_ref, dtype=np.float64))
        if n_sel == 0 or sel_ref.shape != (n_sel, 3):
            raise DcvError(f"superpose: sel_ref must be ({n_sel}, 3) for a selection of {n_sel} atoms, got {sel_ref.shape}")
    if ("aligned" in want or "moments" in want) and n_sel == 0:
        raise DcvError("superpose: aligned coordinates and moments need a selection (sel)")
    dev = xyz.device
    out = {}
    if "transform" in want:
        out["transform"] = torch.empty(n, 16, dtype=torch.float64, device=dev)
    if "rmsd" in want:
        out["rmsd"] = torch.empty(n, 2, dtype=torch.float64, device=dev)
    if "aligned" in want:
        out["aligned"] = torch.empty(n, n_sel, 3, dtype=torch.float32, device=dev)
    if "moments" in want:
        out["moments"] = torch.zeros(n_sel, 3, 2, dtype=torch.float64, device=dev)
    lib = _lib.load()
    ws = _ws(lib.dcv_superpose_workspace(n, n_atoms, fit.size, n_sel), dev)
    # with no frames the library only validates; an empty tensor has no data pointer to hand over
    check(lib.dcv_superpose(base if n else ws.data_ptr(), n, fs, as_, cs, n_atoms, fit.ctypes.data,
                            None if fit_weights is None else fit_weights.ctypes.data, fit_ref.ctypes.data, fit.size,
                            None if sel is None or n_sel == 0 else sel.ctypes.data, None if sel_ref is None else sel_ref.ctypes.data, n_sel,
                            _ptr(out.get("transform")) if n else None, _ptr(out.get("rmsd")) if n else None,
                            _ptr(out.get("aligned")) if n else None, 3 * n_sel, _ptr(out.get("moments")), _ptr(ws), ws.numel(), _stream()),
          "dcv_superpose")
    if "rmsd" in out and sel_ref is None:
        out["rmsd"] = out["rmsd"][:, :1]
    return out


def _output(who: str, out: Optional[torch.Tensor], out_strides, n: int, n_atoms: int, device, source: str = "coordinates"):
    """The ``out`` / ``out_strides`` pair of `who` (interpolate, transform_frames, xtc_decode) checked and resolved for
    `n` frames of `n_atoms` atoms: (the tensor to return, the address of its first coordinate, frame, atom and component
    stride in elements).  Without ``out`` that is a new dense float32 [n, n_atoms, 3] tensor on `device`."""
    if (out is None) != (out_strides is None):
        raise DcvError(f"{who}: out and out_strides go together")
    if out is None:
        out = torch.empty(n, n_atoms, 3, dtype=torch.float32, device=device)
        return out, out.data_ptr(), 3 * n_atoms, 3, 1
    off, ofs, oas, ocs = (int(v) for v in out_strides)
    if out.dim() != 1 or out.dtype != torch.float32 or not out.is_contiguous() or out.device != device:
        raise DcvError(f"{who}: out must be a contiguous 1-D float32 buffer on the device of the {source}")
    last = off + max(n - 1, 0) * ofs + (n_atoms - 1) * oas + 2 * ocs
    if off < 0 or min(ofs, oas, ocs) < 1 or (n > 0 and last >= out.numel()):
        raise DcvError(f"{who}: output layout {tuple(out_strides)} with {n_atoms} atoms and {n} frames reaches element "
                       f"{last} of a buffer of {out.numel()} (strides must be >= 1)")
    return out, out.data_ptr() + 4 * off, ofs, oas, ocs


INTERP_KINDS = {"pchip": INTERP_PCHIP, "makima": INTERP_MAKIMA}


def interpolate(xyz: torch.Tensor, n_atoms: int, t, kind: str = "pchip", sel=None, strides=None, extrapolate: bool = True,
                noise: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_strides=None) -> torch.Tensor:
    """The frames of a trajectory interpolated along time at the times ``t`` (dcv_interpolate): PCHIP or modified Akima
    (``kind`` "pchip" / "makima") through every coordinate column, frame k at time k, float64 arithmetic, equal to
    scipy's PchipInterpolator / Akima1DInterpolator(method="makima") to rounding.  Returns a float32 [n_out, n_sel, 3]
    tensor.

    ``xyz``, ``n_atoms`` and ``strides`` as in :func:`featurize`.  ``t``: n_out finite, non-decreasing float64 times, on
    the host.  ``sel``: the atoms to emit, in output order (None: all).  ``extrapolate``: times outside [0, n - 1] use the
    end pieces; False makes them NaN.  ``noise``: float64 [n_out, n_sel, 3] on the device, added before the one rounding
    to float32.  With ``out`` (a 1-D float32 buffer) and ``out_strides = (offset, frame, atom, comp)`` in elements,
    coordinate c of selected atom s of output frame j is written to ``out[offset + j*frame + s*atom + c*comp]`` -- the
    planes of DCD frame records, for instance -- nothing else is touched, and ``out`` is returned."""
    _require_gpu(xyz, noise, out)
    if kind not in INTERP_KINDS:
        raise DcvError(f"interpolate: kind must be one of {tuple(INTERP_KINDS)}, got {kind!r}")
    n_atoms = int(n_atoms)
    n, base, fs, as_, cs = _coordinates("interpolate", xyz, n_atoms, strides)
    t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1))
    n_out = int(t.size)
    if sel is not None:
        sel = np.ascontiguousarray(np.asarray(sel).reshape(-1), dtype=np.int32)
        if sel.size == 0:
            raise DcvError("interpolate: the selection is empty")
    n_sel = n_atoms if sel is None else int(sel.size)
    if noise is not None and (noise.dtype != torch.float64 or tuple(noise.shape) != (n_out, n_sel, 3) or not noise.is_contiguous()
                              or noise.device != xyz.device):
        raise DcvError(f"interpolate: noise must be a contiguous float64 ({n_out}, {n_sel}, 3) tensor on {xyz.device}, "
                       f"got {tuple(noise.shape)} {noise.dtype} on {noise.device}")
    result, out_ptr, ofs, oas, ocs = _output("interpolate", out, out_strides, n_out, n_sel, xyz.device)
    if n_out == 0:
        return result   # an empty tensor has no data pointer to hand to the library
    lib = _lib.load()
    ws = _ws(lib.dcv_interpolate_workspace(n, n_atoms, 0 if sel is None else n_sel, n_out), xyz.device)
    check(lib.dcv_interpolate(base if n else ws.data_ptr(), n, fs, as_, cs, n_atoms, None if sel is None else sel.ctypes.data,
                              0 if sel is None else n_sel, INTERP_KINDS[kind], int(bool(extrapolate)), t.ctypes.data, n_out,
                              _ptr(noise), out_ptr, ofs, oas, ocs, _ptr(ws), ws.numel(), _stream()),
          "dcv_interpolate")
    return result


def transform_frames(xyz: torch.Tensor, n_atoms: int, transform: torch.Tensor, strides=None, out: Optional[torch.Tensor] = None,
                     out_strides=None) -> torch.Tensor:
    """Every atom of every frame moved by the frame's rigid transform (dcv_transform_frames):
    ``out = (x - c_mob) . R + c_ref`` in float64, rounded once to float32; Angstrom in, Angstrom out.  Returns a float32
    [n, n_atoms, 3] tensor.  No limit on the number of atoms.

    ``xyz``, ``n_atoms`` and ``strides`` as in :func:`featurize`.  ``transform``: float64 [n, >= 15] on the device with
    row stride >= 15, R row-major, c_mob, c_ref -- the ``transform`` output of :func:`superpose` as it is.  ``out`` /
    ``out_strides = (offset, frame, atom, comp)`` as in :func:`interpolate`: a 1-D float32 buffer in which only the
    coordinate slots are written (the planes of DCD frame records, for instance); it must not overlap ``xyz``."""
    _require_gpu(xyz, transform, out)
    n_atoms = int(n_atoms)
    n, base, fs, as_, cs = _coordinates("transform_frames", xyz, n_atoms, strides)
    if (transform.dim() != 2 or transform.dtype != torch.float64 or transform.shape[0] != n or transform.shape[1] < 15
            or transform.stride(1) != 1 or transform.device != xyz.device):
        raise DcvError(f"transform_frames: transform must be a float64 ({n}, >= 15) tensor with unit column stride on {xyz.device}, "
                       f"got {tuple(transform.shape)} {transform.dtype} strides {transform.stride()} on {transform.device}")
    ldt = max(int(transform.stride(0)), int(transform.shape[1])) if n <= 1 else int(transform.stride(0))   # a one-row stride is arbitrary
    result, out_ptr, ofs, oas, ocs = _output("transform_frames", out, out_strides, n, n_atoms, xyz.device)
    if n == 0:
        return result   # an empty tensor has no data pointer to hand to the library
    check(_lib.load().dcv_transform_frames(base, n, fs, as_, cs, n_atoms, _ptr(transform), ldt, out_ptr, ofs, oas, ocs,
                                           _stream()), "dcv_transform_frames")
    return result


def xtc_decode(data: torch.Tensor, frames, n_atoms: int, scale: float = 10.0, out: Optional[torch.Tensor] = None, out_strides=None,
               return_status: bool = False):
    """The frames of a GROMACS ``.xtc`` file decoded on the device (dcv_xtc_decode).  Returns a float32
    [n, n_atoms, 3] tensor: the file's nanometres times ``scale`` (10: Angstrom), ``(float)i * (1.0f / precision) * scale``
    in float32.

    ``data``: the bytes of the file, or a slice of them that starts on a multiple of 4 bytes, as a contiguous 1-D uint8
    tensor on the device.  ``frames``: a host array of ``_lib.XTC_FRAME_DTYPE`` records, one per frame to decode, with
    offsets relative to ``data`` -- ``trajectory.XtcIndex.span`` makes both; choosing records is how a stride or a
    sub-range is applied.  ``out`` / ``out_strides = (offset, frame, atom, comp)`` as in :func:`interpolate`: a 1-D float32
    buffer in which only the coordinate slots are written (the planes of DCD frame records, for instance).
    A frame whose stream is inconsistent (it asks for bits behind its ``nbytes``, a run passes the atom count,
    ``smallidx`` leaves [9, 72]) raises DcvError naming the first such frame; with ``return_status`` nothing is raised
    and ``(out, status)`` is returned, ``status`` an int32 [n] device tensor (0: decoded), the coordinates of a marked
    frame unwritten from the inconsistency on.  No stream makes the kernel read or write out of range."""
    _require_gpu(data, out)
    frames = np.ascontiguousarray(frames)
    if frames.dtype != _lib.XTC_FRAME_DTYPE or frames.ndim != 1:
        raise DcvError(f"xtc_decode: frames must be a 1-D array of XTC_FRAME_DTYPE records, got {frames.dtype} {frames.shape}")
    if data.dim() != 1 or data.dtype != torch.uint8 or not data.is_contiguous():
        raise DcvError(f"xtc_decode: data must be a contiguous 1-D uint8 tensor, got {tuple(data.shape)} {data.dtype}")
    n, n_atoms = int(frames.size), int(n_atoms)
    if n_atoms < 1:
        raise DcvError(f"xtc_decode: {n_atoms} atoms")
    result, out_ptr, ofs, oas, ocs = _output("xtc_decode", out, out_strides, n, n_atoms, data.device, source="bytes")
    status = torch.empty(n, dtype=torch.int32, device=data.device)
    if n == 0:
        return (result, status) if return_status else result   # an empty tensor has no data pointer to hand to the library
    lib = _lib.load()
    ws = _ws(lib.dcv_xtc_decode_workspace(n), data.device)
    check(lib.dcv_xtc_decode(data.data_ptr(), data.numel(), frames.ctypes.data, n, n_atoms, float(scale), out_ptr, ofs, oas, ocs,
                             _ptr(status), _ptr(ws), ws.numel(), _stream()), "dcv_xtc_decode")
    if return_status:
        return result, status
    bad = torch.nonzero(status)
    if bad.numel():
        f = int(bad[0])
        code = int(status[f])
        raise DcvError(f"xtc_decode: frame {f} of the {n} given did not decode: {_lib.XTC_STATUS.get(code, f'status {code}')} (corrupt or truncated file)")
    return result


def xtc_encode_slots(xyz: torch.Tensor, n_atoms: int, strides=None, frames=None, precision: float = 1000.0, inv_scale: float = 0.1,
                     slots: Optional[torch.Tensor] = None):
    """The first half of :func:`xtc_encode` (dcv_xtc_encode): every frame compressed into a slot of its own.  Returns
    ``(slots, desc, status)``: a uint8 device tensor of ``n * dcv_xtc_encode_slot_bytes(n_atoms)`` bytes (``slots`` when
    given: a contiguous uint8 buffer or view of at least that size), the descriptors as a host array of
    ``_lib.XTC_FRAME_DTYPE`` records (``offset`` is the slot's offset) and an int32 [n] device tensor of status words
    (0: encoded; ``_lib.XTC_ENC_STATUS``).  Arguments as in :func:`xtc_encode`."""
    _require_gpu(xyz, slots)
    n_atoms = int(n_atoms)
    if n_atoms < 1:
        raise DcvError(f"xtc_encode: {n_atoms} atoms")
    n_src, base, fs, as_, cs = _coordinates("xtc_encode", xyz, n_atoms, strides)
    if frames is not None:
        frames = np.ascontiguousarray(np.asarray(frames).reshape(-1), dtype=np.int64)
    n = n_src if frames is None else int(frames.size)
    lib = _lib.load()
    slot = int(lib.dcv_xtc_encode_slot_bytes(n_atoms))
    if slots is None:
        slots = torch.empty(n * slot, dtype=torch.uint8, device=xyz.device)
    elif slots.dim() != 1 or slots.dtype != torch.uint8 or not slots.is_contiguous() or slots.device != xyz.device:
        raise DcvError("xtc_encode: slots must be a contiguous 1-D uint8 buffer on the device of the coordinates")
    desc = torch.empty(n * _lib.XTC_FRAME_DTYPE.itemsize, dtype=torch.uint8, device=xyz.device)
    status = torch.empty(n, dtype=torch.int32, device=xyz.device)
    if n == 0:   # an empty tensor has no data pointer to hand to the library
        return slots, np.zeros(0, dtype=_lib.XTC_FRAME_DTYPE), status
    if n_src < 1:
        raise DcvError(f"xtc_encode: {n} frame indices into a trajectory without frames")
    ws = _ws(lib.dcv_xtc_encode_workspace(n), xyz.device)
    check(lib.dcv_xtc_encode(base, n_src, max(fs, 1) if n_src == 1 else fs, as_, cs, n_atoms, None if frames is None else frames.ctypes.data, n,
                             float(inv_scale), float(precision), _ptr(slots), slots.numel(), _ptr(desc), _ptr(status), _ptr(ws), ws.numel(),
                             _stream()), "dcv_xtc_encode")
    return slots, desc.cpu().numpy().view(_lib.XTC_FRAME_DTYPE).reshape(-1), status


def xtc_image_offsets(desc: np.ndarray, status: np.ndarray, n_atoms: int) -> Tuple[np.ndarray, int]:
    """(offsets, bytes): where every frame begins in the file image -- the prefix sum over 56 + 36 + nbytes rounded up to 4
    (56 + 12 n_atoms for raw frames) of the frames that are not marked, -1 for the marked ones -- and the image's size."""
    good = np.asarray(status) == 0
    size = np.full(len(desc), 56 + 12 * int(n_atoms), dtype=np.int64) if n_atoms <= 9 else 92 + (desc["nbytes"].astype(np.int64) + 3) // 4 * 4
    size = np.where(good, size, 0)
    offsets = np.cumsum(size) - size
    offsets[~good] = -1
    return np.ascontiguousarray(offsets, dtype=np.int64), int(size.sum())


def xtc_pack(slots: torch.Tensor, desc: np.ndarray, offsets: np.ndarray, n_atoms: int, step, time, box=None,
             image: Optional[torch.Tensor] = None, image_bytes: Optional[int] = None) -> torch.Tensor:
    """The second half of :func:`xtc_encode` (dcv_xtc_pack): the slots copied behind their headers into one file image
    (a uint8 device tensor of ``image_bytes``, or ``image`` when given).  ``desc`` and ``offsets`` (-1: not packed) on the
    host, ``step`` int32 [n], ``time`` float32 [n], ``box`` float32 [n, 3, 3] or None (zeros)."""
    _require_gpu(slots, image)
    n = len(desc)
    desc = np.ascontiguousarray(desc)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    step = np.ascontiguousarray(np.asarray(step).reshape(-1), dtype=np.int32)
    time = np.ascontiguousarray(np.asarray(time).reshape(-1), dtype=np.float32)
    if desc.dtype != _lib.XTC_FRAME_DTYPE or offsets.size != n or step.size != n or time.size != n:
        raise DcvError(f"xtc_pack: {n} descriptors of {desc.dtype}, {offsets.size} offsets, {step.size} steps and {time.size} times")
    if box is not None:
        box = np.ascontiguousarray(np.asarray(box, dtype=np.float32).reshape(-1))
        if box.size != 9 * n:
            raise DcvError(f"xtc_pack: box must hold 9 values for each of the {n} frames, got {box.size}")
    if image is None:
        image = torch.empty(int(image_bytes), dtype=torch.uint8, device=slots.device)
    elif image.dim() != 1 or image.dtype != torch.uint8 or not image.is_contiguous() or image.device != slots.device:
        raise DcvError("xtc_pack: image must be a contiguous 1-D uint8 buffer on the device of the slots")
    if n == 0:
        return image
    lib = _lib.load()
    ws = _ws(lib.dcv_xtc_pack_workspace(n), slots.device)
    check(lib.dcv_xtc_pack(_ptr(slots), slots.numel(), desc.ctypes.data, offsets.ctypes.data, step.ctypes.data, time.ctypes.data,
                           None if box is None else box.ctypes.data, n, int(n_atoms), _ptr(image) if image.numel() else _ptr(ws), image.numel(),
                           _ptr(ws), ws.numel(), _stream()), "dcv_xtc_pack")
    return image


def xtc_encode(xyz: torch.Tensor, n_atoms: int, strides=None, frames=None, precision: float = 1000.0, inv_scale: float = 0.1, step=None,
               time=None, box=None, return_status: bool = False):
    """Frames written as a GROMACS ``.xtc`` file image on the device (dcv_xtc_encode, dcv_xtc_pack).  Returns the image
    as a uint8 device tensor: the bytes of a file that holds the frames in the order given.

    ``xyz``, ``n_atoms`` and ``strides`` as in :func:`featurize` (Angstrom; ``inv_scale`` 0.1 makes the file's
    nanometres).  ``frames``: indices of the source frames to write, in any order, repeats allowed (None: all, in
    order) -- the frames of a cluster are gathered by the encoder itself.  ``precision``: the file's precision (1000:
    0.001 nm).  ``step`` (int32), ``time`` (float32) and ``box`` ([n, 3, 3] float32, nm) fill the frame headers; the
    defaults are the source frame index, that index as float32, and zeros.
    Internally: encode into per-frame slots, download the descriptors, prefix sum of the lengths on the host, pack.
    A frame with a NaN or infinite coordinate, or one that does not fit a 32-bit integer at this precision, raises
    DcvError naming the first such frame; with ``return_status`` nothing is raised, the marked frames are absent from the
    image and ``(image, desc, status)`` is returned: the descriptors (host, ``_lib.XTC_FRAME_DTYPE``) and an int32 [n]
    device tensor (0: encoded)."""
    slots, desc, status = xtc_encode_slots(xyz, n_atoms, strides, frames, precision, inv_scale)
    n = len(desc)
    status_h = status.cpu().numpy()
    bad = np.flatnonzero(status_h)
    if bad.size and not return_status:
        code = int(status_h[bad[0]])
        raise DcvError(f"xtc_encode: frame {int(bad[0])} of the {n} given cannot be written: {_lib.XTC_ENC_STATUS.get(code, f'status {code}')}")
    source = np.arange(n, dtype=np.int64) if frames is None else np.asarray(frames, dtype=np.int64).reshape(-1)
    step = source if step is None else step
    time = source.astype(np.float32) if time is None else time
    offsets, image_bytes = xtc_image_offsets(desc, status_h, int(n_atoms))
    image = xtc_pack(slots, desc, offsets, n_atoms, step, time, box, image_bytes=image_bytes)
    return (image, desc, status) if return_status else image


def normalize(X: torch.Tensor, mean: torch.Tensor, rng: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(x - mean) / range in float32; ``out`` may be X itself (in place)."""
    _require_gpu(X, mean, rng, out)
    _check_matrix(X)
    if out is None:
        out = torch.empty_like(X)
    _check_matrix(out)
    n, F = X.shape
    if out.shape != X.shape or out.device != X.device:
        raise DcvError(f"normalize: out has shape {tuple(out.shape)} on {out.device}, X {tuple(X.shape)} on {X.device}")
    _check_vector(mean, F, "normalize: mean", X.device)
    _check_vector(rng, F, "normalize: range", X.device)
    check(_lib.load().dcv_normalize(_ptr(X), _ptr(out), n, F, X.stride(0), out.stride(0), _ptr(mean), _ptr(rng), _stream()),
          "dcv_normalize")
    return out


# ------------------------------------------------------------------------------- covariance
def lagged_cov_raw(X: torch.Tensor, n_pairs: int, lag: int, shift: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Raw sums [a (F) | b (F) | A (F*F) | B (F*F)] float64 over pairs (i, i+lag), i < n_pairs."""
    _require_gpu(X, shift)
    _check_matrix(X)
    lib = _lib.load()
    n, F = X.shape
    if n_pairs + lag > n:
        raise DcvError(f"lagged_cov: n_pairs + lag = {n_pairs + lag} exceeds the {n} rows available")
    _check_vector(shift, F, "lagged_cov: shift", X.device)
    out = torch.empty(2 * F + 2 * F * F, dtype=torch.float64, device=X.device)
    ws = _ws(lib.dcv_lagged_cov_workspace(n_pairs, F, lag), X.device)
    check(lib.dcv_lagged_cov(_ptr(X), n_pairs, F, X.stride(0), lag, _ptr(shift), _ptr(out), _ptr(ws), ws.numel(), _stream()),
          "dcv_lagged_cov")
    return out


def covariances_from_raw(raw: np.ndarray, n_pairs: int, F: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(mu_z, C0, Ctau) in float64 from (all-reduced) raw sums, following
    mlcolvar TICA.compute: mean of x_t removed from both, both
    matrices divided by the number of pairs and symmetrised."""
    a = raw[:F]
    b = raw[F:2 * F]
    A = raw[2 * F:2 * F + F * F].reshape(F, F)
    B = raw[2 * F + F * F:].reshape(F, F)
    P = float(n_pairs)
    delta = a / P
    C0 = A / P - np.outer(delta, delta)
    Ct = B / P - np.outer(delta, b / P)
    C0 = 0.5 * (C0 + C0.T)
    Ct = 0.5 * (Ct + Ct.T)
    return delta, C0, Ct


# ------------------------------------------------------------------------------- projection
def project_linear(X: torch.Tensor, W: torch.Tensor, *, fmean=None, frange=None, bias=None, cvmean=None, cvrange=None,
                   want_out=True, want_minmax=False):
    """out = (((x - fmean)/frange) @ W + bias - cvmean)/cvrange ; optional per-column min/max."""
    _require_gpu(X, W, fmean, frange, bias, cvmean, cvrange)
    _check_matrix(X)
    lib = _lib.load()
    n, F = X.shape
    if W.dim() != 2 or W.shape[0] != F or not W.is_contiguous() or W.dtype != torch.float32:
        raise DcvError("project_linear: W must be a contiguous float32 F x d tensor")
    d = W.shape[1]
    for v, length, name in ((fmean, F, "fmean"), (frange, F, "frange"), (bias, d, "bias"), (cvmean, d, "cvmean"),
                            (cvrange, d, "cvrange")):
        _check_vector(v, length, "project_linear: " + name, X.device)
    out = torch.empty(n, d, dtype=torch.float32, device=X.device) if want_out else None
    mm = torch.empty(2, d, dtype=torch.float32, device=X.device) if want_minmax else None
    ws = _ws(lib.dcv_project_linear_workspace(n, F, d), X.device)
    check(lib.dcv_project_linear(_ptr(X), n, F, X.stride(0), _ptr(fmean), _ptr(frange), _ptr(W), d, _ptr(bias),
                                 _ptr(cvmean), _ptr(cvrange), _ptr(out), _ptr(mm), _ptr(ws), ws.numel(), _stream()),
          "dcv_project_linear")
    return out, mm


# ------------------------------------------------------------------------------- GEMM block
def gemm(mode: str, A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """Building block (tests): 'nt' A[M,K].B[N,K]^T, 'nn' A[M,K].B[K,N], 'tn' A[K,M]^T.B[K,N].  Any row stride, unit column
    stride.  The tile family follows the extents and the CU count (gemm_log() says which was launched):
    tests/test_kernels_gpu.py covers the narrow, 64 x 128 and (TN) 64 x 64 tiles, tests/test_gemm_tiles_gpu.py the 128 x 128
    and 64 x 64 families in every mode."""
    _require_gpu(A, B)
    _check_matrix(A)
    _check_matrix(B)
    m = {"nt": 0, "nn": 1, "tn": 2}[mode]
    if m == 0:
        M, K = A.shape
        N = B.shape[0]
    elif m == 1:
        M, K = A.shape
        N = B.shape[1]
    else:
        K, M = A.shape
        N = B.shape[1]
    Cm = torch.empty(M, N, dtype=torch.float32, device=A.device)
    check(_lib.load().dcv_gemm_f32(m, _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(Cm), Cm.stride(0), M, N, K, _stream()),
          "dcv_gemm_f32")
    return Cm


def gemm_tn_split(A: torch.Tensor, B: torch.Tensor, k_chunk: int, slab_cap: int) -> torch.Tensor:
    """Split-K A[K,M]^T.B[K,N]: slabs [ceil(K / k_chunk), M, N]; raises when slab_cap slabs are too few."""
    _require_gpu(A, B)
    _check_matrix(A)
    _check_matrix(B)
    K, M = A.shape
    N = B.shape[1]
    slab = torch.full((slab_cap + 1, M, N), float("nan"), dtype=torch.float32, device=A.device)   # one guard slab behind the capacity
    check(_lib.load().dcv_gemm_tn_split(_ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(slab), slab_cap, M, N, K, int(k_chunk), _stream()),
          "dcv_gemm_tn_split")
    return slab


# ------------------------------------------------------------------------------- launch-plan log (test hook)
GemmLaunch = collections.namedtuple("GemmLaunch", "form mode tm tn split vec gather splits tail_split")
_GEMM_FORMS = ("single", "group", "pair", "ride")
_GEMM_MODES = ("nt", "nn", "tn")


def gemm_log_reset() -> None:
    """Forget the product plans recorded so far (dcv_debug_gemm_log_reset)."""
    _lib.load().dcv_debug_gemm_log_reset()


def gemm_log() -> list:
    """Plans of the block-engine products launched since the last reset, in launch order: GemmLaunch tuples of
    form ('single' | 'group' | 'pair' | 'ride'), mode ('nt' | 'nn' | 'tn'), tile rows and columns, split flavour, 16-byte
    loaders, gather-capable kernel form, split-K slabs and tail-tile chunks (0 = tail tile whole).  The log holds 256 entries;
    a replayed graph records nothing."""
    cap = 256
    buf = (C.c_int32 * (9 * cap))()
    n = min(int(_lib.load().dcv_debug_gemm_log_read(buf, cap)), cap)
    out = []
    for i in range(n):
        e = buf[9 * i:9 * i + 9]
        out.append(GemmLaunch(_GEMM_FORMS[e[0]], _GEMM_MODES[e[1]], e[2], e[3], bool(e[4]), bool(e[5]), bool(e[6]), e[7], e[8]))
    return out


# ------------------------------------------------------------------------------- arithmetic mode
def set_gemm_mode(mode: str) -> None:
    """'split' (default): FP32-accurate split products on the BF16 matrix pipe; 'native': FP32-input MFMA."""
    lib = _lib.load()
    check(lib.dcv_set_gemm_mode({"native": 0, "split": 1}[mode]), "dcv_set_gemm_mode")


def get_gemm_mode() -> str:
    return "split" if _lib.load().dcv_get_gemm_mode() == 1 else "native"


# ------------------------------------------------------------------------------- k-means
def kmeans_step(P: torch.Tensor, centers: torch.Tensor, labels: torch.Tensor, offset: Optional[torch.Tensor] = None,
                want_mindist=False):
    """One Lloyd E-step + accumulation.  Returns (acc, mindist) with
    acc = [sums (k*d) | counts (k) | inertia | changed] float64 on the device."""
    _require_gpu(P, centers, labels, offset)
    _check_matrix(P, torch.float64)
    lib = _lib.load()
    n, d = P.shape
    k = centers.shape[0]
    acc = torch.empty(k * d + k + 2, dtype=torch.float64, device=P.device)
    md = torch.empty(n, dtype=torch.float64, device=P.device) if want_mindist else None
    ws = _ws(lib.dcv_kmeans_workspace(n, d, k), P.device)
    check(lib.dcv_kmeans_step(_ptr(P), n, d, _ptr(offset), _ptr(centers), k, _ptr(labels), _ptr(acc), _ptr(md), _ptr(ws), ws.numel(), _stream()),
          "dcv_kmeans_step")
    return acc, md


def kmeanspp_update(P: torch.Tensor, centre: torch.Tensor, closest: torch.Tensor, first: bool, offset: Optional[torch.Tensor] = None) -> torch.Tensor:
    """closest = first ? dist(., centre) : min(closest, dist(., centre)) in place; returns the new potential (1-element float64)."""
    _require_gpu(P, centre, closest, offset)
    _check_matrix(P, torch.float64)
    lib = _lib.load()
    n, d = P.shape
    if n == 0:   # an empty shard of a frame-sharded run contributes nothing
        return torch.zeros(1, dtype=torch.float64, device=P.device)
    pot = torch.empty(1, dtype=torch.float64, device=P.device)
    ws = _ws(lib.dcv_kmeanspp_workspace(n, 1), P.device)
    check(lib.dcv_kmeanspp_update(_ptr(P), n, d, _ptr(offset), _ptr(centre), 1 if first else 0, _ptr(closest), _ptr(pot), _ptr(ws), ws.numel(),
                                  _stream()), "dcv_kmeanspp_update")
    return pot


def kmeanspp_potentials(P: torch.Tensor, cand: torch.Tensor, closest: torch.Tensor, offset: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pot[t] = sum_i min(closest_i, dist(x_i, cand_t)) for the candidate centres cand (trials x d, offset frame)."""
    _require_gpu(P, cand, closest, offset)
    _check_matrix(P, torch.float64)
    lib = _lib.load()
    n, d = P.shape
    t = cand.shape[0]
    if n == 0:
        return torch.zeros(t, dtype=torch.float64, device=P.device)
    pot = torch.empty(t, dtype=torch.float64, device=P.device)
    ws = _ws(lib.dcv_kmeanspp_workspace(n, t), P.device)
    check(lib.dcv_kmeanspp_potentials(_ptr(P), n, d, _ptr(offset), _ptr(cand.contiguous()), t, _ptr(closest), _ptr(pot), _ptr(ws), ws.numel(),
                                      _stream()), "dcv_kmeanspp_potentials")
    return pot


def label_stats(P: torch.Tensor, labels: torch.Tensor, k: int, centers: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[sums (k*d) | counts (k) | sum ||x - c||^2 (k) | sum ||x - c|| (k)] per label, float64 on the device
    (the last two groups about `centers` when given)."""
    _require_gpu(P, labels, centers)
    _check_matrix(P, torch.float64)
    lib = _lib.load()
    n, d = P.shape
    acc = torch.empty(k * d + 3 * k, dtype=torch.float64, device=P.device)
    ws = _ws(lib.dcv_label_stats_workspace(n, d, k), P.device)
    check(lib.dcv_label_stats(_ptr(P), n, d, _ptr(labels), _ptr(centers), k, _ptr(acc), _ptr(ws), ws.numel(), _stream()), "dcv_label_stats")
    return acc


def cluster_dist_sums(Q: torch.Tensor, P_sorted: torch.Tensor, start: torch.Tensor) -> torch.Tensor:
    """S[i][c] = sum_j in cluster c ||Q_i - P_j||; P_sorted holds cluster c in rows [start[c], start[c+1])."""
    _require_gpu(Q, P_sorted, start)
    _check_matrix(Q, torch.float64)
    _check_matrix(P_sorted, torch.float64)
    lib = _lib.load()
    nq, d = Q.shape
    k = start.numel() - 1
    S = torch.empty(nq, k, dtype=torch.float64, device=Q.device)
    check(lib.dcv_cluster_dist_sums(_ptr(Q), nq, _ptr(P_sorted), _ptr(start), k, d, _ptr(S), _stream()), "dcv_cluster_dist_sums")
    return S


def silhouette_sum(S: torch.Tensor, qlabels: torch.Tensor, start: torch.Tensor) -> torch.Tensor:
    """Sum of the silhouette sample values of the queries (1-element float64 device tensor)."""
    _require_gpu(S, qlabels, start)
    lib = _lib.load()
    nq, k = S.shape
    out = torch.empty(1, dtype=torch.float64, device=S.device)
    ws = _ws(lib.dcv_silhouette_sum_workspace(nq), S.device)
    check(lib.dcv_silhouette_sum(_ptr(S), nq, k, _ptr(qlabels), _ptr(start), _ptr(out), _ptr(ws), ws.numel(), _stream()), "dcv_silhouette_sum")
    return out


def linear_binning(P: torch.Tensor, cols, lo, hi, bins: int):
    """Linear-binning weights of the points on a bins^d grid over [lo, hi] (d = len(cols) <= 2): (grid float64 device
    tensor of shape (bins,) or (bins, bins), number of points outside the bounds)."""
    import ctypes as C

    _require_gpu(P)
    _check_matrix(P, torch.float64)
    lib = _lib.load()
    d = len(cols)
    cols_a = (C.c_int32 * d)(*[int(c) for c in cols])
    lo_a = (C.c_double * d)(*[float(v) for v in lo])
    hi_a = (C.c_double * d)(*[float(v) for v in hi])
    grid = torch.empty((bins,) * d, dtype=torch.float64, device=P.device)
    ws = _ws(lib.dcv_linear_binning_workspace(d, bins), P.device)
    out = C.c_int64(0)
    check(lib.dcv_linear_binning(_ptr(P), P.shape[0], P.stride(0), d, cols_a, lo_a, hi_a, int(bins), _ptr(grid), C.byref(out), _ptr(ws),
                                 ws.numel(), _stream()), "dcv_linear_binning")
    return grid, int(out.value)


def nearest_rows(P: torch.Tensor, centers: torch.Tensor, row_offset: int = 0):
    """Per centroid: (distance, global row) of the nearest point (np.linalg.norm, first index on ties)."""
    _require_gpu(P, centers)
    _check_matrix(P, torch.float64)
    lib = _lib.load()
    n, d = P.shape
    k = centers.shape[0]
    dist = torch.empty(k, dtype=torch.float64, device=P.device)
    rows = torch.empty(k, dtype=torch.int64, device=P.device)
    ws = _ws(lib.dcv_nearest_rows_workspace(n, d, k), P.device)
    check(lib.dcv_nearest_rows(_ptr(P), n, d, _ptr(centers), k, row_offset, _ptr(dist), _ptr(rows), _ptr(ws), ws.numel(), _stream()),
          "dcv_nearest_rows")
    return dist, rows


def nearest_point(train: torch.Tensor, sup: torch.Tensor) -> torch.Tensor:
    _require_gpu(train, sup)
    _check_matrix(train, torch.float64)
    _check_matrix(sup, torch.float64)
    nn = torch.empty(sup.shape[0], dtype=torch.int64, device=sup.device)
    check(_lib.load().dcv_nearest_point(_ptr(train.contiguous()), train.shape[0], _ptr(sup.contiguous()), sup.shape[0],
                                        train.shape[1], _ptr(nn), _stream()), "dcv_nearest_point")
    return nn


LINKAGE_METHOD = {"complete": 0, "average": 1, "ward": 2}


def linkage_workspace_bytes(n: int, d: int) -> int:
    return int(_lib.load().dcv_linkage_workspace(n, d))


def linkage(P: torch.Tensor, method: str = "complete", return_searches: bool = False):
    """scipy.cluster.hierarchy.linkage(P, method, "euclidean") for method in complete / average / ward on the GPU:
    the (n - 1) x 4 float64 linkage matrix as a NumPy array, equal to scipy's (dcv_linkage).  P is n x d float64 on
    the device, finite, n >= 2, d <= 16.  With `return_searches` also the number of row searches the chain ran."""
    _require_gpu(P)
    _check_matrix(P, torch.float64)
    if method not in LINKAGE_METHOD:
        raise DcvError(f"linkage: method {method!r} is not one of {sorted(LINKAGE_METHOD)}")
    P = P.contiguous()
    n, d = P.shape
    # a NaN never compares below anything: the chain would find no neighbour.  Refused here; the kernels keep their own guard
    if n > 0 and not bool(torch.isfinite(P).all()):
        raise DcvError("linkage failed (code -1): the points hold NaN or infinite values")
    import ctypes as C

    lib = _lib.load()
    Z = np.empty((max(n - 1, 0), 4), dtype=np.float64)
    searches = C.c_int64(0)
    nbytes = lib.dcv_linkage_workspace(n, d)
    ws = _ws(nbytes, P.device) if nbytes else None   # 0: the arguments are out of range, dcv_linkage says which
    check(lib.dcv_linkage(_ptr(P), n, d, LINKAGE_METHOD[method], Z.ctypes.data, C.byref(searches), _ptr(ws), nbytes, _stream()),
          "dcv_linkage")
    return (Z, int(searches.value)) if return_searches else Z


CORE_MAX_K = 64   # min_samples dcv_core_distances holds per query


def _check_points(P: torch.Tensor, what: str):
    _require_gpu(P)
    _check_matrix(P, torch.float64)
    n, d = P.shape
    if not (2 <= n < 2 ** 31) or not (1 <= d <= 16):
        raise DcvError(f"{what} failed (code -1): {n} points in {d} dimensions, supported n >= 2, 1 <= d <= 16")
    # a NaN never compares below anything: no neighbour, no candidate.  Refused here; the kernels keep their own guard
    if not bool(torch.isfinite(P).all()):
        raise DcvError(f"{what} failed (code -1): the points hold NaN or infinite values")


def core_distances_workspace_bytes(n: int, d: int, k: int) -> int:
    return int(_lib.load().dcv_core_distances_workspace(n, d, k))


def core_distances(P: torch.Tensor, k: int) -> torch.Tensor:
    """NearestNeighbors(n_neighbors=k).kneighbors(P)[0][:, -1] on the GPU: for every point the k-th smallest Euclidean
    distance to all points, itself included -- HDBSCAN's core distances with min_samples = k, equal to scikit-learn's
    (dcv_core_distances).  P is n x d float64 on the device, finite, n >= 2, d <= 16, 1 <= k <= min(n, CORE_MAX_K).
    Returns a float64 device tensor of n entries."""
    _check_points(P, "core_distances")
    P = P.contiguous()
    n, d = P.shape
    k = int(k)
    if not (1 <= k <= min(n, CORE_MAX_K)):
        raise DcvError(f"core_distances failed (code -1): k = {k}, supported 1..min(n, {CORE_MAX_K})")
    lib = _lib.load()
    core = torch.empty(n, dtype=torch.float64, device=P.device)
    nbytes = lib.dcv_core_distances_workspace(n, d, k)
    ws = _ws(nbytes, P.device)
    check(lib.dcv_core_distances(_ptr(P), n, d, k, _ptr(core), _ptr(ws), nbytes, _stream()), "dcv_core_distances")
    return core


def mr_mst_workspace_bytes(n: int, d: int) -> int:
    return int(_lib.load().dcv_mr_mst_workspace(n, d))


def mr_mst(P: torch.Tensor, core: torch.Tensor) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """sklearn's mst_from_data_matrix(P, core, Euclidean, alpha=1) on the GPU: the minimum spanning tree of the mutual
    reachability graph by Prim's algorithm from node 0.  Returns NumPy arrays (src int64, dst int64, w float64) of
    n - 1 edges in Prim order, equal to scikit-learn's (dcv_mr_mst).  `core`: n float64 on the device, finite."""
    _check_points(P, "mr_mst")
    _require_gpu(core)
    P = P.contiguous()
    n, d = P.shape
    if core.dtype != torch.float64 or core.dim() != 1 or core.shape[0] != n:
        raise DcvError(f"mr_mst failed (code -1): expected {n} float64 core distances, got shape {tuple(core.shape)} dtype {core.dtype}")
    core = core.contiguous()
    if not bool(torch.isfinite(core).all()):
        raise DcvError("mr_mst failed (code -1): the core distances hold NaN or infinite values")
    lib = _lib.load()
    src = np.empty(n - 1, dtype=np.int64)
    dst = np.empty(n - 1, dtype=np.int64)
    w = np.empty(n - 1, dtype=np.float64)
    nbytes = lib.dcv_mr_mst_workspace(n, d)
    ws = _ws(nbytes, P.device)
    check(lib.dcv_mr_mst(_ptr(P), n, d, _ptr(core), src.ctypes.data, dst.ctypes.data, w.ctypes.data, _ptr(ws), nbytes, _stream()),
          "dcv_mr_mst")
    return src, dst, w


# ------------------------------------------------------------------------------- MLP engine
class RcclComm:
    """RCCL communicator owned by the library (dcv_comm_*): the collectives of a data-parallel step are then issued by
    libdcv.so itself, in stream order with its kernels.  `dist` (an initialised torch.distributed, any backend) is used
    once, to hand rank 0's 128-byte unique id to the other ranks; world = 1 needs no bootstrap at all."""

    def __init__(self, dist=None, device="cuda"):
        import ctypes as C

        self.lib = _lib.load()
        world = dist.get_world_size() if dist is not None else 1
        rank = dist.get_rank() if dist is not None else 0
        uid = (C.c_uint8 * 128)()
        if rank == 0:
            check(self.lib.dcv_comm_unique_id(uid), "dcv_comm_unique_id")
        if world > 1:
            backend = dist.get_backend()
            t = torch.tensor(list(uid), dtype=torch.uint8, device=device if backend == "nccl" else "cpu")
            dist.broadcast(t, src=0)
            uid = (C.c_uint8 * 128)(*t.cpu().tolist())
        h = C.c_void_p()
        check(self.lib.dcv_comm_create(world, rank, uid, C.byref(h)), "dcv_comm_create")
        self.h, self.world, self.rank = h, world, rank

    def all_reduce(self, t: torch.Tensor, op: str = "sum"):
        _require_gpu(t)
        dt = {torch.float32: 0, torch.float64: 1}[t.dtype]
        check(self.lib.dcv_comm_allreduce(self.h, _ptr(t), t.numel(), dt, {"sum": 0, "min": 1, "max": 2}[op], _stream()), "dcv_comm_allreduce")

    def close(self):
        if getattr(self, "h", None):
            self.lib.dcv_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mlp:
    """Owner of a ``dcv_mlp`` handle (Deep-TICA, autoencoder or variational autoencoder chain of Linear layers; for "vae"
    the Linear at ``latent_layer - 1`` is the two heads [mean | log-variance] concatenated, see dcv.h DCV_MODEL_VAE).

    ``dims`` = [F, ..., out]; ``acts`` one activation name per Linear.  Parameters are kept
    in the library's flat device buffer; ``set_linear`` / ``get_linear`` move torch-layout
    (out x in weight, out bias) tensors in and out."""

    def __init__(self, model: str, dims, acts, *, max_batch: int, lag: int = 0, tica_reg: float = 1e-6,
                 latent_layer: Optional[int] = None, lr: float = 1e-3, betas=(0.9, 0.999), eps: Optional[float] = None,
                 weight_decay: float = 0.0, optimizer: str = "Adam", amsgrad: bool = False, momentum: float = 0.0,
                 dampening: float = 0.0, nesterov: bool = False, alpha: float = 0.99, centered: bool = False,
                 lr_decay: float = 0.0, initial_accumulator_value: float = 0.0, opt_params=None, dropout=None, seed: int = 0,
                 batchnorm=None, bn_eps: float = 1e-5, bn_momentum: float = 0.1, maximize: bool = False, device="cuda"):
        import ctypes as C

        if not torch.cuda.is_available():
            raise DcvError("the MLP engine needs an MI355X: torch.cuda.is_available() is False and there is no CPU path")
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.model = model
        self.dims = [int(x) for x in dims]
        self.acts = list(acts)
        L = len(self.dims) - 1
        if len(self.acts) != L:
            raise DcvError("one activation per Linear layer expected")
        desc = _lib.MlpDesc()
        desc.model = {"deep_tica": _lib.MODEL_DEEPTICA, "ae": _lib.MODEL_AE, "vae": _lib.MODEL_VAE}[model]
        desc.n_layers = L
        for i, v in enumerate(self.dims):
            desc.dims[i] = v
        for i, a in enumerate(self.acts):
            if a not in _lib.ACT:
                raise DcvError(f"activation {a!r} is not implemented by the HIP engine")
            desc.act[i] = _lib.ACT[a]
        desc.latent_layer = L if latent_layer is None else int(latent_layer)
        desc.lag = int(lag)
        desc.max_batch = int(max_batch)
        desc.tica_reg = float(tica_reg)
        if eps is None:   # torch's default for the optimiser
            eps = {"Adagrad": 1e-10, "Adadelta": 1e-6}.get(optimizer, 1e-8)
        desc.lr, desc.beta1, desc.beta2, desc.eps, desc.weight_decay = float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay)
        if optimizer not in _lib.OPTIMIZER:
            raise DcvError(f"optimizer {optimizer!r} is not implemented by the HIP engine (have: {sorted(_lib.OPTIMIZER)})")
        desc.optimizer = _lib.OPTIMIZER[optimizer]
        desc.amsgrad, desc.nesterov, desc.centered = int(bool(amsgrad)), int(bool(nesterov)), int(bool(centered))
        desc.momentum, desc.dampening, desc.alpha = float(momentum), float(dampening), float(alpha)
        desc.lr_decay, desc.initial_accumulator_value = float(lr_decay), float(initial_accumulator_value)
        for i, v in enumerate(list(opt_params or [])[:4]):   # further constants of Adamax / NAdam / RAdam / Adadelta / ASGD / Rprop (dcv.h: DCV_OPT_*)
            desc.opt_p[i] = float(v)
        self.batchnorm = [bool(b) for b in (batchnorm if batchnorm is not None else [False] * L)]
        if len(self.batchnorm) != L:
            raise DcvError("one batchnorm flag per Linear layer expected")
        for i, b in enumerate(self.batchnorm):
            desc.batchnorm[i] = 1 if b else 0
        desc.bn_eps, desc.bn_momentum = float(bn_eps), float(bn_momentum)
        desc.maximize = 1 if maximize else 0
        self.dropout = [float(p or 0.0) for p in (dropout if dropout is not None else [0.0] * L)]
        if len(self.dropout) != L:
            raise DcvError("one dropout probability per Linear layer expected")
        for i, p in enumerate(self.dropout):
            desc.dropout[i] = p
        desc.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        h = C.c_void_p()
        check(self.lib.dcv_mlp_create(C.byref(desc), C.byref(h)), "dcv_mlp_create")
        self.h = h
        self.L = L
        self.latent_layer = desc.latent_layer
        # input width of each Linear: dims[l], except the VAE's first decoder Linear, which reads z (half the heads' 2d outputs)
        self.in_dims = [self.dims[l] // 2 if model == "vae" and l == self.latent_layer else self.dims[l] for l in range(L)]
        self.max_batch = int(max_batch)
        self.rows_cap = 2 * self.max_batch if model == "deep_tica" else self.max_batch
        self.n_params = self.lib.dcv_mlp_num_params(self.h)
        self.offsets = [(self.lib.dcv_mlp_param_offset(self.h, l, 0), self.lib.dcv_mlp_param_offset(self.h, l, 1)) for l in range(L)]
        self.bn_offsets = [(self.lib.dcv_mlp_param_offset(self.h, l, 2), self.lib.dcv_mlp_param_offset(self.h, l, 3)) for l in range(L)]
        self.log_width = self.lib.dcv_mlp_log_width(self.h)
        self.stats_len = self.lib.dcv_mlp_stats_len(self.h)
        self._log_cap = 0
        self._dp = None            # state of data_parallel_step (callback thunk, tensor views of the library's buffers)
        self._upper_thunk = None   # ctypes thunk of backward(on_upper_grads=...)
        self._upper_fn = None
        self._upper_err = None
        self._noise = None         # VAE: the device noise buffer the engine reads (kept alive here)

    def close(self):
        if getattr(self, "h", None):
            self.lib.dcv_mlp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- parameters
    def set_linears(self, linears, bn=None):
        """linears: list of (weight[out,in], bias[out]) CPU float32 tensors / arrays.  bn (optional): per Linear, None or a
        dict(weight, bias, running_mean, running_var, num_batches_tracked) of the BatchNorm1d behind it; layers with a
        normalisation and no entry start as a fresh BatchNorm1d (weight 1, bias 0, running mean 0 / variance 1)."""
        flat = np.zeros(self.n_params, dtype=np.float32)
        for l in range(self.L):
            if self.batchnorm[l]:
                go, bo_ = self.bn_offsets[l]
                d = (bn[l] if bn is not None else None) or {}
                flat[go: go + self.dims[l + 1]] = np.asarray(d.get("weight", np.ones(self.dims[l + 1])), dtype=np.float32)
                flat[bo_: bo_ + self.dims[l + 1]] = np.asarray(d.get("bias", np.zeros(self.dims[l + 1])), dtype=np.float32)
        for l, (w, b) in enumerate(linears):
            w = np.asarray(w, dtype=np.float32)
            b = np.asarray(b, dtype=np.float32)
            if w.shape != (self.dims[l + 1], self.in_dims[l]) or b.shape != (self.dims[l + 1],):
                raise DcvError(f"layer {l}: expected weight {(self.dims[l + 1], self.in_dims[l])}, got {w.shape}")
            wo, bo = self.offsets[l]
            flat[wo: wo + w.size] = w.ravel()
            flat[bo: bo + b.size] = b
        check(self.lib.dcv_mlp_set_params(self.h, flat.ctypes.data, _stream()), "dcv_mlp_set_params")
        if bn is not None:
            import ctypes as C

            for l in range(self.L):
                if self.batchnorm[l] and bn[l] is not None and "running_mean" in bn[l]:
                    rm = np.ascontiguousarray(np.asarray(bn[l]["running_mean"], dtype=np.float32))
                    rv = np.ascontiguousarray(np.asarray(bn[l]["running_var"], dtype=np.float32))
                    nbt = C.c_int64(int(bn[l].get("num_batches_tracked", 0)))
                    check(self.lib.dcv_mlp_bn_state(self.h, l, rm.ctypes.data, rv.ctypes.data, C.byref(nbt), 1, _stream()), "dcv_mlp_bn_state")

    def get_bn(self):
        """Per Linear: None, or the state of the BatchNorm1d behind it (weight, bias, running_mean, running_var, num_batches_tracked)."""
        import ctypes as C

        flat = np.empty(self.n_params, dtype=np.float32)
        check(self.lib.dcv_mlp_get_params(self.h, flat.ctypes.data, _stream()), "dcv_mlp_get_params")
        out = []
        for l in range(self.L):
            if not self.batchnorm[l]:
                out.append(None)
                continue
            o = self.dims[l + 1]
            go, bo_ = self.bn_offsets[l]
            rm, rv, nbt = np.empty(o, np.float32), np.empty(o, np.float32), C.c_int64(0)
            check(self.lib.dcv_mlp_bn_state(self.h, l, rm.ctypes.data, rv.ctypes.data, C.byref(nbt), 0, _stream()), "dcv_mlp_bn_state")
            out.append({"weight": flat[go: go + o].copy(), "bias": flat[bo_: bo_ + o].copy(), "running_mean": rm, "running_var": rv,
                        "num_batches_tracked": int(nbt.value)})
        return out

    def get_linears(self):
        flat = np.empty(self.n_params, dtype=np.float32)
        check(self.lib.dcv_mlp_get_params(self.h, flat.ctypes.data, _stream()), "dcv_mlp_get_params")
        out = []
        for l in range(self.L):
            wo, bo = self.offsets[l]
            o, i = self.dims[l + 1], self.in_dims[l]
            out.append((flat[wo: wo + o * i].reshape(o, i).copy(), flat[bo: bo + o].copy()))
        return out

    def _flat_view(self, ptr, n, dtype):
        # a torch view over library-owned device memory (for all-reduce / inspection)
        import ctypes as C

        class _Holder:
            pass

        itemsize = torch.tensor([], dtype=dtype).element_size()
        holder = _Holder()
        holder.__cuda_array_interface__ = {
            "shape": (n,), "typestr": {torch.float32: "<f4", torch.float64: "<f8"}[dtype],
            "data": (int(ptr), False), "version": 2, "strides": (itemsize,)}
        return torch.as_tensor(holder, device=self.device)

    def grads_view(self) -> torch.Tensor:
        return self._flat_view(self.lib.dcv_mlp_grads(self.h), self.n_params, torch.float32)

    def params_view(self) -> torch.Tensor:
        return self._flat_view(self.lib.dcv_mlp_params(self.h), self.n_params, torch.float32)

    def stats_view(self) -> torch.Tensor:
        return self._flat_view(self.lib.dcv_mlp_stats(self.h), self.stats_len, torch.float64)

    def set_lr(self, lr: float):
        check(self.lib.dcv_mlp_set_lr(self.h, float(lr)), "dcv_mlp_set_lr")

    def set_momentum(self, value: float):
        """beta1 (Adam family) / momentum (SGD, RMSprop) of the following updates (cycled by OneCycleLR)."""
        check(self.lib.dcv_mlp_set_momentum(self.h, float(value)), "dcv_mlp_set_momentum")

    def last_path(self) -> int:
        """0 = layer by layer, 1 = fused small-network autoencoder step, 2 = fused small-network Deep-TICA kernels."""
        return int(self.lib.dcv_mlp_last_path(self.h))

    def last_ride(self) -> int:
        """Reduction workgroups that rode in the layer-0 weight-gradient launch of the last training backward (0: none)."""
        return int(self.lib.dcv_mlp_last_ride(self.h))

    def last_reduce(self) -> int:
        """Kernel of the final gradient reduction of the last training backward: 0 = none yet, 1 = flat-grid quad, 2 = 4-wave, 3 = 16-wave."""
        return int(self.lib.dcv_mlp_last_reduce(self.h))

    def opt_state_view(self, which: int) -> Optional[torch.Tensor]:
        """The optimiser's state tensor `which` (0, 1; 2 = the auxiliary one, None without it) as a view, laid out like params_view()."""
        ptr = self.lib.dcv_mlp_opt_state(self.h, int(which))
        return self._flat_view(ptr, self.n_params, torch.float32) if ptr else None

    def dropout_step(self) -> int:
        return int(self.lib.dcv_mlp_dropout_step(self.h))

    def dropout_mask(self, layer: int, step: int, rows: int) -> torch.Tensor:
        """keep / (1 - p) multipliers of the dropout behind Linear `layer` in training step `step` (test hook)."""
        out = torch.empty(rows, self.dims[layer + 1], dtype=torch.float32, device=self.device)
        check(self.lib.dcv_mlp_dropout_mask(self.h, int(layer), int(step), int(rows), _ptr(out), _stream()), "dcv_mlp_dropout_mask")
        return out

    def set_row_sharing(self, enable: bool):
        """Deep-TICA contiguous batches: share the rows of the two halves (default) or not."""
        check(self.lib.dcv_mlp_set_row_sharing(self.h, 1 if enable else 0), "dcv_mlp_set_row_sharing")

    def set_feature_range(self, rng):
        r = np.ascontiguousarray(np.asarray(rng, dtype=np.float32))
        check(self.lib.dcv_mlp_set_feature_range(self.h, r.ctypes.data, _stream()), "dcv_mlp_set_feature_range")

    # -- variational autoencoder
    def set_kl_beta(self, beta: float):
        """Weight of the KL term of the following VAE steps."""
        check(self.lib.dcv_mlp_set_kl_beta(self.h, float(beta)), "dcv_mlp_set_kl_beta")

    def set_noise(self, eps: torch.Tensor):
        """The standard-normal noise of the following VAE steps: a [rows, d] float32 device tensor read as a cursor, each
        training / evaluation step taking the next `batch` rows (rewinds the cursor; the tensor is kept alive here)."""
        _require_gpu(eps)
        eps = eps.to(torch.float32).contiguous()
        d = self.dims[self.latent_layer] // 2
        if eps.dim() != 2 or eps.shape[1] != d:
            raise DcvError(f"set_noise: expected a [rows, {d}] tensor, got {tuple(eps.shape)}")
        self._noise = eps
        check(self.lib.dcv_mlp_set_noise(self.h, _ptr(eps), int(eps.shape[0])), "dcv_mlp_set_noise")

    def noise_position(self) -> int:
        """Noise rows consumed since the last set_noise."""
        return int(self.lib.dcv_mlp_noise_position(self.h))

    def latent_sample(self, rows: int) -> torch.Tensor:
        """The sampled latent z of the last forward (test hook, layer-by-layer path)."""
        out = torch.empty(int(rows), self.dims[self.latent_layer] // 2, dtype=torch.float32, device=self.device)
        check(self.lib.dcv_mlp_latent_sample(self.h, int(rows), _ptr(out), _stream()), "dcv_mlp_latent_sample")
        return out

    # -- steps
    def _args(self, Xn, idx, row0, batch):
        _require_gpu(Xn, idx)
        _check_matrix(Xn)
        if idx is not None and (idx.dtype != torch.int64 or not idx.is_contiguous()):
            raise DcvError("batch indices must be a contiguous int64 device tensor")
        return _ptr(Xn), Xn.stride(0), _ptr(idx), int(row0), int(batch)

    def forward(self, Xn, idx=None, row0=0, batch=None, train=True):
        batch = int(batch if batch is not None else idx.numel())
        check(self.lib.dcv_mlp_forward(self.h, *self._args(Xn, idx, row0, batch), 1 if train else 0, _stream()), "dcv_mlp_forward")

    def backward(self, Xn, idx=None, row0=0, batch=None, global_batch=None, train=True, on_upper_grads=None):
        """`on_upper_grads`: host callable invoked inside the call once the gradients of layers 1.. are reduced into
        upper_grads_view() and before the layer-0 weight gradient is enqueued (data-parallel overlap hook)."""
        import ctypes as C

        batch = int(batch if batch is not None else idx.numel())
        gb = int(global_batch if global_batch is not None else batch)
        use_cb = on_upper_grads is not None and train and self.L > 1
        if use_cb:
            if self._upper_thunk is None:   # one thunk per engine; the Python callable of the current call sits in a cell

                def _tramp(_u):
                    try:
                        self._upper_fn()
                    except BaseException as e:   # ctypes would print and swallow it
                        self._upper_err = e

                self._upper_thunk = C.CFUNCTYPE(None, C.c_void_p)(_tramp)
            self._upper_fn, self._upper_err = on_upper_grads, None
            check(self.lib.dcv_mlp_set_upper_grads_callback(self.h, C.cast(self._upper_thunk, C.c_void_p), None), "dcv_mlp_set_upper_grads_callback")
        try:
            check(self.lib.dcv_mlp_backward(self.h, *self._args(Xn, idx, row0, batch), gb, 1 if train else 0, _stream()), "dcv_mlp_backward")
        finally:
            if use_cb:
                check(self.lib.dcv_mlp_set_upper_grads_callback(self.h, None, None), "dcv_mlp_set_upper_grads_callback")
                self._upper_fn = None
        if use_cb and self._upper_err is not None:
            e, self._upper_err = self._upper_err, None
            raise e

    def upper_grads_view(self) -> torch.Tensor:
        """Gradients of layers 1.. (the tail of the flat buffer)."""
        return self.grads_view()[self.offsets[1][0]:] if self.L > 1 else self.grads_view()[:0]

    def layer0_grads_view(self) -> torch.Tensor:
        return self.grads_view()[: self.offsets[1][0]] if self.L > 1 else self.grads_view()

    def data_parallel_step(self, Xn, dist, global_batch, idx=None, row0=0, batch=None, train=True, group=None):
        """One synchronous data-parallel step over `dist` (torch.distributed) as ONE library call (dcv_mlp_dp_step):
        forward, all-reduce of the batch statistics, backward, all-reduce of the gradient buffer (from 32 768 rows per
        rank up in two pieces, the upper layers' started under the layer-0 weight gradient; DCV_DP_OVERLAP=0|1 forces
        either form), optimiser update.  The collectives run in a host callback; an exception raised there (an RCCL
        error, say) aborts the step inside the library and is re-raised here -- never swallowed."""
        import ctypes as C

        rows = int(batch if batch is not None else idx.numel())
        if isinstance(dist, RcclComm):   # the library's own communicator: nothing of the step runs in Python
            env = os.environ.get("DCV_DP_OVERLAP")
            overlap = (rows >= 32768) if env is None else env == "1"
            check(self.lib.dcv_comm_bind_stream(dist.h, _stream()), "dcv_comm_bind_stream")
            check(self.lib.dcv_mlp_dp_step(self.h, *self._args(Xn, idx, row0, rows), int(global_batch), 1 if train else 0, 1 if overlap else 0,
                                           self.lib.dcv_comm_dp_allreduce_fn(), dist.h, _stream()), "dcv_mlp_dp_step")
            return
        env = os.environ.get("DCV_DP_OVERLAP")
        # The two-piece form pays one more collective launch (~15-20 us of latency at these message sizes) to hide the
        # upper layers' all-reduce under the layer-0 weight gradient: worth it only when that product outlasts a
        # collective -- not at a few thousand rows per rank (8192-pair global batch over 1-8 ranks).
        overlap = (rows >= 32768) if env is None else env == "1"
        st = self._dp
        if st is None:
            st = self._dp = {"views": {}, "pending": [], "error": None, "dist": None, "group": None}

            def _cb(_user, buf, count, dtype, phase):
                try:
                    if phase == 3:   # DCV_DP_WAIT
                        for w in st["pending"]:
                            w.wait()
                        st["pending"].clear()
                        return 0
                    key = (int(buf), int(count), int(dtype))
                    t = st["views"].get(key)
                    if t is None:
                        t = st["views"][key] = self._flat_view(buf, int(count), torch.float64 if dtype == 1 else torch.float32)
                    d = st["dist"]
                    if phase == 2:   # DCV_DP_UPPER_START
                        st["pending"].append(d.all_reduce(t, op=d.ReduceOp.SUM, group=st["group"], async_op=True))
                    else:
                        d.all_reduce(t, op=d.ReduceOp.SUM, group=st["group"])
                    return 0
                except BaseException as e:   # ctypes would print and swallow it: stash, fail the step, re-raise outside
                    st["error"] = e
                    return 1

            st["thunk"] = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32)(_cb)
        st["dist"], st["group"], st["error"] = dist, group, None
        st["pending"].clear()
        rc = self.lib.dcv_mlp_dp_step(self.h, *self._args(Xn, idx, row0, rows), int(global_batch), 1 if train else 0, 1 if overlap else 0,
                                      C.cast(st["thunk"], C.c_void_p), None, _stream())
        if st["error"] is not None:
            err, st["error"] = st["error"], None
            raise err
        check(rc, "dcv_mlp_dp_step")

    def set_rank(self, rank: int):
        """Rank of this engine in a data-parallel run (independent dropout masks per rank)."""
        check(self.lib.dcv_mlp_set_rank(self.h, int(rank)), "dcv_mlp_set_rank")

    def layer_output(self, layer: int, rows: int) -> torch.Tensor:
        """Post-activation output of Linear `layer` in the last forward (test hook)."""
        out = torch.empty(int(rows), self.dims[layer + 1], dtype=torch.float32, device=self.device)
        check(self.lib.dcv_mlp_layer_output(self.h, int(layer), int(rows), _ptr(out), _stream()), "dcv_mlp_layer_output")
        return out

    def apply(self):
        check(self.lib.dcv_mlp_apply(self.h, _stream()), "dcv_mlp_apply")

    def set_graph(self, enable: bool):
        """Opt in to hipGraph launches of the step entry points (needs a non-null stream)."""
        check(self.lib.dcv_mlp_set_graph(self.h, 1 if enable else 0), "dcv_mlp_set_graph")

    def graph_launches(self) -> int:
        """Calls of train_step / forward / backward / eval_step that went out as one hipGraph launch."""
        return int(self.lib.dcv_mlp_graph_launches(self.h))

    def train_step(self, Xn, idx=None, row0=0, batch=None):
        batch = int(batch if batch is not None else idx.numel())
        check(self.lib.dcv_mlp_train_step(self.h, *self._args(Xn, idx, row0, batch), _stream()), "dcv_mlp_train_step")

    def eval_step(self, Xn, idx=None, row0=0, batch=None):
        batch = int(batch if batch is not None else idx.numel())
        check(self.lib.dcv_mlp_eval_step(self.h, *self._args(Xn, idx, row0, batch), _stream()), "dcv_mlp_eval_step")

    def train_steps(self, Xn, batch: int, nsteps: int, idx=None, row0=0):
        """`nsteps` training steps in one call (constant learning rate): step j on idx[j * batch:(j + 1) * batch] (or rows
        row0 + j * batch ...), identical to nsteps train_step calls -- the per-call cost of the host is paid once."""
        batch, nsteps = int(batch), int(nsteps)
        if idx is not None and idx.numel() < batch * nsteps:
            raise DcvError(f"train_steps: {idx.numel()} indices for {nsteps} batches of {batch}")
        if idx is None and int(row0) + batch * nsteps > Xn.shape[0]:
            raise DcvError(f"train_steps: rows {row0} + {nsteps} x {batch} exceed the matrix ({Xn.shape[0]} rows)")
        check(self.lib.dcv_mlp_train_steps(self.h, *self._args(Xn, idx, row0, batch), nsteps, _stream()), "dcv_mlp_train_steps")

    def eval_steps(self, Xn, batch: int, nbatches: int, idx=None, row0=0):
        """A validation pass: `nbatches` evaluation steps of `batch` samples, batch j = idx[j * batch:(j + 1) * batch] (or rows
        row0 + j * batch ...), one loss record each in batch order -- the records `nbatches` eval_step calls would append.
        Small networks run many batches per launch (dcv_mlp_eval_steps, include/dcv.h)."""
        batch, nbatches = int(batch), int(nbatches)
        if idx is not None and idx.numel() < batch * nbatches:
            raise DcvError(f"eval_steps: {idx.numel()} indices for {nbatches} batches of {batch}")
        if idx is None and int(row0) + batch * nbatches > Xn.shape[0]:
            raise DcvError(f"eval_steps: rows {row0} + {nbatches} x {batch} exceed the matrix ({Xn.shape[0]} rows)")
        check(self.lib.dcv_mlp_eval_steps(self.h, *self._args(Xn, idx, row0, batch), nbatches, _stream()), "dcv_mlp_eval_steps")

    # -- metrics log
    def reset_log(self, capacity: int):
        check(self.lib.dcv_mlp_reset_log(self.h, int(capacity), _stream()), "dcv_mlp_reset_log")
        self._log_cap = max(self._log_cap, int(capacity))

    def read_log(self) -> np.ndarray:
        import ctypes as C

        out = np.empty((max(self._log_cap, 1), self.log_width), dtype=np.float64)
        n = C.c_int32(0)
        check(self.lib.dcv_mlp_read_log(self.h, out.ctypes.data, out.shape[0], C.byref(n), _stream()), "dcv_mlp_read_log")
        return out[: n.value].copy()

    # -- per-kernel timing (HIP events on the launch stream)
    def profile_begin(self, max_steps: int, level: int = 1):
        check(self.lib.dcv_mlp_profile_begin(self.h, int(max_steps), int(level)), "dcv_mlp_profile_begin")

    def profile_pause(self, paused: bool, skip_kinds=()):
        """Steps issued while paused carry no events (a timed region can be sampled); skip_kinds: launch kinds
        ('fwd', 'wgrad', 'dgrad') left unsampled while not paused."""
        code = 1 if paused else 0
        for k in skip_kinds:
            code |= 2 << ("fwd", "wgrad", "dgrad").index(k)
        check(self.lib.dcv_mlp_profile_pause(self.h, code), "dcv_mlp_profile_pause")

    def profile_end(self):
        """{(layer, kind): (total_ms, launches)} with kind in 'fwd' | 'wgrad' | 'dgrad'."""
        ms = np.zeros(3 * self.L, dtype=np.float64)
        cnt = np.zeros(3 * self.L, dtype=np.int32)
        check(self.lib.dcv_mlp_profile_end(self.h, ms.ctypes.data, cnt.ctypes.data), "dcv_mlp_profile_end")
        kinds = ("fwd", "wgrad", "dgrad")
        return {(c // 3, kinds[c % 3]): (float(ms[c]), int(cnt[c])) for c in range(3 * self.L) if cnt[c] > 0}

    # -- inference
    def input_sensitivity(self, Xn, gout, scale):
        """sum over the rows of Xn of |d(sum_j cv_j)/d xn_i| * scale_i  (float64 [F], device),
        chunked to the engine's row capacity.  gout [d_latent]: gradient of the summed CV with
        respect to the network output; scale [F]."""
        _require_gpu(Xn, gout, scale)
        _check_matrix(Xn)
        n, F = Xn.shape
        total = torch.zeros(F, dtype=torch.float64, device=Xn.device)
        part = torch.empty(F, dtype=torch.float64, device=Xn.device)
        cap = min(self.rows_cap, max(1, n))
        nbytes = self.lib.dcv_mlp_input_sensitivity_workspace(self.h, cap)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=Xn.device)
        gout = gout.to(torch.float32).contiguous()
        scale = scale.to(torch.float32).contiguous()
        for s in range(0, n, cap):
            e = min(n, s + cap)
            check(self.lib.dcv_mlp_input_sensitivity(self.h, _ptr(Xn[s:e]), e - s, Xn.stride(0), _ptr(gout), _ptr(scale), _ptr(part),
                                                     _ptr(ws), ws.numel(), _stream()), "dcv_mlp_input_sensitivity")
            total += part
        return total

    def infer(self, Xn, *, tmean=None, tevecs=None, pmean=None, prange=None, want_out=True, want_minmax=False):
        """Forward of every row of Xn (chunked to the engine's row capacity).
        Returns (out [n, d] or None, minmax [2, d] or None)."""
        _require_gpu(Xn, tmean, tevecs, pmean, prange)
        _check_matrix(Xn)
        n = Xn.shape[0]
        d = self.dims[self.latent_layer] // (2 if self.model == "vae" else 1)
        out = torch.empty(n, d, dtype=torch.float32, device=Xn.device) if want_out else None
        mm = None
        for s in range(0, n, self.rows_cap):
            e = min(n, s + self.rows_cap)
            chunk = Xn[s:e]
            mmc = torch.empty(2, d, dtype=torch.float32, device=Xn.device) if want_minmax else None
            check(self.lib.dcv_mlp_infer(self.h, _ptr(chunk), e - s, Xn.stride(0), _ptr(tmean), _ptr(tevecs), _ptr(pmean), _ptr(prange),
                                         _ptr(out[s:e]) if want_out else None, _ptr(mmc), _stream()), "dcv_mlp_infer")
            if want_minmax:
                if mm is None:
                    mm = mmc
                else:  # merging 2*d extrema of chunks
                    mm = torch.stack([torch.minimum(mm[0], mmc[0]), torch.maximum(mm[1], mmc[1])])
        return out, mm
