"""One case per stream-taking entry of include/dcv.h, reached through its hip.py wrapper (five entries, whose wrappers
wait for the stream before they call the library, are called directly: see "entries called WITHOUT their wrapper"): the table behind
tests/test_stream_order_gpu.py (the caller-stream contract) and tests/test_stream_cases_cpu.py (no entry without a case).

Importable without a GPU: building a case makes NumPy arrays only; ``steps`` touches the device.

A case keeps its clean inputs apart: ``dev`` (name -> NumPy array that the probes upload) and ``host`` (name -> NumPy array
handed to the wrapper as it is).  ``host_arrays`` names the host arrays that reach the library UNCHANGED -- the wrappers
pass ``np.ascontiguousarray(x, dtype)``, which is ``x`` itself when dtype and layout match, so the builders make them
C-contiguous in the wrapper's dtype (tests/test_stream_cases_cpu.py checks that) and the probes may overwrite them the
moment the call returns.  ``steps(hip, dev, host)`` returns the calls as segments of steps: the probes put pending work in
front of every segment and look at the gate after every step.  A table case is one segment of one step; an ``hip.Mlp``
engine is a fixed sequence in two segments, because its first step (``set_linears``) synchronises by contract.

The shapes are the smallest parametrisation of each entry's oracle test that launches more than one workgroup (and
reaches the finishing launch where there is one); none is the workload's own.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

# why a step may hold the host: anything else must return while the work in front of it is still pending
SYNC = "synchronises the stream by contract (host outputs)"
PAGEABLE = "copies from pageable host memory"


@dataclasses.dataclass
class Step:
    name: str
    fn: Callable[[], Optional[dict]]      # runs the call on the current stream; returns the outputs to compare (or None)
    blocks: Optional[str] = None          # None: asynchronous, no host array, no host output -- must not wait for the stream


@dataclasses.dataclass
class Case:
    name: str
    entries: Tuple[str, ...]                                  # the dcv_* functions with a stream parameter the steps call
    build: Callable[[], Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]]
    steps: Callable[..., List[List[Step]]]                    # (hip, dev tensors, host arrays) -> segments of steps
    host_arrays: Tuple[str, ...] = ()
    host_dtypes: Dict[str, object] = dataclasses.field(default_factory=dict)   # the dtype the wrapper converts each host array to
    poison: Dict[str, str] = dataclasses.field(default_factory=dict)           # dev name -> "nan" | "zeros" (default by dtype)
    scribble: Dict[str, float] = dataclasses.field(default_factory=dict)       # host name -> the constant written at return (default 0)
    stateless: bool = True                                    # the caller owns every buffer: eligible for the two-stream probe as it is
    flavours: Tuple[Optional[str], ...] = (None,)             # arithmetic flavours of dcv_set_gemm_mode to run under
    tolerance: Optional[Tuple[float, float]] = None           # (rtol, atol) of the entry's oracle test, used ONLY when two
                                                              # default-stream runs differ in bits (atomics in float)
    engine: Optional[Callable] = None                         # hip -> hip.Mlp: the case owns an engine (built once, closed by the probes)


def default_poison(a: np.ndarray) -> str:
    """Poison never turns into an address: floats are NaN, integers (indices, labels, bytes) are zeros."""
    return "nan" if np.issubdtype(a.dtype, np.floating) else "zeros"


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _one(name, entries, build, call, blocks=None, **kw) -> Case:
    """A table case: one segment of one step."""
    def steps(hip, dev, host):
        return [[Step(name, lambda: call(hip, dev, host), blocks)]]
    return Case(name, tuple(entries), build, steps, **kw)


# ------------------------------------------------------------------------------------------------ statistics, filters
def _matrix(n, F, seed):
    r = _rng(seed)
    return (r.standard_normal((n, F)) * r.uniform(0.5, 3.0, F) + r.uniform(-2, 2, F)).astype(np.float32)


def _build_col_stats():
    return {"X": _matrix(3001, 130, 1)}, {}


def _build_histogram():
    X = _matrix(1000, 67, 2)
    edges = np.stack([np.histogram_bin_edges(X[:, c], bins=37) for c in range(67)]).astype(np.float32)
    return {"X": X, "edges": np.ascontiguousarray(edges)}, {}


def _build_dip():
    return {"Xs": np.ascontiguousarray(np.sort(_matrix(164, 100, 3), axis=0))}, {}


def _build_normalize():
    X = _matrix(1000, 100, 4)
    return {"X": X, "mean": X.mean(0).astype(np.float32), "range": (X.max(0) - X.min(0)).astype(np.float32)}, {}


def _build_cov(shift):
    def build():
        X = _matrix(2053 + 3, 130, 5)
        dev = {"X": X}
        if shift:
            dev["shift"] = X.mean(0).astype(np.float32)
        return dev, {}
    return build


def _build_project():
    r = _rng(6)
    F, d = 100, 8
    dev = {"X": _matrix(777, F, 6), "W": r.standard_normal((F, d)).astype(np.float32), "fmean": r.standard_normal(F).astype(np.float32),
           "frange": r.uniform(0.5, 2.0, F).astype(np.float32), "bias": r.standard_normal(d).astype(np.float32),
           "cvmean": r.standard_normal(d).astype(np.float32), "cvrange": r.uniform(0.5, 3.0, d).astype(np.float32)}
    return dev, {}


def _call_project(hip, dev, host):
    out, mm = hip.project_linear(dev["X"], dev["W"], fmean=dev["fmean"], frange=dev["frange"], bias=dev["bias"], cvmean=dev["cvmean"],
                                 cvrange=dev["cvrange"], want_out=True, want_minmax=True)
    return {"out": out, "minmax": mm}


# ------------------------------------------------------------------------------------------------ products
GEMM_QUARTER = (96, 160, 300)          # tests/test_gemm_tiles_gpu.py random_case("quarter"): six 64 x 64 tiles
TN_SPLIT_QUARTER = (96, 160, 512, 4096 - 5)   # its tn_split_case("quarter"): M, N, k_chunk, K -- eight slabs, the last ragged


def _build_gemm(mode):
    def build():
        M, N, K = GEMM_QUARTER
        r = _rng(7)
        A, B = r.standard_normal((M, K)).astype(np.float32), r.standard_normal((K, N)).astype(np.float32)
        if mode == "nt":
            return {"A": A, "B": np.ascontiguousarray(B.T)}, {}
        if mode == "nn":
            return {"A": A, "B": B}, {}
        return {"A": np.ascontiguousarray(A.T), "B": B}, {}
    return build


def _build_tn_split():
    M, N, _, K = TN_SPLIT_QUARTER
    r = _rng(8)
    return {"A": r.standard_normal((K, M)).astype(np.float32), "B": r.standard_normal((K, N)).astype(np.float32)}, {}


def _call_tn_split(hip, dev, host):
    _, _, kc, K = TN_SPLIT_QUARTER
    return {"slabs": hip.gemm_tn_split(dev["A"], dev["B"], kc, -(-K // kc))}


# ------------------------------------------------------------------------------------------------ coordinates
def _coordinates(n, A, seed):
    return (_rng(seed).standard_normal((n, A, 3)) * 12).astype(np.float32)


def _build_featurize():
    n, A, n_defs = 65, 37, 50
    r = _rng(9)
    defs, col = [], 0
    for i in range(n_defs):
        kind = (0, 1, 2)[i % 3]
        atoms = r.choice(A, size=4, replace=False).tolist()
        defs.append([kind, *atoms, col])
        col += 2 if kind == 1 else 1
    return {"xyz": _coordinates(n, A, 9)}, {"defs": np.ascontiguousarray(np.asarray(defs, dtype=np.int32))}


def _build_featurize_project():
    from tests.test_featurize_project_gpu import A, N, model, random_coordinates, random_records

    rec, F = random_records(A, 65, 165)
    W, v = model(F, 5, 655)
    dev = {"xyz": random_coordinates(N, A, 7), "W": W}
    dev.update(v)
    return dev, {"records": np.ascontiguousarray(rec, dtype=np.int32), "F": np.asarray(F)}


def _call_featurize_project(hip, dev, host):
    vec = {k: dev[k] for k in ("fmean", "frange", "bias", "cvmean", "cvrange")}
    out, mm = hip.featurize_project(dev["xyz"], host["records"], dev["xyz"].shape[1], int(host["F"]), dev["W"], want_minmax=True, **vec)
    return {"out": out, "minmax": mm}


def _build_superpose():
    n, A, n_fit, n_sel = 33, 40, 17, 11
    r = _rng(10)
    base = r.standard_normal((A, 3)) * 8
    xyz = (base[None] + r.standard_normal((n, A, 3)) * 0.7 + r.standard_normal((n, 1, 3)) * 5).astype(np.float32)
    fit = np.ascontiguousarray(np.sort(r.choice(A, n_fit, replace=False)).astype(np.int32))
    sel = np.ascontiguousarray(r.choice(A, n_sel, replace=False).astype(np.int32))
    host = {"fit": fit, "fit_ref": np.ascontiguousarray(base[fit]), "fit_weights": r.uniform(0.5, 2.0, n_fit),
            "sel": sel, "sel_ref": np.ascontiguousarray(base[sel])}
    return {"xyz": xyz}, host


def _call_superpose(hip, dev, host):
    return hip.superpose(dev["xyz"], dev["xyz"].shape[1], host["fit"], host["fit_ref"], sel=host["sel"], sel_ref=host["sel_ref"],
                         fit_weights=host["fit_weights"], want=hip.SUPERPOSE_OUTPUTS)


def _build_interpolate():
    from tests.augmentation_oracle import crafted

    n, A = 40, 100
    t = np.sort(np.concatenate([np.linspace(-0.5, n - 0.5, n), [0.0, 7.0, n - 1.0]]))   # tests/test_augmentation_gpu.py _times(40, 1)
    sel = np.ascontiguousarray(_rng(11).permutation(A)[:50].astype(np.int32))
    return {"xyz": crafted(n, A, 11, special_atoms=(int(sel[0]), int(sel[1]))).astype(np.float32)}, {"t": np.ascontiguousarray(t), "sel": sel}


LONG_T = 1_500_000   # 12 MB of query times: a pageable source far above anything a runtime would stage in one piece


def _build_interpolate_long():
    from tests.augmentation_oracle import crafted

    n, A = 40, 4
    return ({"xyz": crafted(n, A, 21).astype(np.float32)},
            {"t": np.ascontiguousarray(np.linspace(-0.5, n - 0.5, LONG_T)), "sel": np.ascontiguousarray(np.array([2], dtype=np.int32))})


def _build_transform():
    n, A = 9, 257
    r = _rng(12)
    T = np.zeros((n, 16))
    for f in range(n):
        q, _ = np.linalg.qr(r.standard_normal((3, 3)))
        T[f, :9] = (q * np.sign(np.linalg.det(q))).reshape(-1)
        T[f, 9:15] = r.standard_normal(6) * 10
    return {"xyz": _coordinates(n, A, 12), "transform": T}, {}


def _build_xtc_decode():
    from deep_cartograph_amd import _lib
    from tests import xtc_oracle as xo
    from tests.conftest import load_golden

    data = load_golden("xtc_golden.npz")["aladip_xtc"].tobytes()
    frames = xo.frames(data)
    desc = np.zeros(len(frames), dtype=_lib.XTC_FRAME_DTYPE)
    for i, f in enumerate(frames):
        desc[i] = (f["offset"], f["nbytes"], f["smallidx"], f["precision"], 0, f["minint"], f["maxint"])
    return {"bytes": np.frombuffer(data, dtype=np.uint8).copy()}, {"frames": desc, "n_atoms": np.asarray(frames[0]["natoms"])}


def _call_xtc_decode(hip, dev, host):
    out, status = hip.xtc_decode(dev["bytes"], host["frames"], int(host["n_atoms"]), return_status=True)
    return {"xyz": out, "status": status}


def _build_xtc_encode():
    from tests import xtc_encode_oracle as eo

    xyz = eo.synthetic("chain", 64, 17)
    frames = np.ascontiguousarray(_rng(13).integers(0, 64, 64).astype(np.int64))   # any order, repeats allowed
    return {"xyz": np.ascontiguousarray(xyz)}, {"frames": frames}


# ---- entries called WITHOUT their wrapper.  hip.dip_sorted, hip.linkage, hip.core_distances and hip.mr_mst read the input
# back to refuse non-finite values before they call the library, and hip.xtc_encode downloads the descriptors between
# dcv_xtc_encode and dcv_xtc_pack: through the wrapper the side stream has drained when the C entry runs, and the probes
# could not fail.  These cases marshal the arguments as the wrappers do and call _lib.load() themselves, so that the
# pending work stands in front of the entry and the host arrays are overwritten at ITS return.
def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _direct(name, rc):
    from deep_cartograph_amd._lib import check

    check(rc, name)


def _call_dip_direct(hip, dev, host):
    import torch
    from deep_cartograph_amd import _lib

    lib, Xs = _lib.load(), dev["Xs"]
    n, C = Xs.shape
    dip = torch.empty(C, dtype=torch.float64, device=Xs.device)
    lo, hi = torch.empty(C, dtype=torch.int32, device=Xs.device), torch.empty(C, dtype=torch.int32, device=Xs.device)
    ws = hip._ws(lib.dcv_dip_sorted_workspace(n, C), Xs.device)
    _direct("dcv_dip_sorted", lib.dcv_dip_sorted(Xs.data_ptr(), n, C, Xs.stride(0), dip.data_ptr(), lo.data_ptr(), hi.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), _stream()))
    return {"dip": dip, "lo": lo, "hi": hi}


def _call_xtc_encode_direct(hip, dev, host):
    """dcv_xtc_encode as hip.xtc_encode_slots calls it; the slots start as zeros (the entry writes the payloads only)."""
    import torch
    from deep_cartograph_amd import _lib

    lib, xyz, frames = _lib.load(), dev["xyz"], host["frames"]
    n_src, A = xyz.shape[:2]
    n = int(frames.size)
    slot = int(lib.dcv_xtc_encode_slot_bytes(A))
    slots = torch.zeros(n * slot, dtype=torch.uint8, device=xyz.device)
    desc = torch.zeros(n * _lib.XTC_FRAME_DTYPE.itemsize, dtype=torch.uint8, device=xyz.device)
    status = torch.empty(n, dtype=torch.int32, device=xyz.device)
    ws = hip._ws(lib.dcv_xtc_encode_workspace(n), xyz.device)
    fs, as_, cs = (int(v) for v in xyz.stride())
    _direct("dcv_xtc_encode", lib.dcv_xtc_encode(xyz.data_ptr(), n_src, fs, as_, cs, A, frames.ctypes.data, n, 0.1, 1000.0, slots.data_ptr(),
                                                 slots.numel(), desc.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return {"slots": slots, "desc": desc, "status": status}


def _build_xtc_pack():
    """The slots and descriptors dcv_xtc_encode would leave, from the oracle: dcv_xtc_pack then has device input of its own to
    poison and pending work in front of it."""
    from tests import xtc_encode_oracle as eo

    A, n = 17, 64
    xyz = eo.synthetic("chain", n, A)
    bodies, desc, status = eo.encode(xyz)
    assert not status.any()
    slot = eo.slot_bytes(A)
    slots = np.zeros(n * slot, dtype=np.uint8)
    for f, body in enumerate(bodies):
        pay = np.frombuffer(eo.slot_payload(body, A), dtype=np.uint8)
        slots[f * slot: f * slot + pay.size] = pay
    size = 92 + (desc["nbytes"].astype(np.int64) + 3) // 4 * 4
    host = {"desc": np.ascontiguousarray(desc), "offsets": np.ascontiguousarray(np.cumsum(size) - size, dtype=np.int64),
            "step": np.arange(n, dtype=np.int32) * 500, "time": np.arange(n, dtype=np.float32) * 2, "image_bytes": np.asarray(int(size.sum()))}
    return {"slots": slots}, host


def _call_xtc_pack(hip, dev, host):
    return {"image": hip.xtc_pack(dev["slots"], host["desc"], host["offsets"], 17, host["step"], host["time"], image_bytes=int(host["image_bytes"]))}


def _call_linkage_direct(hip, dev, host):
    import ctypes as C
    from deep_cartograph_amd import _lib

    lib, P = _lib.load(), dev["P"]
    n, d = P.shape
    Z = np.empty((n - 1, 4), dtype=np.float64)
    searches = C.c_int64(0)
    nbytes = lib.dcv_linkage_workspace(n, d)
    ws = hip._ws(nbytes, P.device)
    _direct("dcv_linkage", lib.dcv_linkage(P.data_ptr(), n, d, hip.LINKAGE_METHOD["average"], Z.ctypes.data, C.byref(searches), ws.data_ptr(), nbytes,
                                           _stream()))
    return {"Z": Z, "searches": np.asarray(searches.value)}


def _call_core_direct(hip, dev, host):
    import torch
    from deep_cartograph_amd import _lib

    lib, P = _lib.load(), dev["P"]
    n, d = P.shape
    core = torch.empty(n, dtype=torch.float64, device=P.device)
    nbytes = lib.dcv_core_distances_workspace(n, d, 3)
    ws = hip._ws(nbytes, P.device)
    _direct("dcv_core_distances", lib.dcv_core_distances(P.data_ptr(), n, d, 3, core.data_ptr(), ws.data_ptr(), nbytes, _stream()))
    return {"core": core}


def _build_mst():
    """Core distances (k = 3, the point itself included) from NumPy: dcv_mr_mst gets both inputs from the caller, so that it
    is a case of its own with pending work in front of it."""
    P = _build_points513()[0]["P"]
    dist = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    return {"P": P, "core": np.ascontiguousarray(np.sort(dist, axis=1)[:, 2])}, {}


def _call_mst_direct(hip, dev, host):
    from deep_cartograph_amd import _lib

    lib, P, core = _lib.load(), dev["P"], dev["core"]
    n, d = P.shape
    src, dst, w = np.empty(n - 1, dtype=np.int64), np.empty(n - 1, dtype=np.int64), np.empty(n - 1, dtype=np.float64)
    nbytes = lib.dcv_mr_mst_workspace(n, d)
    ws = hip._ws(nbytes, P.device)
    _direct("dcv_mr_mst", lib.dcv_mr_mst(P.data_ptr(), n, d, core.data_ptr(), src.ctypes.data, dst.ctypes.data, w.ctypes.data, ws.data_ptr(), nbytes,
                                         _stream()))
    return {"src": src, "dst": dst, "w": w}


# ------------------------------------------------------------------------------------------------ points
def _lloyd(d, k, n, seed):
    r = _rng(seed)
    cent = r.uniform(-1, 1, (k, d))
    P = np.round(cent[r.integers(0, k, n)] + 0.15 * r.standard_normal((n, d)), 4)
    C = P[r.choice(n, k, replace=False)] + 1e-3
    mean = P.mean(0)
    return {"P": P, "centers": C - mean, "offset": mean, "labels": np.full(n, -1, dtype=np.int32)}, {}


def _call_kmeans(mindist):
    def call(hip, dev, host):
        acc, md = hip.kmeans_step(dev["P"], dev["centers"], dev["labels"], offset=dev["offset"], want_mindist=mindist)
        out = {"acc": acc, "labels": dev["labels"]}
        if mindist:
            out["mindist"] = md
        return out
    return call


def _build_kmeanspp():
    n, d = 1537, 5
    r = _rng(3005)
    P = np.round(r.uniform(-1, 1, (n, d)), 4)
    mean = P.mean(0)
    return {"P": P, "offset": mean, "c0": r.uniform(-1, 1, d) - mean, "c1": r.uniform(-1, 1, d) - mean,
            "cand": r.uniform(-1, 1, (3, d)) - mean, "closest": np.full(n, -1.0)}, {}


def _steps_kmeanspp(hip, dev, host):
    def first():
        return {"pot0": hip.kmeanspp_update(dev["P"], dev["c0"], dev["closest"], True, offset=dev["offset"])}

    def potentials():
        return {"pots": hip.kmeanspp_potentials(dev["P"], dev["cand"], dev["closest"], offset=dev["offset"])}

    def second():
        return {"pot1": hip.kmeanspp_update(dev["P"], dev["c1"], dev["closest"], False, offset=dev["offset"]), "closest": dev["closest"]}
    return [[Step("update first", first), Step("potentials", potentials), Step("update second", second)]]


def _build_label_stats():
    from tests.scores_oracle import mixture

    P, labels = mixture(1025, 1025, 3, 5)
    centers = np.stack([P[labels == c].mean(0) for c in range(5)])
    return {"P": np.ascontiguousarray(P), "labels": np.ascontiguousarray(labels.astype(np.int32)), "centers": centers}, {}


def _build_dist_sums():
    from tests.scores_oracle import DIST_SUM_CASES, dist_sum_case

    Q, P_sorted, start = dist_sum_case(*DIST_SUM_CASES[0])
    return {"Q": np.ascontiguousarray(Q), "P_sorted": np.ascontiguousarray(P_sorted), "start": np.ascontiguousarray(start, dtype=np.int64)}, {}


def _build_silhouette():
    r = _rng(14)
    sizes = np.array([5, 1, 300, 0, 207])
    nq, k = int(sizes.sum()), len(sizes)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return {"S": r.uniform(0.1, 50.0, (nq, k)), "qlabels": np.repeat(np.arange(k), sizes).astype(np.int32), "start": start}, {}


def _build_binning():
    r = _rng(15)
    return {"P": r.standard_normal((3001, 3))}, {}


def _call_binning(hip, dev, host):
    grid, outside = hip.linear_binning(dev["P"], (2, 0), (-1.5, -2.0), (1.0, 2.5), 37)
    return {"grid": grid, "outside": np.asarray(outside)}


def _build_nearest_rows():
    r = _rng(113)
    P = np.round(r.uniform(-1, 1, (150_001, 1)), 4)
    P[70_000:70_050] = P[10_000:10_050]
    C = np.round(r.uniform(-1, 1, (3, 1)), 3)
    C[0] = P[70_010]
    return {"P": P, "centers": C}, {}


def _call_nearest_rows(hip, dev, host):
    dist, rows = hip.nearest_rows(dev["P"], dev["centers"])
    return {"dist": dist, "rows": rows}


def _build_nearest_point():
    r = _rng(16)
    return {"train": np.round(r.standard_normal((255, 2)), 4), "sup": np.round(r.standard_normal((257, 2)), 4)}, {}


def _build_points513():
    return {"P": np.round(_rng(17).standard_normal((513, 3)), 4)}, {}


def _table() -> List[Case]:
    t = [
        _one("col_stats_raw", ["dcv_col_stats"], _build_col_stats, lambda hip, dev, host: {"raw": hip.col_stats_raw(dev["X"])}),
        _one("col_histogram", ["dcv_col_histogram"], _build_histogram, lambda hip, dev, host: {"counts": hip.col_histogram(dev["X"], dev["edges"])}),
        # sorted finite columns are the entry's precondition: the poison is a constant (sorted, dip 0).  Called directly: no
        # host array, no host output, so it must return with the gate closed
        _one("dip_sorted", ["dcv_dip_sorted"], _build_dip, _call_dip_direct, poison={"Xs": "zeros"}),
        _one("normalize", ["dcv_normalize"], _build_normalize, lambda hip, dev, host: {"out": hip.normalize(dev["X"], dev["mean"], dev["range"])}),
        _one("lagged_cov_raw", ["dcv_lagged_cov"], _build_cov(False), lambda hip, dev, host: {"raw": hip.lagged_cov_raw(dev["X"], 2053, 3)},
             flavours=("split", "native")),
        _one("lagged_cov_raw shift", ["dcv_lagged_cov"], _build_cov(True),
             lambda hip, dev, host: {"raw": hip.lagged_cov_raw(dev["X"], 2053, 3, shift=dev["shift"])}, flavours=("split", "native")),
        _one("project_linear", ["dcv_project_linear"], _build_project, _call_project),
    ]
    for mode in ("nt", "nn", "tn"):
        t.append(_one(f"gemm {mode}", ["dcv_gemm_f32"], _build_gemm(mode), lambda hip, dev, host, mode=mode: {"C": hip.gemm(mode, dev["A"], dev["B"])},
                      flavours=("split", "native")))
    t += [
        _one("gemm_tn_split", ["dcv_gemm_tn_split"], _build_tn_split, _call_tn_split, flavours=("split", "native")),
        _one("featurize", ["dcv_featurize"], _build_featurize, lambda hip, dev, host: {"out": hip.featurize(dev["xyz"], host["defs"], 37)},
             blocks=PAGEABLE, host_arrays=("defs",), host_dtypes={"defs": np.int32}),
        _one("featurize_project", ["dcv_featurize_project"], _build_featurize_project, _call_featurize_project, blocks=PAGEABLE,
             host_arrays=("records",), host_dtypes={"records": np.int32}),
        _one("superpose", ["dcv_superpose"], _build_superpose, _call_superpose, blocks=PAGEABLE,
             host_arrays=("fit", "fit_ref", "fit_weights", "sel", "sel_ref"),
             host_dtypes={"fit": np.int32, "fit_ref": np.float64, "fit_weights": np.float64, "sel": np.int32, "sel_ref": np.float64},
             scribble={"fit_weights": 1.0}),
    ]
    for kind in ("pchip", "makima"):
        t.append(_one(f"interpolate {kind}", ["dcv_interpolate"], _build_interpolate,
                      lambda hip, dev, host, kind=kind: {"out": hip.interpolate(dev["xyz"], 100, host["t"], kind=kind, sel=host["sel"])},
                      blocks=PAGEABLE, host_arrays=("t", "sel"), host_dtypes={"t": np.float64, "sel": np.int32}, scribble={"t": 3.0}))
    # beyond the table of small host arrays: the one caller-owned array that grows with the output.  Whether the runtime
    # has taken its copy of a LARGE pageable source when hipMemcpyAsync returns is what the released-inputs probe measures here
    t.append(_one("interpolate long t", ["dcv_interpolate"], _build_interpolate_long,
                  lambda hip, dev, host: {"out": hip.interpolate(dev["xyz"], 4, host["t"], kind="pchip", sel=host["sel"])},
                  blocks=PAGEABLE, host_arrays=("t", "sel"), host_dtypes={"t": np.float64, "sel": np.int32}, scribble={"t": 3.0}))
    t += [
        _one("transform_frames", ["dcv_transform_frames"], _build_transform,
             lambda hip, dev, host: {"out": hip.transform_frames(dev["xyz"], 257, dev["transform"])}),
        _one("xtc_decode", ["dcv_xtc_decode"], _build_xtc_decode, _call_xtc_decode, blocks=PAGEABLE, host_arrays=("frames",),
             host_dtypes={"frames": "XTC_FRAME_DTYPE"}),
        _one("xtc_encode", ["dcv_xtc_encode"], _build_xtc_encode, _call_xtc_encode_direct, blocks=PAGEABLE, host_arrays=("frames",),
             host_dtypes={"frames": np.int64}),
        _one("xtc_pack", ["dcv_xtc_pack"], _build_xtc_pack, _call_xtc_pack, blocks=SYNC, host_arrays=("desc", "offsets", "step", "time"),
             host_dtypes={"desc": "XTC_FRAME_DTYPE", "offsets": np.int64, "step": np.int32, "time": np.float32}),
        # sums in float64 may combine through atomics: the tolerance is test_kmeans_pass_through_the_lds_ring's
        _one("kmeans_step ring", ["dcv_kmeans_step"], lambda: _lloyd(4, 6, 70_001, 1046), _call_kmeans(False), tolerance=(1e-12, 1e-9)),
        _one("kmeans_step general", ["dcv_kmeans_step"], lambda: _lloyd(5, 3, 1000, 2053), _call_kmeans(True), tolerance=(1e-12, 1e-9)),
        Case("kmeanspp", ("dcv_kmeanspp_update", "dcv_kmeanspp_potentials"), _build_kmeanspp, _steps_kmeanspp, tolerance=(1e-12, 1e-15)),
        _one("label_stats", ["dcv_label_stats"], _build_label_stats,
             lambda hip, dev, host: {"acc": hip.label_stats(dev["P"], dev["labels"], 5, centers=dev["centers"])}, tolerance=(1e-12, 1e-9)),
        _one("cluster_dist_sums", ["dcv_cluster_dist_sums"], _build_dist_sums,
             lambda hip, dev, host: {"S": hip.cluster_dist_sums(dev["Q"], dev["P_sorted"], dev["start"])}),
        _one("silhouette_sum", ["dcv_silhouette_sum"], _build_silhouette,
             lambda hip, dev, host: {"sum": hip.silhouette_sum(dev["S"], dev["qlabels"], dev["start"])}),
        _one("linear_binning", ["dcv_linear_binning"], _build_binning, _call_binning, blocks=SYNC),
        _one("nearest_rows", ["dcv_nearest_rows"], _build_nearest_rows, _call_nearest_rows),
        _one("nearest_point", ["dcv_nearest_point"], _build_nearest_point,
             lambda hip, dev, host: {"nn": hip.nearest_point(dev["train"], dev["sup"])}),
        # finite points are the precondition of both families: the poison is zeros.  Called directly (see above)
        _one("linkage", ["dcv_linkage"], _build_points513, _call_linkage_direct, blocks=SYNC, poison={"P": "zeros"}),
        _one("core_distances", ["dcv_core_distances"], _build_points513, _call_core_direct, blocks=SYNC, poison={"P": "zeros"}),
        _one("mr_mst", ["dcv_mr_mst"], _build_mst, _call_mst_direct, blocks=SYNC, poison={"P": "zeros", "core": "zeros"}),
    ]
    return t


# ------------------------------------------------------------------------------------------------ hip.Mlp engines
@dataclasses.dataclass
class EngineSpec:
    name: str
    model: str
    dims: Tuple[int, ...]
    acts: Tuple[Optional[str], ...]
    batch: int
    latent: Optional[int] = None
    dropout: Optional[Tuple[float, ...]] = None
    flavours: Tuple[Optional[str], ...] = (None,)
    lag: int = 3
    path: int = 0                # dcv_mlp_last_path the training steps must take: 0 layer by layer, 1 fused AE / VAE, 2 fused Deep-TICA
    batchnorm: Optional[Tuple[bool, ...]] = None


_T3 = ("tanh", "tanh", None)
ENGINES = [
    EngineSpec("deep_tica block", "deep_tica", (256, 512, 128, 3), _T3, 1000, flavours=("split", "native")),
    # the fused launches have one arithmetic; infer and input_sensitivity of the same engine are block-engine products and have two
    EngineSpec("deep_tica fused", "deep_tica", (54, 16, 8, 2), _T3, 128, flavours=("split", "native"), path=2),
    EngineSpec("ae block", "ae", (256, 512, 128, 3, 128, 512, 256), _T3 * 2, 1000, latent=3, flavours=("split", "native"), lag=0),
    EngineSpec("ae fused", "ae", (54, 16, 8, 2, 8, 16, 54), _T3 * 2, 128, latent=3, flavours=("split", "native"), lag=0, path=1),
    # the reference-sized VAE; dropout keeps it off the fused launch (snet.hip refuses dropout), so it steps layer by layer on
    # the block engine in both flavours -- which is also why latent_sample can be read
    EngineSpec("vae dropout", "vae", (54, 16, 8, 4, 4, 8, 54), ("leaky_relu", "leaky_relu", None, "leaky_relu", "leaky_relu", None), 128,
               latent=3, dropout=(0.25, 0, 0, 0, 0, 0), flavours=("split", "native"), lag=0),
    # the same network without dropout takes the fused launch: the KL partials and the eps cursor inside snet.hip
    EngineSpec("vae fused", "vae", (54, 16, 8, 4, 4, 8, 54), ("leaky_relu", "leaky_relu", None, "leaky_relu", "leaky_relu", None), 128,
               latent=3, flavours=("split", "native"), lag=0, path=1),
    # a batch normalisation behind the first Linear (which also keeps the network off the fused launch): dcv_mlp_bn_state, both ways
    EngineSpec("deep_tica batchnorm", "deep_tica", (54, 16, 8, 2), _T3, 128, flavours=("split", "native"), batchnorm=(True, False, False)),
]
MLP_ENTRIES = ("dcv_mlp_set_params", "dcv_mlp_reset_log", "dcv_mlp_train_step", "dcv_mlp_eval_step", "dcv_mlp_train_steps", "dcv_mlp_eval_steps",
               "dcv_mlp_infer", "dcv_mlp_input_sensitivity", "dcv_mlp_read_log", "dcv_mlp_get_params", "dcv_mlp_forward", "dcv_mlp_backward",
               "dcv_mlp_apply")
MLP_ENTRIES_AE = ("dcv_mlp_set_feature_range",)
MLP_ENTRIES_VAE = ("dcv_mlp_latent_sample",)
MLP_ENTRIES_DROPOUT = ("dcv_mlp_dropout_mask",)
MLP_ENTRIES_BLOCK = ("dcv_mlp_layer_output",)
MLP_ENTRIES_BN = ("dcv_mlp_bn_state",)


def _engine_case(spec: EngineSpec) -> Case:
    L = len(spec.dims) - 1
    vae = spec.model == "vae"
    latent = spec.latent if spec.latent is not None else L
    d = spec.dims[latent] // (2 if vae else 1)
    F, B = spec.dims[0], spec.batch
    n = 2 * B + 64

    def build():
        r = _rng(100 + sum(spec.dims) + B)
        dev = {"X": r.standard_normal((n, F)).astype(np.float32), "idx": r.permutation(n - spec.lag)[:B].astype(np.int64),
               "idx2": r.permutation(n - spec.lag)[:2 * B].astype(np.int64), "gout": r.standard_normal(spec.dims[latent]).astype(np.float32),
               "scale": r.uniform(0.5, 2.0, F).astype(np.float32), "pmean": r.standard_normal(d).astype(np.float32),
               "prange": r.uniform(0.5, 2.0, d).astype(np.float32)}
        if vae:
            dev["gout"][d:] = 0
            dev["eps"] = r.standard_normal((12 * B, d)).astype(np.float32)
        if spec.model == "deep_tica":
            dev["tmean"], dev["tevecs"] = r.standard_normal(d).astype(np.float32), r.standard_normal((d, d)).astype(np.float32)
        host = {}
        for l in range(L):
            fan_in = spec.dims[l] // 2 if vae and l == latent else spec.dims[l]
            bound = 1.0 / np.sqrt(fan_in)
            host[f"w{l}"] = r.uniform(-bound, bound, (spec.dims[l + 1], fan_in)).astype(np.float32)
            host[f"b{l}"] = r.uniform(-bound, bound, spec.dims[l + 1]).astype(np.float32)
        if spec.model != "deep_tica":
            host["range"] = np.ascontiguousarray(r.uniform(0.5, 2.0, F).astype(np.float32))
        if spec.batchnorm:
            host["bn_mean"] = np.ascontiguousarray((0.1 * r.standard_normal(spec.dims[1])).astype(np.float32))
            host["bn_var"] = np.ascontiguousarray(r.uniform(0.5, 1.5, spec.dims[1]).astype(np.float32))
        return dev, host

    def engine(hip):
        kw = dict(max_batch=B, lr=1e-3)
        if spec.model == "deep_tica":
            kw.update(lag=spec.lag, tica_reg=1e-6)
        else:
            kw.update(latent_layer=latent)
        if spec.dropout is not None:
            kw.update(dropout=list(spec.dropout), seed=5)
        if spec.batchnorm:
            kw.update(batchnorm=list(spec.batchnorm))
        return hip.Mlp(spec.model, list(spec.dims), list(spec.acts), **kw)

    def steps(hip, dev, host, eng):
        X = dev["X"]
        setup, run = [], []
        if "range" in host:
            setup.append(Step("set_feature_range", lambda: eng.set_feature_range(host["range"]), SYNC))
        def set_linears():   # with a normalisation also dcv_mlp_bn_state(set = 1): the running statistics go up from the caller's arrays
            bn = [{"running_mean": host["bn_mean"], "running_var": host["bn_var"], "num_batches_tracked": 3}] + [None] * (L - 1) if spec.batchnorm else None
            eng.set_linears([(host[f"w{l}"], host[f"b{l}"]) for l in range(L)], bn=bn)
        setup.append(Step("set_linears", set_linears, SYNC))
        if vae:
            def noise():
                eng.set_kl_beta(0.1)
                eng.set_noise(dev["eps"])
            run.append(Step("set_noise", noise))
        def first_step():
            eng.train_step(X, row0=0, batch=B)
            # a fallback would compute the same numbers on other kernels and every comparison would still pass
            assert eng.last_path() == spec.path, f"{spec.name}: the training step took path {eng.last_path()}, the case is about path {spec.path}"
        run += [Step("reset_log", lambda: eng.reset_log(16)),
                Step("train_step", first_step),
                Step("train_step idx", lambda: eng.train_step(X, idx=dev["idx"])),
                Step("train_step row0", lambda: eng.train_step(X, row0=7, batch=B))]

        def phases():   # one more training step, phase by phase
            eng.forward(X, row0=11, batch=B)
            out = {"layer0": eng.layer_output(0, B)} if eng.last_path() == 0 else None
            eng.backward(X, row0=11, batch=B)
            eng.apply()
            return out
        run.append(Step("forward backward apply", phases))
        if vae and spec.path == 0:   # z never leaves LDS on the fused launch
            run.append(Step("latent_sample", lambda: {"z": eng.latent_sample(B)}))
        run += [Step("eval_step", lambda: eng.eval_step(X, row0=3, batch=B)),
                Step("train_steps", lambda: eng.train_steps(X, B, 2, idx=dev["idx2"])),
                Step("eval_steps", lambda: eng.eval_steps(X, B, 2, row0=5))]

        def infer():
            extra = {"tmean": dev["tmean"], "tevecs": dev["tevecs"]} if spec.model == "deep_tica" else {}
            out, mm = eng.infer(X, pmean=dev["pmean"], prange=dev["prange"], want_minmax=True, **extra)
            return {"cv": out, "minmax": mm}
        run += [Step("infer", infer),
                Step("input_sensitivity", lambda: {"sens": eng.input_sensitivity(X, dev["gout"], dev["scale"])})]
        if spec.dropout is not None:
            run.append(Step("dropout_mask", lambda: {"mask": eng.dropout_mask(0, 1, B)}))
        def linears():
            out = {}
            for l, (w, b) in enumerate(eng.get_linears()):
                out[f"weight{l}"], out[f"bias{l}"] = w, b
            return out
        run += [Step("read_log", lambda: {"log": eng.read_log(), "path": np.asarray(eng.last_path())}, SYNC),
                Step("get_linears", linears, SYNC)]
        if spec.batchnorm:
            def get_bn():
                st = eng.get_bn()[0]
                return {k: np.asarray(st[k]) for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
            run.append(Step("get_bn", get_bn, SYNC))
        return [setup, run]

    entries = MLP_ENTRIES + (MLP_ENTRIES_AE if spec.model != "deep_tica" else ()) + (MLP_ENTRIES_VAE if vae else ()) + \
        (MLP_ENTRIES_DROPOUT if spec.dropout is not None else ()) + (MLP_ENTRIES_BLOCK if spec.path == 0 else ()) + \
        (MLP_ENTRIES_BN if spec.batchnorm else ())
    listed = (("range",) if spec.model != "deep_tica" else ()) + (("bn_mean", "bn_var") if spec.batchnorm else ())
    return Case("mlp " + spec.name, entries, build, steps, host_arrays=listed, host_dtypes={k: np.float32 for k in listed},
                scribble={"range": 1.0, "bn_var": 1.0}, stateless=False,
                flavours=spec.flavours, engine=engine,
                # log records and parameters against float64: the tolerances of tests/test_vae_gpu.py (rtol 1e-4) -- used only if
                # two default-stream runs of the engine differ in bits
                tolerance=(1e-4, 1e-6))


CASES: List[Case] = _table() + [_engine_case(s) for s in ENGINES]

# Stream-taking entries of include/dcv.h without a case, each with its reason (tests/test_stream_cases_cpu.py keeps it short)
EXCLUDED = {
    "dcv_mlp_dp_step": "data-parallel step: its collectives are callbacks of the caller, exercised by the two-rank tests",
    "dcv_comm_bind_stream": "dcv_comm_*: an RCCL communicator needs more than one device to mean anything",
    "dcv_comm_allreduce": "dcv_comm_*: an RCCL communicator needs more than one device to mean anything",
    "dcv_linkage_pdist": "benchmark hook: the first stage of dcv_linkage, which the linkage case runs on the same stream argument",
}


def covered_entries() -> set:
    return {e for c in CASES for e in c.entries}
