"""The refusals of the seven coordinate entries -- dcv_featurize, dcv_featurize_project, dcv_superpose, dcv_interpolate,
dcv_transform_frames, dcv_xtc_decode, dcv_xtc_encode (with dcv_xtc_pack) -- that concern strides, extents, overlap,
alignment, workspace size and NULL pointers: return code and dcv_last_error() text against
tests/golden/coord_refusals.json, recorded by tests/golden/make_golden_coord_refusals.py from the commit named in that
file.  Error texts are part of the interface; a change that only moves the validation code passes against the file as it
stands.

The validation of these entries runs before the first HIP call, so on a machine without a GPU a refused call answers with
its code and text and never touches a device pointer: the device addresses here are made up (4-, 8- or 16-byte aligned
numbers), the host arrays are real.  Each case breaks exactly one requirement of one valid base call per entry: 4 frames
of 10 atoms (compressed XTC frames, not raw ones), dense strides (30, 3, 1).  With a GPU the module skips itself: a case
that slipped through validation would launch on the made-up addresses."""
import json
import os

import numpy as np
import pytest
import torch

from deep_cartograph_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coord_refusals.json")
EINVAL, ENOMEM = -1, -3

# made-up device addresses, 256 MiB apart
XYZ, OUT, T, WS, STATUS, SLOTS, DESC, BYTES, IMAGE, W = (0x10000000 * k for k in range(1, 11))
N, A = 4, 10
BIG = 1 << 61   # a stride with which nothing fits the address space

# host arrays of the base calls
DEFS = np.array([[_lib.FEAT_DISTANCE, 0, 1, 0, 0, 0]], dtype=np.int32)
RECS = np.array([[_lib.FEAT_DISTANCE, 0, 1, 0, 0, 0, -1, 0]], dtype=np.int32)
FIT = np.array([0, 1, 2], dtype=np.int32)
FIT_REF = np.arange(9, dtype=np.float64)
TIMES = np.arange(2 * N - 1, dtype=np.float64) / 2.0
INDEX = np.arange(N, dtype=np.int64)[::-1].copy()
STEP = np.arange(N, dtype=np.int32)
TIME = np.arange(N, dtype=np.float32)


KEEP = []   # the host arrays whose addresses the base calls hold


def host(array):
    KEEP.append(array)
    return array.ctypes.data


def frame_records(stride, nbytes):
    d = np.zeros(N, dtype=_lib.XTC_FRAME_DTYPE)
    d["offset"], d["nbytes"], d["smallidx"], d["precision"] = stride * np.arange(N), nbytes, 20, 1000.0
    return host(d)


def entries(lib):
    """{entry: (argument names in order, the valid base call)}"""
    slot = int(lib.dcv_xtc_encode_slot_bytes(A))
    coords = dict(xyz=XYZ, n_frames=N, fs=3 * A, as_=3, cs=1, n_atoms=A)
    out = dict(out=OUT, ofs=3 * A, oas=3, ocs=1)
    tail = dict(ws=WS, stream=None)
    e = {}
    e["dcv_featurize"] = dict(coords, defs=DEFS.ctypes.data, n_defs=1, unit=0.1, out=OUT, ldo=1, ws_bytes=lib.dcv_featurize_workspace(N, A, 1), **tail)
    e["dcv_featurize_project"] = dict(coords, rec=RECS.ctypes.data, n_rec=1, F=1, unit=0.1, fmean=None, frange=None, W=W, d=1, bias=None,
                                      cvmean=None, cvrange=None, out=OUT, ldo=1, minmax=None,
                                      ws_bytes=lib.dcv_featurize_project_workspace(N, A, 1, 1, 1), **tail)
    e["dcv_superpose"] = dict(coords, fit=FIT.ctypes.data, fit_w=None, fit_ref=FIT_REF.ctypes.data, n_fit=3, sel=None, sel_ref=None, n_sel=0,
                              transform=T, rmsd=None, aligned=None, lda=0, moments=None, ws_bytes=lib.dcv_superpose_workspace(N, A, 3, 0), **tail)
    e["dcv_interpolate"] = dict(coords, sel=None, n_sel=0, kind=_lib.INTERP_PCHIP, extrapolate=1, t=TIMES.ctypes.data, n_out=TIMES.size,
                                noise=None, **out, ws_bytes=lib.dcv_interpolate_workspace(N, A, 0, TIMES.size), **tail)
    e["dcv_transform_frames"] = dict(coords, transform=T, ldt=16, **out, stream=None)
    e["dcv_xtc_decode"] = dict(bytes=BYTES, n_bytes=400, frames=frame_records(100, 90), n_frames=N, n_atoms=A, scale=10.0, **out,
                               status=STATUS, ws_bytes=lib.dcv_xtc_decode_workspace(N), **tail)
    e["dcv_xtc_encode"] = dict(xyz=XYZ, n_src_frames=N, fs=3 * A, as_=3, cs=1, n_atoms=A, frames=INDEX.ctypes.data, n_frames=N, inv_scale=0.1,
                               precision=1000.0, slots=SLOTS, slots_bytes=N * slot, desc=DESC, status=STATUS,
                               ws_bytes=lib.dcv_xtc_encode_workspace(N), **tail)
    e["dcv_xtc_pack"] = dict(slots=SLOTS, slots_bytes=N * slot, desc=frame_records(slot, 50),
                             image_offset=host(144 * np.arange(N, dtype=np.int64)), step=STEP.ctypes.data, time=TIME.ctypes.data, box=None,
                             n_frames=N, n_atoms=A, image=IMAGE, image_bytes=N * 144, ws_bytes=lib.dcv_xtc_pack_workspace(N), **tail)
    order = {
        "dcv_featurize": "xyz n_frames fs as_ cs n_atoms defs n_defs unit out ldo ws ws_bytes stream",
        "dcv_featurize_project": "xyz n_frames fs as_ cs n_atoms rec n_rec F unit fmean frange W d bias cvmean cvrange out ldo minmax ws ws_bytes stream",
        "dcv_superpose": "xyz n_frames fs as_ cs n_atoms fit fit_w fit_ref n_fit sel sel_ref n_sel transform rmsd aligned lda moments ws ws_bytes stream",
        "dcv_interpolate": "xyz n_frames fs as_ cs n_atoms sel n_sel kind extrapolate t n_out noise out ofs oas ocs ws ws_bytes stream",
        "dcv_transform_frames": "xyz n_frames fs as_ cs n_atoms transform ldt out ofs oas ocs stream",
        "dcv_xtc_decode": "bytes n_bytes frames n_frames n_atoms scale out ofs oas ocs status ws ws_bytes stream",
        "dcv_xtc_encode": "xyz n_src_frames fs as_ cs n_atoms frames n_frames inv_scale precision slots slots_bytes desc status ws ws_bytes stream",
        "dcv_xtc_pack": "slots slots_bytes desc image_offset step time box n_frames n_atoms image image_bytes ws ws_bytes stream",
    }
    for name, base in e.items():
        assert sorted(order[name].split()) == sorted(base) and len(order[name].split()) == len(_lib.SIGNATURES[name][1]), name
    return {name: (order[name].split(), base) for name, base in e.items()}


IN_STRIDES = [("frame stride -1", dict(fs=-1)), ("atom stride 0", dict(as_=0)), ("component stride 0", dict(cs=0))]
OUT_STRIDES = [("output frame stride 0", dict(ofs=0)), ("output atom stride 0", dict(oas=0)), ("output component stride 0", dict(ocs=0))]
WORKSPACE = [("workspace one byte short", "short"), ("workspace NULL", dict(ws=None))]

# entry -> [(what the case breaks, the arguments it changes)]: every refusal recorded in the golden file
REFUSALS = {
    "dcv_featurize": [("xyz NULL", dict(xyz=None)), ("out NULL", dict(out=None))] + IN_STRIDES + WORKSPACE,
    "dcv_featurize_project": [("xyz NULL", dict(xyz=None)), ("out NULL", dict(out=None)), ("W NULL", dict(W=None))] + IN_STRIDES + WORKSPACE,
    "dcv_superpose": [("xyz NULL", dict(xyz=None))] + IN_STRIDES + WORKSPACE,
    "dcv_interpolate": [("xyz NULL", dict(xyz=None)), ("out NULL", dict(out=None)), ("times NULL", dict(t=None))] + IN_STRIDES + OUT_STRIDES + WORKSPACE,
    "dcv_transform_frames": [("xyz NULL", dict(xyz=None)), ("transform NULL", dict(transform=None)), ("out NULL", dict(out=None))]
    + IN_STRIDES + OUT_STRIDES + [
        ("xyz off the 4-byte grid", dict(xyz=XYZ + 2)), ("out off the 4-byte grid", dict(out=OUT + 2)),
        ("transform off the 8-byte grid", dict(transform=T + 4)), ("ldt 14", dict(ldt=14)),
        ("frame stride 2^61", dict(fs=BIG)), ("output frame stride 2^61", dict(ofs=BIG)), ("atom stride INT64_MAX", dict(as_=(1 << 63) - 1)),
        ("out == xyz", dict(out=XYZ)), ("out = the last input element", dict(out=XYZ + 4 * (N * 3 * A - 1))),
        ("out ends inside xyz", dict(out=XYZ - 4 * (N * 3 * A - 1))), ("transform rows 2^61 doubles apart", dict(ldt=BIG)),
        ("transform rows overlap the output", dict(transform=OUT + 8)), ("the last transform double lies on the output's first elements", dict(transform=OUT - 8 * (3 * 16 + 15) + 8)),
    ],
    "dcv_xtc_decode": [("bytes NULL", dict(bytes=None)), ("descriptors NULL", dict(frames=None)), ("out NULL", dict(out=None)),
                       ("status NULL", dict(status=None))] + OUT_STRIDES + WORKSPACE + [
        ("bytes off the 4-byte grid", dict(bytes=BYTES + 2)), ("out off the 4-byte grid", dict(out=OUT + 2)),
        ("status off the 4-byte grid", dict(status=STATUS + 2)), ("workspace off the 8-byte grid", dict(ws=WS + 4)),
        ("frames reach behind the bytes", dict(n_bytes=390)), ("output frame stride 2^61", dict(ofs=BIG)),
        ("output inside the input bytes", dict(out=BYTES + 100)), ("status inside the output", dict(status=OUT + 8)),
        ("workspace inside the input bytes", dict(ws=BYTES + 8)), ("status inside the workspace", dict(status=WS + 4)),
    ],
    "dcv_xtc_encode": [("xyz NULL", dict(xyz=None)), ("slots NULL", dict(slots=None)), ("descriptors NULL", dict(desc=None)),
                       ("status NULL", dict(status=None)), ("frame stride 0", dict(fs=0)), ("atom stride 0", dict(as_=0)),
                       ("component stride 0", dict(cs=0))] + WORKSPACE + [
        ("slot buffer one byte short", "slots short"),
        ("xyz off the 4-byte grid", dict(xyz=XYZ + 2)), ("slots off the 4-byte grid", dict(slots=SLOTS + 2)),
        ("status off the 4-byte grid", dict(status=STATUS + 2)), ("descriptors off the 8-byte grid", dict(desc=DESC + 4)),
        ("workspace off the 8-byte grid", dict(ws=WS + 4)), ("frame stride 2^61", dict(fs=BIG)),
        ("slots overlap the coordinates", dict(slots=XYZ + 8)), ("descriptors overlap the status words", dict(desc=STATUS + 8)),
        ("workspace overlaps the coordinates", dict(ws=XYZ + 8)), ("status words overlap the slots", dict(status=SLOTS + 4)),
    ],
    "dcv_xtc_pack": [("slots NULL", dict(slots=None)), ("descriptors NULL", dict(desc=None)), ("image NULL", dict(image=None))] + WORKSPACE + [
        ("slots off the 4-byte grid", dict(slots=SLOTS + 2)), ("image off the 4-byte grid", dict(image=IMAGE + 2)),
        ("workspace off the 8-byte grid", dict(ws=WS + 4)), ("slots end before the last frame", dict(slots_bytes=100)),
        ("image ends before the last frame", dict(image_bytes=N * 144 - 4)), ("image overlaps the slots", dict(image=SLOTS + 16)),
        ("workspace overlaps the image", dict(ws=IMAGE + 8)), ("workspace overlaps the slots", dict(ws=SLOTS + 8)),
    ],
}

# the refusals this header adds to the four entries that had none: asserted directly, not part of the recorded file
NEW_EXTENT = [("dcv_featurize", dict(fs=BIG)), ("dcv_featurize_project", dict(fs=BIG)), ("dcv_superpose", dict(fs=BIG)),
              ("dcv_superpose", dict(as_=(1 << 63) - 1)), ("dcv_interpolate", dict(fs=BIG)), ("dcv_interpolate", dict(ofs=BIG)),
              ("dcv_interpolate", dict(oas=(1 << 63) - 1))]


def call(lib, table, entry, change):
    """(code, dcv_last_error() text) of the entry's base call with `change` applied"""
    names, base = table[entry]
    args = dict(base)
    if change == "short":
        args["ws_bytes"] -= 1
    elif change == "slots short":
        args["slots_bytes"] -= 1
    else:
        assert set(change) <= set(args), (entry, change)
        args.update(change)
    rc = getattr(lib, entry)(*[args[k] for k in names])
    return int(rc), lib.dcv_last_error().decode()


def compute_refusals():
    """{"entry: what is broken": {"code", "text"}} from the library at hand; only ever called without a GPU"""
    assert not torch.cuda.is_available(), "made-up device addresses: never with a GPU"
    lib = _lib.load()
    table = entries(lib)
    out = {}
    for entry, cases in REFUSALS.items():
        for what, change in cases:
            code, text = call(lib, table, entry, change)
            out[f"{entry}: {what}"] = {"code": code, "text": text}
    return out


@pytest.fixture(scope="module")
def library():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    return _lib.load()


def test_refusals_keep_code_and_text(library):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = compute_refusals()
    assert sorted(got) == sorted(golden["refusals"])
    for key, want in golden["refusals"].items():
        assert want["code"] in (EINVAL, ENOMEM) and want["text"].startswith(key.split(":")[0] + ": "), key
    differ = {k: (got[k], golden["refusals"][k]) for k in got if got[k] != golden["refusals"][k]}
    assert not differ, differ
    enomem = [k for k, v in got.items() if v["code"] == ENOMEM]
    assert len([k for k in enomem if k.endswith("workspace one byte short")]) == 7 and len(enomem) == 15, enomem


@pytest.mark.parametrize("entry,change", NEW_EXTENT, ids=[f"{e}-{'-'.join(c)}" for e, c in NEW_EXTENT])
def test_layouts_that_wrap_are_refused(library, entry, change):
    code, text = call(library, entries(library), entry, change)
    assert code == EINVAL and text.startswith(entry + ": ") and "do not fit the address space" in text, (code, text)


@pytest.mark.parametrize("entry", ["dcv_featurize", "dcv_featurize_project", "dcv_superpose", "dcv_interpolate"])
def test_without_frames_a_wrapping_layout_only_validates(library, entry):
    """the extent check sits behind the return for zero frames: such a call is DCV_OK as before"""
    code, text = call(library, entries(library), entry, dict(fs=BIG, n_out=0) if entry == "dcv_interpolate" else dict(fs=BIG, n_frames=0))
    assert code == 0, (code, text)
