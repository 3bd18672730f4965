"""No stream-taking entry of include/dcv.h without a case in tests/stream_cases.py: the header is parsed, every ``dcv_*``
function with a ``stream`` parameter must be named by a case or by the short exclusion list (each with its reason), so a
new entry cannot arrive untested by tests/test_stream_order_gpu.py.  Also checked here, without a GPU: every case builds,
and the host arrays it hands to the library unchanged are what the wrappers' ``np.ascontiguousarray`` passes through."""
import os
import re

import numpy as np

from tests import stream_cases as sc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dcv.h")


def stream_entries():
    """Names of the functions declared in dcv.h whose parameter list holds ``void* stream``."""
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)      # comments (some quote prototypes)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)       # preprocessor lines
    out = []
    for m in re.finditer(r"\b(dcv_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            out.append(m.group(1))
    return out


def test_the_parser_finds_the_entries_it_should():
    found = stream_entries()
    assert len(found) == len(set(found)) and len(found) >= 45, found
    for name in ("dcv_col_stats", "dcv_superpose", "dcv_mlp_train_step", "dcv_mr_mst", "dcv_gemm_tn_split", "dcv_xtc_pack", "dcv_comm_allreduce"):
        assert name in found, name
    for name in ("dcv_mlp_create", "dcv_mlp_set_noise", "dcv_set_gemm_mode", "dcv_mlp_profile_begin", "dcv_col_stats_workspace"):
        assert name not in found, name


def test_every_stream_entry_has_a_case_or_a_reason():
    found = set(stream_entries())
    covered = sc.covered_entries()
    assert covered <= found, f"cases name entries the header does not have: {sorted(covered - found)}"
    assert set(sc.EXCLUDED) <= found, f"exclusions name entries the header does not have: {sorted(set(sc.EXCLUDED) - found)}"
    assert not covered & set(sc.EXCLUDED), sorted(covered & set(sc.EXCLUDED))
    missing = found - covered - set(sc.EXCLUDED)
    assert not missing, f"stream-taking entries without a case in tests/stream_cases.py: {sorted(missing)}"
    assert len(sc.EXCLUDED) <= 6 and all(len(reason) > 20 for reason in sc.EXCLUDED.values())


def test_cases_build_and_host_arrays_pass_through_the_wrappers_unchanged():
    from deep_cartograph_amd import _lib

    names = [c.name for c in sc.CASES]
    assert len(names) == len(set(names))
    for case in sc.CASES:
        dev, host = case.build()
        dev2, host2 = case.build()
        for k in dev:   # deterministic builders: reference and probes see the same inputs
            assert isinstance(dev[k], np.ndarray) and dev[k].flags.c_contiguous, (case.name, k)
            assert np.array_equal(dev[k].view(np.uint8), dev2[k].view(np.uint8)), (case.name, k)
            assert case.poison.get(k, sc.default_poison(dev[k])) in ("nan", "zeros"), (case.name, k)
            if case.poison.get(k) == "nan":
                assert np.issubdtype(dev[k].dtype, np.floating), (case.name, k)
        assert set(case.poison) <= set(dev) and set(case.host_arrays) <= set(host) and set(case.host_arrays) == set(case.host_dtypes), case.name
        for k in case.host_arrays:
            a = host[k]
            want = _lib.XTC_FRAME_DTYPE if case.host_dtypes[k] == "XTC_FRAME_DTYPE" else np.dtype(case.host_dtypes[k])
            assert a.dtype == want and a.flags.c_contiguous and a.flags.writeable, (case.name, k, a.dtype)
            assert np.ascontiguousarray(a, dtype=a.dtype) is a, (case.name, k)
        segments = case.steps(None, dev, host, None) if case.engine else case.steps(None, dev, host)
        # an asynchronous step has no host array: every table case that lists one says why it may hold the host
        if case.host_arrays and case.engine is None:
            assert all(s.blocks for seg in segments for s in seg), case.name
        # inside a segment no asynchronous step follows one that may hold the host: run alone, every asynchronous step of a
        # case is judged against the gate (the probes' waiver for steps behind a waiting one only ever applies across two streams)
        for seg in segments:
            kinds = [bool(s.blocks) for s in seg]
            assert kinds == sorted(kinds), (case.name, [s.name for s in seg])
