"""Hierarchical clustering without a GPU: the NumPy restatement of scipy's nearest-neighbour chain and of
scikit-learn's tree cut (tests/linkage_oracle.py) against the fixtures recorded from scipy and the reference
(tests/golden/linkage_golden.npz); statistics.cut_tree against the same labels; the argument checks of the C-ABI,
which come before any GPU call."""
import ctypes

import numpy as np
import pytest

from tests import linkage_oracle as lo
from tests.conftest import load_golden


@pytest.fixture(scope="module")
def golden():
    return load_golden("linkage_golden.npz")


@pytest.mark.parametrize("name", list(lo.POINT_SETS))
def test_point_sets_are_the_recorded_ones(golden, name):
    assert lo.digest(lo.points(name)) == str(golden[f"{name}.digest"])


@pytest.mark.parametrize("name", list(lo.POINT_SETS))
@pytest.mark.parametrize("method", lo.METHODS)
def test_restatement_equals_scipy_and_reference(golden, name, method):
    P = lo.points(name)
    n = len(P)
    Z, searches = lo.nn_chain(P, method)
    np.testing.assert_array_equal(Z[:, :2], golden[f"{name}.{method}.children"])
    np.testing.assert_array_equal(Z[:, 2], golden[f"{name}.{method}.heights"])
    np.testing.assert_array_equal(Z[:, 3], golden[f"{name}.{method}.sizes"])
    assert searches <= 3 * (n - 1)
    for row, k in enumerate(lo.CUTS):
        np.testing.assert_array_equal(lo.hc_cut(Z[:, :2], k), golden[f"{name}.{method}.labels"][row])


@pytest.mark.parametrize("name", list(lo.POINT_SETS))
@pytest.mark.parametrize("method", lo.METHODS)
def test_cut_tree_equals_reference_labels(golden, name, method):
    from deep_cartograph_amd import statistics

    children = golden[f"{name}.{method}.children"]
    for row, k in enumerate(lo.CUTS):
        np.testing.assert_array_equal(statistics.cut_tree(children, k), golden[f"{name}.{method}.labels"][row])
    np.testing.assert_array_equal(statistics.cut_tree(children, 1), np.zeros(len(children) + 1, dtype=np.int64))


def test_cut_tree_every_k_against_scikit_learn(golden):
    from sklearn.cluster._agglomerative import _hc_cut

    from deep_cartograph_amd import statistics

    children = golden["lattice.average.children"].astype(np.intp)
    n = len(children) + 1
    for k in list(range(1, 40)) + [n - 1, n]:
        np.testing.assert_array_equal(statistics.cut_tree(children, k), _hc_cut(k, children, n))
    with pytest.raises(ValueError, match="Cannot extract more clusters than samples"):
        statistics.cut_tree(children, n + 1)


def test_capi_refuses_bad_arguments_without_a_gpu_call():
    import __graft_entry__ as ge
    from deep_cartograph_amd import _lib

    ge.build()
    lib = _lib.load()
    EINVAL, ENOMEM = -1, -3
    Z = np.zeros((8, 4))
    searches = ctypes.c_int64(-7)
    P = 0x1000   # never dereferenced: every call below is refused before anything touches the device
    ws = 0x1000
    for n, d, method in ((1, 2, 0), (0, 2, 0), (8, 17, 0), (8, 0, 0), (8, 2, 3), (8, 2, -1)):
        assert lib.dcv_linkage(P, n, d, method, Z.ctypes.data, ctypes.byref(searches), ws, 1 << 40, None) == EINVAL
        assert b"dcv_linkage" in lib.dcv_last_error()
    assert lib.dcv_linkage_workspace(1, 2) == 0 and lib.dcv_linkage_workspace(8, 17) == 0
    need = lib.dcv_linkage_workspace(8, 2)
    assert need >= 8 * 8 * 8
    assert lib.dcv_linkage(P, 8, 2, 0, Z.ctypes.data, ctypes.byref(searches), ws, need - 1, None) == ENOMEM
    assert lib.dcv_linkage(P, 8, 2, 0, Z.ctypes.data, ctypes.byref(searches), None, need, None) == ENOMEM
    assert searches.value == -7 and not Z.any()
    # the matrix dominates: 8 bytes per pair, rows padded to 16 doubles
    n = 20000
    assert 8 * n * n <= lib.dcv_linkage_workspace(n, 2) <= 8 * n * (n + 16) + (1 << 20)


def test_hip_linkage_has_no_cpu_path():
    import torch

    from deep_cartograph_amd import hip
    from deep_cartograph_amd._lib import DcvError

    with pytest.raises(DcvError):
        hip.linkage(torch.zeros(8, 2, dtype=torch.float64), "complete")
