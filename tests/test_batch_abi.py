"""The batched collect-all engine's C ABI (the fu_batch section of include/fu.h) and its
Python front, on a host without a GPU: the symbols exist, and every check on the arguments
comes before the first HIP call, so a bad k or an asymmetric graph is reported as such and
only a valid call reaches "no HIP device"."""
import ctypes

import numpy as np
import pytest

import fu
from fu import _lib as L

BATCH_SYMBOLS = ["fu_batch_create", "fu_batch_create_from_graph", "fu_batch_reset", "fu_batch_run",
                 "fu_batch_run_timed", "fu_batch_set_targets", "fu_batch_max_err", "fu_batch_get_estimates",
                 "fu_batch_get_flows", "fu_batch_get_round", "fu_batch_synchronize", "fu_batch_destroy"]


def _ring(n=8):
    i = np.arange(n)
    return fu.Graph.from_edges(n, i, (i + 1) % n)


def test_symbols_exported_and_version_unchanged():
    for s in BATCH_SYMBOLS:
        assert hasattr(L.lib, s), s
        assert s in L.EXPORTED, s
    assert L.lib.fu_version() == 2


def test_null_handles_are_bad_arguments():
    buf = np.zeros(4)
    r, ms = L.i64(), L.f32()
    calls = [("fu_batch_reset", (None,)), ("fu_batch_run", (None, 1, 0, None)),
             ("fu_batch_run_timed", (None, 1, ctypes.byref(ms))), ("fu_batch_set_targets", (None, L.ptr(buf))),
             ("fu_batch_max_err", (None, L.ptr(buf))), ("fu_batch_get_estimates", (None, L.ptr(buf))),
             ("fu_batch_get_flows", (None, L.ptr(buf))), ("fu_batch_get_round", (None, ctypes.byref(r))),
             ("fu_batch_synchronize", (None,)), ("fu_batch_destroy", (None,))]
    for name, args in calls:
        assert getattr(L.lib, name)(*args) == -1, name  # FU_ERR_ARG
        assert "bad arguments" in L.last_error(), name
    g = _ring()
    out = L.vp()
    assert L.lib.fu_batch_create_from_graph(None, 2, L.ptr(buf), 0, ctypes.byref(out)) == -1
    assert "bad arguments" in L.last_error()
    assert L.lib.fu_batch_create_from_graph(g._h, 2, None, 0, ctypes.byref(out)) == -1
    assert "bad arguments" in L.last_error()
    assert L.lib.fu_batch_create(g.n, g.E, None, L.ptr(g.col), None, 2, L.ptr(buf), 0, ctypes.byref(out)) == -1
    assert "bad arguments" in L.last_error()
    assert L.lib.fu_batch_create(g.n, g.E, L.ptr(g.rowptr), L.ptr(g.col), None, 2, L.ptr(buf), 0, None) == -1
    assert "bad arguments" in L.last_error()


@pytest.mark.parametrize("k", [0, 17])
def test_k_out_of_range_names_the_range(k):
    g = _ring()
    v = np.zeros((g.n, max(k, 1)))
    out = L.vp()
    assert L.lib.fu_batch_create_from_graph(g._h, k, L.ptr(v), 0, ctypes.byref(out)) == -1
    assert "1..16" in L.last_error()
    assert L.lib.fu_batch_create(g.n, g.E, L.ptr(g.rowptr), L.ptr(g.col), L.ptr(g.rev), k, L.ptr(v), 0,
                                 ctypes.byref(out)) == -1
    assert "1..16" in L.last_error()
    with pytest.raises(fu.FuError, match=r"1\.\.16"):
        fu.CollectAllBatch(g, np.zeros((g.n, k)))


def test_asymmetric_csr_is_rejected():
    rp = np.array([0, 1, 1], dtype=np.int64)  # 0 -> 1 without 1 -> 0
    col = np.array([1], dtype=np.int32)
    with pytest.raises(fu.FuError, match="not symmetric") as ei:
        fu.CollectAllBatch(rowptr=rp, col=col, values=np.ones((2, 2)))
    assert ei.value.code == -5  # FU_ERR_GRAPH
    with pytest.raises(fu.FuError, match="symmetric") as ei:  # a rev that is not the reverse pairing
        fu.CollectAllBatch(rowptr=rp, col=col, rev=np.array([0], dtype=np.int32), values=np.ones((2, 2)))
    assert ei.value.code == -5
    g = fu.Graph.from_csr(rp, col, require_symmetric=False)
    with pytest.raises(fu.FuError, match="not symmetric") as ei:
        fu.CollectAllBatch(g, np.ones((2, 2)))
    assert ei.value.code == -5


def test_valid_create_without_a_gpu_says_no_hip_device():
    if fu.device_count() > 0:
        with fu.CollectAllBatch(_ring(), np.ones((8, 3))) as eng:
            assert (eng.K, eng.rounds_done) == (3, 0)
        return
    g = _ring()
    with pytest.raises(fu.FuError, match="no HIP device") as ei:
        fu.CollectAllBatch(g, np.ones((g.n, 3)))
    assert ei.value.code == -2  # FU_ERR_HIP
    with pytest.raises(fu.FuError, match="no HIP device"):
        fu.CollectAllBatch(rowptr=g.rowptr, col=g.col, values=np.ones((g.n, 16)))


def test_one_dimensional_values_are_not_reshaped():
    g = _ring()
    with pytest.raises(ValueError, match="shape"):
        fu.CollectAllBatch(g, np.ones(g.n))
    with pytest.raises(ValueError, match="shape"):
        fu.CollectAllBatch(rowptr=g.rowptr, col=g.col, values=np.ones(g.n))


def test_wrong_first_dimension():
    g = _ring()
    with pytest.raises(ValueError, match="graph.n"):
        fu.CollectAllBatch(g, np.ones((g.n + 1, 2)))
    with pytest.raises(ValueError, match="!= n"):
        fu.CollectAllBatch(rowptr=g.rowptr, col=g.col, values=np.ones((g.n - 1, 2)))
