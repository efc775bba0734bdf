"""The lossy engine's C ABI without a GPU: symbols, argument errors (all checked before any
HIP call), the host restatement of the loss decision (fu_lossy_delivered) against Python
ints, and the test helper itself (tests/lossy_cases.py) against the pinned oracle."""
import ctypes

import numpy as np
import pytest

import coracle
import fu
from fu import _lib as L
from lossy_cases import delivered_np, delivered_py, hashed, hub60, lossy_python, oracle_lossy
from parity_util import assert_same_bits

LOSSY_SYMBOLS = ["fu_lossy_create", "fu_lossy_create_from_graph", "fu_lossy_set_loss", "fu_lossy_set_link_mask",
                 "fu_lossy_set_values", "fu_lossy_reset", "fu_lossy_run", "fu_lossy_run_timed", "fu_lossy_set_targets",
                 "fu_lossy_max_err", "fu_lossy_get_estimates", "fu_lossy_get_flows", "fu_lossy_get_round",
                 "fu_lossy_get_stats", "fu_lossy_synchronize", "fu_lossy_destroy", "fu_lossy_delivered"]


def test_every_lossy_symbol_loads():
    for s in LOSSY_SYMBOLS:
        assert hasattr(L.lib, s), s
        assert s in L.EXPORTED
    assert L.lib.fu_version() == 2
    assert hasattr(fu, "CollectAllLossy")


@pytest.mark.parametrize("p", [-0.1, 1.5, float("nan")])
def test_loss_probability_outside_the_unit_interval(p):
    """FU_ERR_ARG from fu_lossy_delivered (no handle needed) and, where a GPU gives a handle,
    from fu_lossy_set_loss, which keeps its old setting."""
    out = np.zeros(4, dtype=np.uint8)
    assert L.lib.fu_lossy_delivered(1, 1, 0, 4, p, L.ptr(out)) == -1
    assert L.lib.fu_lossy_set_loss(None, p, 0) == -1
    if fu.device_count() > 0:
        g = hub60()
        with fu.CollectAllLossy(g, np.ones(g.n)) as eng:
            with pytest.raises(fu.FuError) as ei:
                eng.set_loss(p, 3)
            assert ei.value.code == -1
        with pytest.raises(fu.FuError) as ei:
            fu.CollectAllLossy(g, np.ones(g.n), loss=p)
        assert ei.value.code == -1


def _create(rp, col, rev, v):
    out = L.vp()
    rc = L.lib.fu_lossy_create(len(rp) - 1, int(rp[-1]), L.ptr(rp), L.ptr(col), None if rev is None else L.ptr(rev),
                               L.ptr(v), 0, ctypes.byref(out))
    if rc == 0:
        L.lib.fu_lossy_destroy(out)
    return rc


def test_asymmetric_csr_is_a_graph_error():
    rp = np.array([0, 1, 1], dtype=np.int64)
    col = np.array([1], dtype=np.int32)
    assert _create(rp, col, None, np.ones(2)) == -5
    assert "not symmetric" in L.last_error()
    with pytest.raises(fu.FuError) as ei:
        fu.CollectAllLossy(rowptr=rp, col=col, values=np.ones(2))
    assert ei.value.code == -5
    g = fu.Graph.from_csr(rp, col, require_symmetric=False)
    with pytest.raises(fu.FuError) as ei:
        fu.CollectAllLossy(g, np.ones(2))
    assert ei.value.code == -5


def test_wrong_caller_rev_is_a_graph_error():
    """Two entries of a correct rev swapped (both still in range), an entry out of range and a
    negative one: FU_ERR_GRAPH before any HIP call, so no bad gather can reach a device."""
    g = hub60()
    rp, col, rev = g.arrays()
    v = np.ones(g.n)
    for bad in ("swap", "range", "negative"):
        r = rev.copy()
        if bad == "swap":
            r[[3, 57]] = r[[57, 3]]
        elif bad == "range":
            r[10] = g.E
        else:
            r[10] = -1
        assert _create(rp, col, r, v) == -5, bad
        assert "rev" in L.last_error()
    with pytest.raises(fu.FuError) as ei:
        r = rev.copy()
        r[[3, 57]] = r[[57, 3]]
        fu.CollectAllLossy(rowptr=rp, col=col, rev=r, values=v)
    assert ei.value.code == -5
    if fu.device_count() == 0:  # the correct rev passes every check and reaches the device probe
        assert _create(rp, col, rev, v) == -2
        assert "no HIP device" in L.last_error()


def test_other_bad_arguments():
    g = hub60()
    with pytest.raises(ValueError):
        fu.CollectAllLossy(g, np.ones((g.n, 2)))
    with pytest.raises(ValueError):
        fu.CollectAllLossy(g, np.ones(g.n + 1))
    rp, col, _ = g.arrays()
    c = col.copy()
    c[0] = g.n
    assert _create(rp, c, None, np.ones(g.n)) == -1
    assert L.lib.fu_lossy_run(None, 1, 0, None) == -1
    assert L.lib.fu_lossy_get_stats(None, None) == -1
    assert L.lib.fu_lossy_delivered(1, -1, 0, 0, 0.5, None) == -1
    assert L.lib.fu_lossy_delivered(1, 1, 0, 0, 0.5, None) == 0


@pytest.mark.parametrize("first", [0, 2 ** 31 + 5])
def test_delivered_equals_the_python_int_hash(first):
    """Slot for slot: 3 seeds x rounds {1, 2, 1000} x p {0, 0.25, 1} over 4096 slots, from slot
    0 and from a window past 2^31 (the slot index is a 64-bit counter). p = 0 delivers
    everything and p = 1 nothing; round 0 delivers nothing at any p."""
    n = 4096
    for seed in (0, 11, 0xFEDCBA9876543210):
        for r in (1, 2, 1000):
            for p in (0.0, 0.25, 1.0):
                got = fu.lossy_delivered(seed, r, first, n, p)
                assert got.dtype == np.uint8 and got.tolist() == delivered_py(seed, r, first, n, p), (seed, r, p)
                if p == 0.0:
                    assert got.all()
                if p == 1.0:
                    assert not got.any()
                if first == 0:
                    assert np.array_equal(got.astype(bool), delivered_np(seed, r, n, p))
        assert not fu.lossy_delivered(seed, 0, first, n, 0.0).any()
    lost = 1.0 - fu.lossy_delivered(11, 1, first, n, 0.25).mean()
    assert 0.2 < lost < 0.3  # 4096 draws: 0.25 +- 7 sigma
    assert not np.array_equal(fu.lossy_delivered(11, 1, first, n, 0.25), fu.lossy_delivered(11, 2, first, n, 0.25))
    assert not np.array_equal(fu.lossy_delivered(11, 1, first, n, 0.25), fu.lossy_delivered(12, 1, first, n, 0.25))


# ------------------------------------------------------------------------------------
# the helper itself, on the 60-node graph with one row of degree 49 (conditions on the
# yardstick: they hold without the engine)
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [1, 2, 9])
def test_helper_trace_without_loss_is_ca_sync(rounds):
    g = hub60()
    v = fu.uniform_values(g.n, seed=4)
    a, f, _ = oracle_lossy(*g.arrays(), v, rounds, hashed(0.0, 0, g.E))
    a_ref, f_ref = coracle.ca_sync(*g.arrays(), v, rounds)
    assert_same_bits(a, a_ref, "estimates")
    assert_same_bits(f, f_ref, "flows")


@pytest.mark.parametrize("p", [0.25, 1.0])
def test_helper_trace_equals_python_floats_under_loss(p):
    g = hub60()
    v = fu.uniform_values(g.n, seed=4)
    dl = hashed(p, 11, g.E)
    a, f, _ = oracle_lossy(*g.arrays(), v, 12, dl)
    a_py, f_py = lossy_python(*g.arrays(), v, 12, dl)
    assert_same_bits(a, a_py, "estimates")
    assert_same_bits(f, f_py, "flows")
    if p == 0.25:  # the loss changes the result, and the rule still converges to the mean
        a0, _ = coracle.ca_sync(*g.arrays(), v, 12)
        assert not np.array_equal(a, a0)
        a200, _ = lossy_python(*g.arrays(), v, 200, dl)
        tgt, _ = fu.component_means(g.rowptr, g.col, v)
        assert np.max(np.abs(a200 - tgt)) < 1e-12
