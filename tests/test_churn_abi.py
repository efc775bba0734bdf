"""The churn engine's C ABI without a GPU: symbols, the host restatement of the liveness rule
(fu_churn_live) against numpy, argument errors (all checked before any HIP call), the Python
class's own shape checks and the command line's exclusive options."""
import ctypes

import numpy as np
import pytest

import fu
from churn_cases import byte_masks, cut, hub60, live_np, random_masks
from fu import _lib as L

CHURN_SYMBOLS = ["fu_churn_create", "fu_churn_create_from_graph", "fu_churn_set_topology", "fu_churn_set_values",
                 "fu_churn_reset", "fu_churn_run", "fu_churn_run_timed", "fu_churn_set_targets", "fu_churn_max_err",
                 "fu_churn_get_estimates", "fu_churn_get_flows", "fu_churn_get_round", "fu_churn_get_stats",
                 "fu_churn_get_slot_state", "fu_churn_synchronize", "fu_churn_destroy", "fu_churn_live"]


def test_every_churn_symbol_loads():
    for s in CHURN_SYMBOLS:
        assert hasattr(L.lib, s), s
        assert s in L.EXPORTED
    assert L.lib.fu_version() == 2
    for name in ("CollectAllChurn", "churn_live", "churn_targets"):
        assert hasattr(fu, name) and name in fu.__all__


# ------------------------------------------------------------------------------------
# fu_churn_live
# ------------------------------------------------------------------------------------
def _live(rp, col, rev, alive, link_up):
    out = np.full(max(int(rp[-1]), 1), 7, dtype=np.uint8)
    rc = L.lib.fu_churn_live(len(rp) - 1, L.ptr(rp), L.ptr(col), L.ptr(rev), L.ptr(alive), L.ptr(link_up), L.ptr(out))
    return rc, out[:int(rp[-1])]


def test_live_equals_the_numpy_rule():
    g = hub60()
    rp, col, rev = g.arrays()
    for seed in range(6):
        alive, up = random_masks(g, 0.2, 0.2, seed)
        assert 0 < alive.sum() < g.n and 0 < up.sum() < g.E
        want = live_np(rp, col, rev, alive, up)
        for r in (rev, None):  # the native rev gives the same answer
            rc, got = _live(rp, col, r, alive, up)
            assert rc == 0 and np.array_equal(got.astype(bool), want), seed
        assert np.array_equal(fu.churn_live(g, alive, up).astype(bool), want)
        assert np.array_equal(fu.churn_live((rp, col, None), alive.astype(bool), up.astype(np.int64)).astype(bool), want)
        # any non-zero byte is "on"
        assert np.array_equal(_live(rp, col, rev, alive * 200, up * 3)[1].astype(bool), want)
    ones_n, ones_e = np.ones(g.n, dtype=np.uint8), np.ones(g.E, dtype=np.uint8)
    for alive, up in ((ones_n, ones_e), (None, None), (ones_n, None), (None, ones_e)):
        rc, got = _live(rp, col, rev, alive, up)
        assert rc == 0 and got.dtype == np.uint8 and (got == 1).all()
    alive, up = random_masks(g, 0.2, 0.2, 9)
    assert np.array_equal(_live(rp, col, rev, alive, None)[1].astype(bool), live_np(rp, col, rev, alive, None))
    assert np.array_equal(_live(rp, col, rev, None, up)[1].astype(bool), up.astype(bool))


def test_live_with_mask_bytes_other_than_0_and_1():
    """The masks of test_churn_gpu.test_any_nonzero_mask_byte_is_on: alive bytes from {0, 1, 2,
    128, 255}, link_up 7 on a slot and 255 on its reverse. The symmetry check compares zero with
    non-zero, not the bytes, and the answer is the one for the same masks as 0 / 1."""
    g = hub60()
    rp, col, rev = g.arrays()
    alive, up = byte_masks(g, 71)
    want = live_np(rp, col, rev, alive != 0, up != 0)
    assert 0 < want.sum() < (up != 0).sum()
    for r in (rev, None):
        rc, got = _live(rp, col, r, alive, up)
        assert rc == 0 and np.array_equal(got, want.astype(np.uint8))  # 0 / 1 out, whatever came in
        rc, norm = _live(rp, col, r, (alive != 0).astype(np.uint8), (up != 0).astype(np.uint8))
        assert rc == 0 and np.array_equal(got, norm)


def test_live_with_a_dead_hub():
    """Every slot of the hub's row and every slot that points at the hub is off; the rest stay."""
    g = hub60()
    rp, col, rev = g.arrays()
    alive = np.ones(g.n, dtype=np.uint8)
    alive[0] = 0
    rc, got = _live(rp, col, rev, alive, None)
    src = np.repeat(np.arange(g.n), np.diff(rp))
    assert rc == 0 and np.array_equal(got.astype(bool), (src != 0) & (col != 0))
    assert int((got == 0).sum()) == 2 * 49


def test_live_argument_errors():
    g = hub60()
    rp, col, rev = g.arrays()
    up = np.ones(g.E, dtype=np.uint8)
    k = int(rp[5])
    up[k] = 0  # one direction only
    assert up[rev[k]] == 1
    rc, _ = _live(rp, col, rev, None, up)
    assert rc == -1 and "link_up" in L.last_error()
    with pytest.raises(fu.FuError) as ei:
        fu.churn_live(g, None, up)
    assert ei.value.code == -1
    assert _live(rp, col, rev, None, cut(g, np.ones(g.E, dtype=np.uint8), [k]))[0] == 0
    r = rev.copy()
    r[[3, 57]] = r[[57, 3]]
    rc, _ = _live(rp, col, r, None, None)
    assert rc == -5 and "rev" in L.last_error()
    r = rev.copy()
    r[10] = g.E
    assert _live(rp, col, r, None, None)[0] == -5
    # an asymmetric graph, with the native rev
    assert _live(np.array([0, 1, 1], dtype=np.int64), np.array([1], dtype=np.int32), None, None, None)[0] == -5
    c = col.copy()
    c[0] = g.n
    assert _live(rp, c, rev, None, None)[0] == -1
    out = np.zeros(4, dtype=np.uint8)
    assert L.lib.fu_churn_live(0, L.ptr(rp), L.ptr(col), None, None, None, L.ptr(out)) == -1
    assert L.lib.fu_churn_live(g.n, None, L.ptr(col), None, None, None, L.ptr(out)) == -1
    assert L.lib.fu_churn_live(g.n, L.ptr(rp), L.ptr(col), None, None, None, None) == -1


# ------------------------------------------------------------------------------------
# fu_churn_create: every argument error before any HIP call
# ------------------------------------------------------------------------------------
def _create(n, e, rp, col, rev, v, out=True):
    h = L.vp()
    rc = L.lib.fu_churn_create(n, e, L.ptr(rp), L.ptr(col), L.ptr(rev), L.ptr(v), 0, ctypes.byref(h) if out else None)
    if rc == 0:
        L.lib.fu_churn_destroy(h)
    return rc


def test_create_argument_errors_come_before_any_hip_call():
    g = hub60()
    rp, col, rev = g.arrays()
    v = np.ones(g.n)
    assert _create(0, g.E, rp, col, rev, v) == -1
    assert _create(-3, g.E, rp, col, rev, v) == -1
    assert _create(g.n, -1, rp, col, rev, v) == -1
    assert _create(g.n, g.E, None, col, rev, v) == -1
    assert _create(g.n, g.E, rp, None, rev, v) == -1
    assert _create(g.n, g.E, rp, col, rev, None) == -1
    assert _create(g.n, g.E, rp, col, rev, v, out=False) == -1
    assert "bad arguments" in L.last_error()
    assert _create(g.n, g.E - 1, rp, col, rev, v) == -1  # rowptr[n] != e
    c = col.copy()
    c[0] = g.n
    assert _create(g.n, g.E, rp, c, None, v) == -1
    # an asymmetric graph
    arp, acol = np.array([0, 1, 1], dtype=np.int64), np.array([1], dtype=np.int32)
    assert _create(2, 1, arp, acol, None, np.ones(2)) == -5
    assert "not symmetric" in L.last_error()
    with pytest.raises(fu.FuError) as ei:
        fu.CollectAllChurn(rowptr=arp, col=acol, values=np.ones(2))
    assert ei.value.code == -5
    with pytest.raises(fu.FuError) as ei:
        fu.CollectAllChurn(fu.Graph.from_csr(arp, acol, require_symmetric=False), np.ones(2))
    assert ei.value.code == -5
    # a bad rev: two entries swapped, one out of range, one negative
    for bad in ("swap", "range", "negative"):
        r = rev.copy()
        if bad == "swap":
            r[[3, 57]] = r[[57, 3]]
        else:
            r[10] = g.E if bad == "range" else -1
        assert _create(g.n, g.E, rp, col, r, v) == -5, bad
        assert "rev" in L.last_error()
    if fu.device_count() == 0:  # valid arguments pass every check and reach the device probe
        for r in (rev, None):
            assert _create(g.n, g.E, rp, col, r, v) == -2
            assert "no HIP device" in L.last_error()
        with pytest.raises(fu.FuError, match="no HIP device"):
            fu.CollectAllChurn(g, v)


def test_null_handles_are_argument_errors():
    for name, args in (("fu_churn_set_topology", (None, None)), ("fu_churn_set_values", (None,)), ("fu_churn_reset", ()),
                       ("fu_churn_run", (1, 0, None)), ("fu_churn_run_timed", (1, None)), ("fu_churn_set_targets", (None,)),
                       ("fu_churn_max_err", (None,)), ("fu_churn_get_estimates", (None,)), ("fu_churn_get_flows", (None,)),
                       ("fu_churn_get_round", (None,)), ("fu_churn_get_stats", (None,)),
                       ("fu_churn_get_slot_state", (None,)), ("fu_churn_synchronize", ()), ("fu_churn_destroy", ())):
        assert getattr(L.lib, name)(None, *args) == -1, name
        assert name in L.last_error()


# ------------------------------------------------------------------------------------
# Python-side checks
# ------------------------------------------------------------------------------------
def test_python_shape_errors():
    g = hub60()
    with pytest.raises(ValueError):
        fu.CollectAllChurn(g, np.ones((g.n, 2)))
    with pytest.raises(ValueError):
        fu.CollectAllChurn(g, np.ones(g.n + 1))
    rp, col, rev = g.arrays()
    with pytest.raises(ValueError):
        fu.CollectAllChurn(rowptr=rp, col=col, rev=rev[:-1], values=np.ones(g.n))
    # set_topology, set_values and set_targets check before the C call: a stand-in handle that
    # no C entry point may see
    eng = object.__new__(fu.CollectAllChurn)
    eng.n, eng.E, eng._h = g.n, g.E, None
    for kw in ({"alive": np.ones(g.n + 1, dtype=np.uint8)}, {"alive": np.ones((g.n, 1), dtype=np.uint8)},
               {"link_up": np.ones(g.E - 1, dtype=np.uint8)}, {"alive": np.ones(g.E, dtype=np.uint8)},
               {"alive": np.ones(g.n)}, {"link_up": np.ones(g.E, dtype=np.float32)}):
        with pytest.raises(ValueError):
            eng.set_topology(**kw)
    with pytest.raises(ValueError):
        eng.set_values(np.ones(g.n + 1))
    with pytest.raises(ValueError):
        eng.set_targets(np.ones((g.n, 2)))
    with pytest.raises(ValueError):
        fu.churn_live(g, np.ones(g.n - 1, dtype=np.uint8), None)
    with pytest.raises(ValueError):
        fu.churn_targets(g, np.ones(g.n), None, np.ones(g.E + 1, dtype=np.uint8))


def test_churn_targets_are_the_means_of_the_alive_inputs_per_live_component():
    g = hub60()
    v = fu.uniform_values(g.n, seed=2)
    tgt, _ = fu.component_means(g.rowptr, g.col, v)
    np.testing.assert_array_equal(fu.churn_targets(g, v), tgt)
    alive = np.ones(g.n, dtype=np.uint8)
    alive[0] = 0
    t = fu.churn_targets(g, v, alive)
    assert t[0] == v[0]
    live = live_np(*g.arrays(), alive, None)
    # label propagation over the live slots: the components of the alive nodes
    comp = np.arange(g.n)
    src = np.repeat(np.arange(g.n), np.diff(g.rowptr))
    for _ in range(g.n):
        new = comp.copy()
        np.minimum.at(new, src[live], comp[g.col[live]])
        if np.array_equal(new, comp):
            break
        comp = new
    assert len(set(comp[1:])) >= 1
    for c in set(comp):
        m = comp == c
        assert np.allclose(t[m], v[m].mean(), rtol=1e-14, atol=0.0), c


def test_cli_churn_is_exclusive_with_loss_and_pairs(capsys):
    from fu.__main__ import main

    for extra in (["--loss", "0.1"], ["--pairs"], ["--loss", "0.1", "--pairs"]):
        with pytest.raises(SystemExit) as ex:
            main(["bench-graph", "er:n=200,m=800", "--rounds", "4", "--churn", "0.1"] + extra)
        assert ex.value.code == 2
        assert "exclusive" in capsys.readouterr().err
