"""The K-column entry points of the lossy and churn engines without a GPU: symbols, argument
errors (all before any HIP call), the Python classes' own shape checks, fu.churn_targets on
(n, K) values, the command line's --columns, and the K-dependent plan of light tiles restated on
the host against the graphs that the GPU tests run."""
import ctypes

import numpy as np
import pytest

import fu
from fu import _lib as L
from lossy_cases import hub60, tile_census, tile_limit_graph
from rev_columns_cases import (HEAVY_WIDTHS, WIDTHS, check_light_boundary_plan, chunk_slots, heavy_boundary_graph,
                               heavy_boundary_script, heavy_degrees, tile_census_k)

NEW_SYMBOLS = ["fu_lossy_create_k", "fu_lossy_create_from_graph_k", "fu_lossy_get_columns", "fu_churn_create_k",
               "fu_churn_create_from_graph_k", "fu_churn_get_columns"]
ENGINES = ["lossy", "churn"]


def test_every_new_symbol_loads():
    for s in NEW_SYMBOLS:
        assert hasattr(L.lib, s), s
        assert s in L.EXPORTED
    assert L.lib.fu_version() == 2  # not bumped
    for name in ("CollectAllLossyBatch", "CollectAllChurnBatch"):
        assert hasattr(fu, name) and name in fu.__all__
    assert issubclass(fu.CollectAllLossyBatch, fu.CollectAllLossy) and issubclass(fu.CollectAllChurnBatch, fu.CollectAllChurn)


def _create_k(eng, n, e, rp, col, rev, k, v):
    h = L.vp()
    rc = getattr(L.lib, f"fu_{eng}_create_k")(n, e, L.ptr(rp), L.ptr(col), L.ptr(rev), k, L.ptr(v), 0, ctypes.byref(h))
    if rc == 0:
        getattr(L.lib, f"fu_{eng}_destroy")(h)
    return rc


@pytest.mark.parametrize("eng", ENGINES)
def test_k_outside_1_to_16_is_an_argument_error(eng):
    g = hub60()
    rp, col, rev = g.arrays()
    v = np.ones((g.n, 17))
    for k in (0, 17, -1):
        assert _create_k(eng, g.n, g.E, rp, col, rev, k, v) == -1, k
        assert f"fu_{eng}_create_k" in L.last_error() and "1..16" in L.last_error()
        h = L.vp()
        rc = getattr(L.lib, f"fu_{eng}_create_from_graph_k")(g._h, k, L.ptr(v), 0, ctypes.byref(h))
        assert rc == -1 and f"fu_{eng}_create_from_graph_k" in L.last_error(), k
    assert _create_k(eng, g.n, g.E, None, col, rev, 2, v) == -1
    assert f"fu_{eng}_create_k" in L.last_error() and "bad arguments" in L.last_error()
    assert getattr(L.lib, f"fu_{eng}_get_columns")(None, None) == -1
    assert f"fu_{eng}_get_columns" in L.last_error()


@pytest.mark.parametrize("eng", ENGINES)
def test_graph_errors_come_through_the_k_creates_before_any_hip_call(eng):
    g = hub60()
    rp, col, rev = g.arrays()
    v = np.ones((g.n, 3))
    arp, acol = np.array([0, 1, 1], dtype=np.int64), np.array([1], dtype=np.int32)
    assert _create_k(eng, 2, 1, arp, acol, None, 3, np.ones((2, 3))) == -5
    assert "not symmetric" in L.last_error()
    h = L.vp()
    ag = fu.Graph.from_csr(arp, acol, require_symmetric=False)
    assert getattr(L.lib, f"fu_{eng}_create_from_graph_k")(ag._h, 3, L.ptr(np.ones((2, 3))), 0, ctypes.byref(h)) == -5
    r = rev.copy()
    r[[3, 57]] = r[[57, 3]]
    assert _create_k(eng, g.n, g.E, rp, col, r, 3, v) == -5 and "rev" in L.last_error()
    r = rev.copy()
    r[10] = g.E
    assert _create_k(eng, g.n, g.E, rp, col, r, 3, v) == -5
    if fu.device_count() == 0:  # valid arguments pass every check and reach the device probe
        for k in (1, 3, 16):
            assert _create_k(eng, g.n, g.E, rp, col, rev, k, np.ones((g.n, k))) == -2
            assert "no HIP device" in L.last_error()
        cls = {"lossy": fu.CollectAllLossyBatch, "churn": fu.CollectAllChurnBatch}[eng]
        with pytest.raises(fu.FuError, match="no HIP device"):
            cls(g, v)


@pytest.mark.parametrize("cls", [fu.CollectAllLossyBatch, fu.CollectAllChurnBatch])
def test_python_shape_errors(cls):
    g = hub60()
    with pytest.raises(ValueError):
        cls(g, np.ones(g.n))  # 1-D values
    with pytest.raises(ValueError):
        cls(g, np.ones((g.n + 1, 2)))
    rp, col, rev = g.arrays()
    with pytest.raises(ValueError):
        cls(rowptr=rp, col=col, rev=rev, values=np.ones((g.n - 1, 2)))
    # a stand-in handle of 3 columns that no C entry point may see
    eng = object.__new__(cls)
    eng.n, eng.E, eng._h, eng._cols = g.n, g.E, None, 3
    for bad in (np.ones(g.n), np.ones((g.n, 2)), np.ones((g.n + 1, 3))):
        with pytest.raises(ValueError):
            eng.set_targets(bad)
        with pytest.raises(ValueError):
            eng.set_values(bad)
    # the scalar classes keep rejecting 2-D values
    for scalar in (fu.CollectAllLossy, fu.CollectAllChurn):
        with pytest.raises(ValueError):
            scalar(g, np.ones((g.n, 2)))


def test_churn_targets_on_columns_equals_a_call_per_column():
    g = hub60()
    V = np.stack([fu.uniform_values(g.n, seed=s) for s in (2, 3, 4)], axis=1)
    alive = np.ones(g.n, dtype=np.uint8)
    alive[[0, 7, 30]] = 0
    up = np.ones(g.E, dtype=np.uint8)
    up[[5, g.rev[5]]] = 0
    for a, u in ((None, None), (alive, None), (alive, up)):
        got = fu.churn_targets(g, V, a, u)
        assert got.shape == (g.n, 3)
        for c in range(3):
            np.testing.assert_array_equal(got[:, c], fu.churn_targets(g, V[:, c], a, u))
    with pytest.raises(ValueError):
        fu.churn_targets(g, np.ones((g.n + 1, 2)))


def test_cli_columns_needs_loss_or_churn(capsys):
    from fu.__main__ import main

    for extra in ([], ["--pairs"]):
        with pytest.raises(SystemExit) as ex:
            main(["bench-graph", "er:n=200,m=800", "--rounds", "4", "--columns", "3"] + extra)
        assert ex.value.code == 2
        assert "--columns" in capsys.readouterr().err
    for k in ("0", "17"):
        with pytest.raises(SystemExit) as ex:
            main(["bench-graph", "er:n=200,m=800", "--rounds", "4", "--loss", "0.1", "--columns", k])
        assert ex.value.code == 2
        capsys.readouterr()


# ------------------------------------------------------------------------------------
# the plan of light tiles for K columns
# ------------------------------------------------------------------------------------
def test_the_plan_for_one_column_is_the_scalar_plan():
    g = tile_limit_graph()
    assert tile_census_k(g.rowptr, 1) == tile_census(g.rowptr)


@pytest.mark.parametrize("K", WIDTHS)
def test_boundary_graph_closes_its_tiles_in_every_way(K):
    tiles = check_light_boundary_plan(K)
    assert {"rows", "slots", "heavy", "end"} <= {t[3] for t in tiles}
    # tile_limit_graph() under the plan of K: every tile within both limits, and both kinds of
    # closing still occur
    census = tile_census_k(tile_limit_graph().rowptr, K)
    assert all(j - i <= 256 // K and s * K <= 2048 for i, j, s, _ in census)
    assert {"rows", "slots"} <= {t[3] for t in census}


@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_heavy_boundary_graph_and_script(K):
    g, rows = heavy_boundary_graph(K)
    ce = chunk_slots(K)
    assert sorted(rows) == heavy_degrees(K) and {129, ce + 1, 2 * ce, 2 * ce + 1} <= set(rows)
    if K == 16:
        assert ce + 1 == 129
    assert sorted(rows.values())[-2:] == [g.n - 2, g.n - 1] and min(rows.values()) == 0
    script, events = heavy_boundary_script(K)
    assert sum(s[1] for s in script if s[0] == "run") <= 12
    live = [fu.churn_live(g, a, u).astype(bool) for a, u in events]
    for d, h in rows.items():
        ks = np.arange(g.rowptr[h], g.rowptr[h + 1])
        if d > ce:  # DOWN on both sides of the chunk boundary, live slots beside them
            assert not live[0][ks[[ce - 1, ce]]].any() and live[0][ks[ce - 2]] and (d in (ce + 1, 2 * ce) or live[0][ks[ce + 1]])
    ks = np.arange(g.rowptr[rows[2 * ce]], g.rowptr[rows[2 * ce] + 1])
    assert not live[0][ks[ce:2 * ce]].any() and live[0][ks[:ce]].any()  # a whole chunk DOWN
    was, now = live[0][ks[ce:2 * ce]], live[1][ks[ce:2 * ce]]
    assert now.any() and (~now).any()  # FRESH and DOWN in that chunk after the revival
    ks0 = ks[:ce]
    assert (live[0][ks0] & live[1][ks0]).any() and (~live[0][ks0] & live[1][ks0]).any() and (~live[1][ks0]).any()  # UP, FRESH, DOWN
    a3, u3 = events[2]
    lo, hi = rows[min(rows)], rows[max(rows)]
    assert a3[lo] == 1 and not live[2][g.rowptr[lo]:g.rowptr[lo + 1]].any()  # alive, no live slot
    assert a3[hi] == 0  # a dead heavy row
    del was
