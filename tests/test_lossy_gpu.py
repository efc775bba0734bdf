"""fu.CollectAllLossy (csrc/fu_lossy.hip) against restatements that do not run it: the recorded
fixtures and coracle.ca_sync without loss, the C oracle's replay of a synthetic RECV / FIRE_CA
trace (lossy_cases.oracle_lossy) under loss, Python floats where the inputs change. Every
comparison is by bit pattern, on estimates and flows.

The graph of most cases is parity_util._class_edge_graph(7): star centres of degrees 0 ... 12000.
The kernel's row classes change at degree 128 (light tiles / one block per row) and its heavy
rows are staged in chunks of 2048 slots; 127, 128, 129, 2047, 2048, 2049, 4095, 4096, 4097 and
8191, 8192, 8193 are all centres of that graph. The slot limit (2048) closes all of its light
tiles but two (a heavy row closes the first, the end of the graph the last), and none of them
holds 256 rows or no slot: the cases of section 8 run on lossy_cases.tile_limit_graph(), whose
tiles close in every way (test_engine_case_inputs.py has the census of both graphs)."""
import functools

import numpy as np
import pytest

import coracle
import fu
import oracle
from conftest import ca_sync_fixtures, load_npz
from lossy_cases import (SEED, TILE_ROWS, TILE_SLOTS, delivered_np, hashed, hub60, lossy_python, oracle_lossy, tile_limit_graph,
                         tile_segment)
from parity_util import CLASS_EDGE_DEGREES, FAMILIES, _class_edge_graph, assert_same_bits, count_neg_zero

pytestmark = pytest.mark.gpu


def _check(eng, a_ref, f_ref, what):
    assert_same_bits(eng.estimates(), a_ref, what + ("estimates",))
    assert_same_bits(eng.flows(), f_ref, what + ("flows",))


@functools.lru_cache(maxsize=None)
def _class_graph():
    return _class_edge_graph(7)


def _values(family, n):
    return fu.uniform_values(n, seed=3) if family == "uniform" else FAMILIES[family](n, seed=3)


@functools.lru_cache(maxsize=None)
def _class_ref(family, p, rounds, snaps=()):
    """(a, f, snapshots) after `rounds` rounds on the class graph at (p, SEED), from the oracle."""
    g = _class_graph()
    return oracle_lossy(*g.arrays(), _values(family, g.n), rounds, hashed(p, SEED, g.E), snaps=snaps)


# ------------------------------------------------------------------------------------
# 1. no loss: the engine is CollectAll
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,meta", ca_sync_fixtures())
def test_no_loss_equals_the_recorded_fixtures(name, meta):
    d = load_npz(meta["file"])
    rp, col = d["rowptr"], d["col"]
    eng = fu.CollectAllLossy(rowptr=rp, col=col, values=d["values"])
    done = 0
    for k, r in enumerate(int(r) + 1 for r in d["rounds"]):
        eng.run(r - done)
        done = r
        assert eng.rounds_done == r
        _check(eng, np.ascontiguousarray(d["last_avg"][k], dtype=np.float64),
               np.ascontiguousarray(d["flows"][k], dtype=np.float64), (name, r))
    assert eng.stats == (int(rp[-1]) * (done - 1), 0)
    eng.close()


def test_no_loss_on_every_row_class():
    """After 1, 3, 8 and 17 rounds against coracle.ca_sync / ca_rounds; the native rev and a
    caller's rev (oracle.build_rev) give the same handle."""
    g = _class_graph()
    v = _values("uniform", g.n)
    engs = [fu.CollectAllLossy(g, v), fu.CollectAllLossy(rowptr=g.rowptr, col=g.col, values=v),
            fu.CollectAllLossy(rowptr=g.rowptr, col=g.col, rev=oracle.build_rev(g.rowptr, g.col), values=v)]
    a = f = None
    done = 0
    for r in (1, 3, 8, 17):
        if a is None:
            a, f = coracle.ca_sync(*g.arrays(), v, r, nthreads=16)
        else:
            coracle.ca_rounds(*g.arrays(), v, r - done, a, f, nthreads=16)
        for q, eng in enumerate(engs):
            eng.run(r - done)
            _check(eng, a, f, ("handle", q, "round", r))
        done = r
    for eng in engs:
        eng.close()


# ------------------------------------------------------------------------------------
# 2. loss on every row class
# ------------------------------------------------------------------------------------
def test_loss_reaches_every_row_class():
    """A condition on the case below, from fu_lossy_delivered alone: at p = 0.25 every centre
    of degree >= 2 has a lost and a delivered slot within rounds 1-8 (so both branches run in
    every row class), and some row of degree 1 has its only slot lost."""
    g = _class_graph()
    D = np.stack([fu.lossy_delivered(SEED, r, 0, g.E, 0.25) for r in range(1, 9)]).astype(bool)
    for c, d in enumerate(CLASS_EDGE_DEGREES):
        if d >= 2:
            row = D[:, g.rowptr[c]:g.rowptr[c + 1]]
            assert row.any() and not row.all(), d
    leaves = np.flatnonzero(g.degrees == 1)
    assert len(leaves) and (~D[:, g.rowptr[leaves]]).any()


@pytest.mark.parametrize("p", [0.25, 0.9, 1.0])
def test_loss_on_every_row_class(p):
    g = _class_graph()
    eng = fu.CollectAllLossy(g, _values("uniform", g.n), loss=p, seed=SEED)
    done = 0
    for r in (1, 2, 5, 9):
        eng.run(r - done)
        done = r
        a, f, _ = _class_ref("uniform", p, r, snaps=tuple(range(9)) if r == 9 and p == 0.25 else ())
        _check(eng, a, f, ("p", p, "round", r))
    eng.close()


# ------------------------------------------------------------------------------------
# 3. the fp64 value domain under loss
# ------------------------------------------------------------------------------------
def test_value_domain_inputs_reach_the_edges():
    """From the oracle alone: `subn` reaches -0.0 in estimates and flows, `huge` reaches both
    infinities and NaN."""
    a, f, _ = _class_ref("subn", 0.25, 9)
    assert count_neg_zero(a) > 0 and count_neg_zero(f) > 0
    _, f3, _ = _class_ref("huge", 0.25, 3)
    a9, _, _ = _class_ref("huge", 0.25, 9)
    assert np.isposinf(f3).any() and np.isneginf(f3).any() and np.isnan(a9).any()


@pytest.mark.parametrize("family", ["subn", "huge"])
def test_value_domain_under_loss(family):
    g = _class_graph()
    eng = fu.CollectAllLossy(g, _values(family, g.n), loss=0.25, seed=SEED)
    done = 0
    for r in (3, 9):
        eng.run(r - done)
        done = r
        a, f, _ = _class_ref(family, 0.25, r)
        _check(eng, a, f, (family, "round", r))
    eng.close()


# ------------------------------------------------------------------------------------
# 4. split runs and parameters that change between runs
# ------------------------------------------------------------------------------------
def test_split_run_equals_one_run():
    g = _class_graph()
    v = _values("uniform", g.n)
    a, f, _ = oracle_lossy(*g.arrays(), v, 17, hashed(0.25, SEED, g.E))
    with fu.CollectAllLossy(g, v, loss=0.25, seed=SEED) as eng:
        eng.run(5)
        eng.run(12)
        assert eng.rounds_done == 17
        _check(eng, a, f, ("run(5); run(12)",))


def test_loss_changes_between_runs():
    """set_loss(0.5, 3) for rounds 0-5, set_loss(0, 0) for 6-11, set_loss(0.2, 9) for 12-16: the
    round counter is absolute, so round 12 draws element 12 of seed 9's stream."""
    g = _class_graph()
    v = _values("uniform", g.n)

    def delivered(r):
        p, seed = (0.5, 3) if r < 6 else (0.0, 0) if r < 12 else (0.2, 9)
        return delivered_np(seed, r, g.E, p)

    a, f, _ = oracle_lossy(*g.arrays(), v, 17, delivered)
    with fu.CollectAllLossy(g, v) as eng:
        for (p, seed), rounds in (((0.5, 3), 6), ((0.0, 0), 6), ((0.2, 9), 5)):
            eng.set_loss(p, seed)
            eng.run(rounds)
        _check(eng, a, f, ("three loss settings",))
        lost = sum(int((~delivered(r)).sum()) for r in range(1, 17))
        assert eng.stats == (g.E * 16, lost)


def test_link_outage_then_reset_and_rerun():
    """Every link of the degree-2049 centre is down (both directions) in rounds 3-7 and up again
    from round 8, at p = 0.1; then reset() and the same 12 rounds without the outage."""
    g = _class_graph()
    v = _values("uniform", g.n)
    c = CLASS_EDGE_DEGREES.index(2049)
    down = np.zeros(g.E, dtype=np.uint8)
    down[g.rowptr[c]:g.rowptr[c + 1]] = 1
    down[g.rev[g.rowptr[c]:g.rowptr[c + 1]]] = 1
    assert int(down.sum()) == 2 * 2049
    plain = hashed(0.1, SEED, g.E)
    masked = hashed(0.1, SEED, g.E, down)
    a, f, _ = oracle_lossy(*g.arrays(), v, 12, lambda r: masked(r) if 3 <= r <= 7 else plain(r))
    a2, f2, _ = oracle_lossy(*g.arrays(), v, 12, plain)
    assert not np.array_equal(a, a2)
    with fu.CollectAllLossy(g, v, loss=0.1, seed=SEED) as eng:
        eng.run(3)
        eng.set_link_mask(down)
        eng.run(5)
        eng.set_link_mask(None)
        eng.run(4)
        _check(eng, a, f, ("outage in rounds 3-7",))
        lost = sum(int((~(masked(r) if 3 <= r <= 7 else plain(r))).sum()) for r in range(1, 12))
        assert eng.stats == (g.E * 11, lost)
        eng.reset()
        assert eng.rounds_done == 0 and eng.stats == (0, 0)
        assert not eng.estimates().any() and not eng.flows().any()
        eng.run(12)
        _check(eng, a2, f2, ("after reset",))


# ------------------------------------------------------------------------------------
# 5. the inputs change in mid-run
# ------------------------------------------------------------------------------------
def test_set_values_in_mid_run():
    g = hub60()
    vs = [fu.uniform_values(g.n, seed=s) for s in (4, 5, 6)]
    dl = hashed(0.25, SEED, g.E)
    a, f = lossy_python(*g.arrays(), lambda r: vs[0] if r < 4 else vs[1] if r < 9 else vs[2], 14, dl)
    with fu.CollectAllLossy(g, vs[0], loss=0.25, seed=SEED) as eng:
        eng.run(4)
        eng.set_values(vs[1])
        eng.run(5)
        eng.set_values(vs[2])
        eng.run(5)
        assert eng.rounds_done == 14
        _check(eng, a, f, ("values replaced after rounds 4 and 9",))


# ------------------------------------------------------------------------------------
# 6. error trace and statistics
# ------------------------------------------------------------------------------------
def test_error_trace_max_err_and_stats():
    g = _class_graph()
    v = _values("uniform", g.n)
    tgt, _ = fu.component_means(g.rowptr, g.col, v)
    _, _, snaps = _class_ref("uniform", 0.25, 9, snaps=tuple(range(9)))
    want = np.array([np.max(np.abs(snaps[r] - tgt)) for r in range(9)])
    with fu.CollectAllLossy(g, v, loss=0.25, seed=SEED) as eng:
        eng.set_targets(tgt)
        trace = eng.run(9, err_every=1)
        assert_same_bits(trace, want, "error trace")
        assert_same_bits(np.array([eng.max_err()]), want[-1:], "max_err")
        zeros = sum(int((fu.lossy_delivered(SEED, r, 0, g.E, 0.25) == 0).sum()) for r in range(1, 9))
        assert eng.stats == (g.E * 8, zeros)
        t2 = tgt.copy()
        t2[5] = np.nan  # the NaN rule of the other engines: one NaN target makes the maximum NaN
        eng.set_targets(t2)
        assert np.isnan(eng.max_err())


def test_cli_bench_graph_with_loss(capsys):
    """`python -m fu bench-graph SPEC --loss P --loss-seed S` (in process): the usual line plus
    lost=<count>, the count being the zeros of fu_lossy_delivered over rounds 1 .. R-1."""
    from fu.__main__ import main

    assert main(["bench-graph", "er:n=2000,m=8000", "--rounds", "6", "--loss", "0.25", "--loss-seed", "4"]) == 0
    line = capsys.readouterr().out.strip()
    g = fu.Graph.from_spec("er:n=2000,m=8000", seed=1)
    zeros = sum(int((fu.lossy_delivered(4, r, 0, g.E, 0.25) == 0).sum()) for r in range(1, 6))
    assert line.startswith(f"graph n={g.n} E={g.E} ") and " rounds=6 " in line and " max_err=" in line
    assert line.endswith(f" lost={zeros}")


# ------------------------------------------------------------------------------------
# 7. edge shapes
# ------------------------------------------------------------------------------------
def test_one_node_isolated_nodes_and_a_single_edge():
    no_i32 = np.zeros(0, dtype=np.int32)
    with fu.CollectAllLossy(rowptr=np.zeros(2, dtype=np.int64), col=no_i32, values=np.array([3.5]), loss=0.5) as eng:
        eng.run(4)
        _check(eng, np.array([3.5]), np.zeros(0), ("n = 1",))
        assert eng.stats == (0, 0)
    v = np.array([1.0, -2.5, -0.0, 1e300, 5e-324])
    with fu.CollectAllLossy(rowptr=np.zeros(6, dtype=np.int64), col=no_i32, values=v, loss=1.0) as eng:
        eng.run(3)
        _check(eng, (v - 0.0) + 0.0, np.zeros(0), ("isolated nodes",))
    rp, col, rev = np.array([0, 1, 2], dtype=np.int64), np.array([1, 0], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    v = np.array([1.0, 4.0])
    a, f = lossy_python(rp, col, rev, v, 6, lambda r: np.zeros(2, dtype=bool))
    with fu.CollectAllLossy(rowptr=rp, col=col, values=v, loss=1.0, seed=5) as eng:
        eng.run(6)
        _check(eng, a, f, ("single edge, p = 1",))
        assert eng.stats == (2 * 5, 2 * 5)


# ------------------------------------------------------------------------------------
# 8. light tiles at the row limit and without slots, under loss
# ------------------------------------------------------------------------------------
TILE_STOPS = (1, 2, 5, 9)


def _lost(g, delivered, rounds):
    """The restated count of lost messages of rounds 1 .. rounds-1."""
    return sum(int((~delivered(r)).sum()) for r in range(1, rounds))


@pytest.mark.parametrize("family,p", [("uniform", 0.25), ("uniform", 1.0), ("wide", 0.25)])
def test_loss_on_tiles_closed_in_every_way(family, p):
    """Tiles of 256 rows with 0, 768 and 2048 slots, tiles closed by the slot limit, by a heavy
    row and by the end of the graph, after rounds 1, 2, 5 and 9 against the oracle's replay."""
    g = tile_limit_graph()
    v = _values(family, g.n)
    dl = hashed(p, SEED, g.E)
    with fu.CollectAllLossy(g, v, loss=p, seed=SEED) as eng:
        for r in TILE_STOPS:
            eng.run(r - eng.rounds_done)
            a, f, _ = oracle_lossy(*g.arrays(), v, r, dl)
            _check(eng, a, f, (family, "p", p, "round", r))
            assert eng.stats == (g.E * (r - 1), _lost(g, dl, r)), r
        if p == 1.0:
            assert eng.stats == (g.E * 8, g.E * 8)


def test_no_loss_on_tiles_closed_in_every_way():
    g = tile_limit_graph()
    v = _values("uniform", g.n)
    with fu.CollectAllLossy(g, v) as eng:
        for r in TILE_STOPS:
            eng.run(r - eng.rounds_done)
            a, f = coracle.ca_sync(*g.arrays(), v, r)
            _check(eng, a, f, ("p", 0, "round", r))
            assert eng.stats == (g.E * (r - 1), 0), r


def test_outage_of_a_whole_full_tile():
    """Every slot of the tile of 256 rows and 2048 slots (the 8-regular segment) is down in
    rounds 3-5, in both directions, at p = 0.25: all its threads take the lost branch, the
    256th row included, while its neighbours in the plan do not."""
    g = tile_limit_graph()
    v = _values("uniform", g.n)
    first, rows = tile_segment("rr8")
    assert rows == TILE_ROWS
    e0, e1 = int(g.rowptr[first]), int(g.rowptr[first + rows])
    assert e1 - e0 == TILE_SLOTS
    down = np.zeros(g.E, dtype=np.uint8)
    down[e0:e1] = 1
    down[g.rev[e0:e1]] = 1
    assert int(down.sum()) == TILE_SLOTS  # the segment is closed: every reverse slot is in the tile
    plain = hashed(0.25, SEED, g.E)
    masked = hashed(0.25, SEED, g.E, down)

    def delivered(r):
        return masked(r) if 3 <= r <= 5 else plain(r)

    assert int(plain(3)[e0:e1].sum()) > 0  # the mask takes down slots that the hash delivers
    with fu.CollectAllLossy(g, v, loss=0.25, seed=SEED) as eng:
        for r, mask in ((3, None), (4, down), (6, down), (9, None)):  # rounds 0-2, 3, 4-5, 6-8
            eng.set_link_mask(mask)
            eng.run(r - eng.rounds_done)
            a, f, _ = oracle_lossy(*g.arrays(), v, r, delivered)
            _check(eng, a, f, ("outage of a tile", "round", r))
            assert eng.stats == (g.E * (r - 1), _lost(g, delivered, r)), r
    a2, _, _ = oracle_lossy(*g.arrays(), v, 9, plain)
    assert not np.array_equal(a, a2)


# ------------------------------------------------------------------------------------
# 10. the rule itself: the reference's Peers under the recorded loss (tests/golden/)
# ------------------------------------------------------------------------------------
def test_reference_peers_under_recorded_loss():
    """hub_mix (rows of 2101 and 130 slots, light tiles, isolated rows) at the recorded (p, seed)
    and link mask, run from stop to stop: estimates and flows are what the reference's own
    on_receive / tick / avg_and_send left (make_golden.ca_lossy_sync), and the lost counter is
    the number of slots the recording marks lost."""
    import rule_cases

    d = rule_cases.load("lossy")
    with fu.CollectAllLossy(rowptr=d.rowptr, col=d.col, rev=d.rev, values=d.values) as eng:
        eng.set_loss(d.loss, d.seed)
        eng.set_link_mask(d.down)
        for q, stop in enumerate(d.stops):
            eng.run(stop - eng.rounds_done)
            _check(eng, d.last_avg[q], d.flows[q], ("reference peers", "after", stop))
            assert eng.stats == (d.E * (stop - 1), rule_cases.lost_before(d, stop)), stop
