"""K value columns in the lossy and churn engines (fu.CollectAllLossyBatch, fu.CollectAllChurnBatch;
csrc/fu_rev_round.h k_light_cols and k_heavy_cols): every column of a K-column run holds the bits
of a reference run of that column alone, and what belongs to a message (the loss decision, the
statistics, the slot states) is that of one column. The references never run the engine:
churn_cases.churn_python, lossy_cases.oracle_lossy / lossy_python once per column, the recordings
of the reference's Peer code (rule_cases), coracle.ca_sync on the live subgraph.

Nearly every value here is fu.uniform_values: one sign, one decade, no zero, nothing non-finite.
Signed zeros, subnormals, overflow, infinities and NaN as columns, against the reference's
value-domain recordings, are in test_rev_columns_value_domain_gpu.py (inputs and Python references:
test_rev_columns_value_domain.py, rev_columns_vd_cases.py)."""
import numpy as np
import pytest

import fu
import rule_cases
from churn_cases import UP, check_static, churn_python, flapping_case, random_masks
from lossy_cases import hashed, lossy_python, tile_limit_graph, tile_segment
from parity_util import FAMILIES, assert_same_bits
from rev_columns_cases import (HEAVY_WIDTHS, LOSS_SEED, WIDTHS, churn_reference, chunk_slots, columns,
                               drive_churn, heavy_boundary_graph, heavy_boundary_script, light_boundary_graph, link_mask,
                               lossy_reference)

pytestmark = pytest.mark.gpu


def _width_graph(which, K):
    return tile_limit_graph() if which == "tile_limit" else light_boundary_graph(K)[0]


# ------------------------------------------------------------------------------------
# 1. pinned to the reference's Peer code
# ------------------------------------------------------------------------------------
def _rule_columns(d):
    """The recorded values as column 0, a permutation of them and uniform values beside them."""
    perm = np.random.default_rng(3).permutation(d.n)
    return np.ascontiguousarray(np.stack([d.values, d.values[perm], fu.uniform_values(d.n, seed=8)], axis=1))


def test_lossy_column_0_reproduces_the_recorded_peer_run():
    d = rule_cases.load("lossy")
    V = _rule_columns(d)
    delivered = lambda r: d.delivered[r]  # noqa: E731
    with fu.CollectAllLossyBatch(rowptr=d.rowptr, col=d.col, rev=d.rev, values=V, loss=d.loss, seed=d.seed) as eng:
        eng.set_link_mask(d.down)
        done = 0
        for q, stop in enumerate(d.stops):
            eng.run(stop - done)
            done = stop
            a, f = eng.estimates(), eng.flows()
            assert_same_bits(a[:, 0], d.last_avg[q], ("recorded estimates", stop))
            assert_same_bits(f[:, 0], d.flows[q], ("recorded flows", stop))
            assert eng.stats == (d.E * (stop - 1), rule_cases.lost_before(d, stop))
            if stop <= 12:
                for c in (1, 2):
                    ra, rf = lossy_python(d.rowptr, d.col, d.rev, V[:, c], stop, delivered)
                    assert_same_bits(a[:, c], ra, ("estimates", stop, c))
                    assert_same_bits(f[:, c], rf, ("flows", stop, c))


def test_churn_column_0_reproduces_the_recorded_peer_run():
    d = rule_cases.load("churn")
    V = _rule_columns(d)
    states = rule_cases.churn_states_after_events(d)
    ref = {c: churn_python(d.rowptr, d.col, d.rev, V[:, c], rule_cases.churn_script(d, 12)) for c in (1, 2)}
    with fu.CollectAllChurnBatch(rowptr=d.rowptr, col=d.col, rev=d.rev, values=V) as eng:
        done = 0
        for q, stop in enumerate(d.stops):
            e = d.event_rounds.index(done)
            if done > 0:
                eng.set_topology(d.alive[e], d.link_up[e])
                assert np.array_equal(eng.slot_state(), states[e])
            if done < 12 <= stop:
                eng.run(12 - done)
                done = 12
                for c in (1, 2):
                    assert_same_bits(eng.estimates()[:, c], ref[c].a, ("estimates at 12", c))
                    assert_same_bits(eng.flows()[:, c], ref[c].f, ("flows at 12", c))
            eng.run(stop - done)
            done = stop
            assert_same_bits(eng.estimates()[:, 0], d.last_avg[q], ("recorded estimates", stop))
            assert_same_bits(eng.flows()[:, 0], d.flows[q], ("recorded flows", stop))


# ------------------------------------------------------------------------------------
# 2. widths
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tile_limit", "boundary"])
@pytest.mark.parametrize("K", WIDTHS)
def test_lossy_widths(K, which):
    g = _width_graph(which, K)
    V = columns(g.n, K, first=20)
    down = link_mask(g, 0.1, 5)
    want_a, want_f = lossy_reference(g, V, (10,), 0.3, down=down)[10]
    with fu.CollectAllLossyBatch(g, V, loss=0.3, seed=LOSS_SEED) as eng:
        eng.set_link_mask(down)
        eng.run(10)
        assert_same_bits(eng.estimates(), want_a, (K, which, "estimates"))
        assert_same_bits(eng.flows(), want_f, (K, which, "flows"))
        if K == 1:
            with fu.CollectAllLossy(g, V[:, 0], loss=0.3, seed=LOSS_SEED) as old:
                old.set_link_mask(down)
                old.run(10)
                assert_same_bits(eng.estimates()[:, 0], old.estimates(), "old create, estimates")
                assert_same_bits(eng.flows()[:, 0], old.flows(), "old create, flows")
                assert eng.stats == old.stats


@pytest.mark.parametrize("which", ["tile_limit", "boundary"])
@pytest.mark.parametrize("K", WIDTHS)
def test_churn_widths(K, which):
    g = _width_graph(which, K)
    V = columns(g.n, K, first=20)
    hub = int(np.argmax(g.degrees))
    t1, t2 = random_masks(g, 0.2, 0.1, 60 + K, keep=(hub,)), random_masks(g, 0.1, 0.2, 80 + K)
    script = [("run", 4), ("topology",) + t1, ("run", 3), ("topology",) + t2, ("run", 3)]
    steps = churn_reference(g, V, script)
    with fu.CollectAllChurnBatch(g, V) as eng:
        drive_churn(eng, script, steps, (K, which))
        if K == 1:
            with fu.CollectAllChurn(g, V[:, 0]) as old:
                drive_churn(old, script, [s._replace(a=s.a[:, 0], f=s.f[:, 0]) for s in steps], ("old create", which))


# ------------------------------------------------------------------------------------
# 3. heavy rows at the chunk edges
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_churn_heavy_chunk_edges(K):
    g, rows = heavy_boundary_graph(K)
    assert chunk_slots(K) + 1 in rows and 2 * chunk_slots(K) + 1 in rows
    script, _ = heavy_boundary_script(K)
    V = columns(g.n, K, first=30)
    with fu.CollectAllChurnBatch(g, V) as eng:
        drive_churn(eng, script, churn_reference(g, V, script), (K,))


@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_lossy_heavy_chunk_edges(K):
    g, _ = heavy_boundary_graph(K)
    V = columns(g.n, K, first=30)
    stops = (1, 2, 5, 10)
    want = lossy_reference(g, V, stops, 0.5)
    lost = 0
    with fu.CollectAllLossyBatch(g, V, loss=0.5, seed=LOSS_SEED) as eng:
        done = 0
        for stop in stops:
            eng.run(stop - done)
            lost += sum(int((~hashed(0.5, LOSS_SEED, g.E)(r)).sum()) for r in range(max(done, 1), stop))
            done = stop
            assert_same_bits(eng.estimates(), want[stop][0], (K, "estimates", stop))
            assert_same_bits(eng.flows(), want[stop][1], (K, "flows", stop))
            assert eng.stats == (g.E * (stop - 1), lost)


# ------------------------------------------------------------------------------------
# 4. column isolation
# ------------------------------------------------------------------------------------
def _special_columns(g):
    """Finite columns 0, 2 and 4 beside an all-NaN column, a column with +-inf and -0.0 inputs on
    the busiest rows' neighbourhood, and a subnormal one."""
    n = g.n
    fin = columns(n, 3, first=40)
    inf = fu.uniform_values(n, seed=44)
    hub = int(np.argmax(g.degrees))
    nb = g.col[g.rowptr[hub]:g.rowptr[hub + 1]]
    inf[nb[:3]] = [np.inf, -np.inf, -0.0]
    inf[hub] = -0.0
    V = np.stack([fin[:, 0], np.full(n, np.nan), fin[:, 1], inf, fin[:, 2], FAMILIES["subn"](n, 4)], axis=1)
    return np.ascontiguousarray(V), [0, 2, 4]


def _run(cls, g, V, rounds, prepare):
    with cls(g, np.ascontiguousarray(V)) as eng:
        prepare(eng)
        eng.run(rounds)
        return eng.estimates(), eng.flows()


@pytest.mark.parametrize("engine", ["lossy", "churn"])
def test_columns_do_not_see_each_other(engine):
    g = tile_limit_graph()
    V, finite = _special_columns(g)
    if engine == "lossy":
        cls = fu.CollectAllLossyBatch
        prepare = lambda eng: eng.set_loss(0.3, LOSS_SEED)  # noqa: E731
    else:
        cls = fu.CollectAllChurnBatch
        alive, up = random_masks(g, 0.2, 0.1, 7, keep=(tile_segment("heavy")[0],))
        prepare = lambda eng: (eng.run(2), eng.set_topology(alive, up))  # noqa: E731
    a, f = _run(cls, g, V, 8, prepare)
    assert np.isnan(a[:, 1]).any() and not np.isfinite(a[:, 3]).all()
    assert np.isfinite(a[:, finite]).all() and np.isfinite(f[:, finite]).all()
    a2, f2 = _run(cls, g, V[:, finite], 8, prepare)  # without the special columns
    assert_same_bits(a[:, finite], a2, "estimates beside special columns")
    assert_same_bits(f[:, finite], f2, "flows beside special columns")
    a3, f3 = _run(cls, g, V[:, [3, 0, 3, 5, 5]], 8, prepare)  # the same column twice
    assert_same_bits(a3[:, 0], a3[:, 2], "twice, estimates")
    assert_same_bits(f3[:, 3], f3[:, 4], "twice, flows")
    assert_same_bits(a3[:, 0], a[:, 3], "the column in another place")
    a4, f4 = _run(cls, g, V[:, ::-1], 8, prepare)  # the columns in reverse order
    assert_same_bits(a4, a[:, ::-1], "reverse, estimates")
    assert_same_bits(f4, f[:, ::-1], "reverse, flows")


# ------------------------------------------------------------------------------------
# 5. messages, not columns
# ------------------------------------------------------------------------------------
def test_lossy_stats_count_messages():
    g = tile_limit_graph()
    V = columns(g.n, 5, first=50)
    down = link_mask(g, 0.1, 6)
    with fu.CollectAllLossyBatch(g, V, loss=0.25, seed=3) as wide, fu.CollectAllLossy(g, V[:, 2], loss=0.25, seed=3) as one:
        for eng in (wide, one):
            eng.set_link_mask(down)
            eng.run(9)
        assert wide.stats == one.stats and wide.stats[0] == 8 * g.E and 0 < wide.stats[1] < wide.stats[0]
        assert_same_bits(wide.estimates()[:, 2], one.estimates())


def test_churn_stats_and_states_are_per_slot():
    g = tile_limit_graph()
    V = columns(g.n, 5, first=50)
    t1, t2 = random_masks(g, 0.2, 0.1, 61), random_masks(g, 0.1, 0.1, 62)
    with fu.CollectAllChurnBatch(g, V) as wide, fu.CollectAllChurn(g, V[:, 4]) as one:
        for t in (t1, t2):
            for eng in (wide, one):
                eng.run(2)
                eng.set_topology(*t)
            assert wide.stats == one.stats
            s = wide.slot_state()
            assert s.shape == (g.E,) and np.array_equal(s, one.slot_state())
        assert_same_bits(wide.flows()[:, 4], one.flows())


# ------------------------------------------------------------------------------------
# 6. the scaffold at width K
# ------------------------------------------------------------------------------------
def _pair(engine, g, V):
    if engine == "lossy":
        return [fu.CollectAllLossyBatch(g, V, loss=0.2, seed=5) for _ in range(2)]
    alive, up = random_masks(g, 0.15, 0.1, 9, keep=(tile_segment("heavy")[0],))
    out = [fu.CollectAllChurnBatch(g, V) for _ in range(2)]
    for eng in out:
        eng.set_topology(alive, up)
    return out


@pytest.mark.parametrize("engine", ["lossy", "churn"])
def test_split_runs_values_reset_and_timed_runs(engine):
    g = tile_limit_graph()
    V, V2 = columns(g.n, 3, first=60), columns(g.n, 3, first=70)
    a, b = _pair(engine, g, V)
    with a, b:
        a.run(17)
        b.run(5)
        b.run(12)
        assert_same_bits(a.estimates(), b.estimates(), "run(17) against run(5); run(12)")
        assert_same_bits(a.flows(), b.flows())
        # new (n, K) values mid-run, the state kept (against the Python rule: the next test)
        a.set_values(V2)
        a.run(2)
        b.set_values(V2)
        ms = b.run_timed(2)
        assert ms > 0.0 and b.rounds_done == 19
        assert_same_bits(a.estimates(), b.estimates(), "run against run_timed")
        # reset and rerun against a fresh handle
        a.reset()
        a.run(6)
        c, spare = _pair(engine, g, V2)
        with c, spare:
            c.run(6)
            assert_same_bits(a.estimates(), c.estimates(), "reset against a fresh handle")
            assert_same_bits(a.flows(), c.flows())


def test_set_values_mid_run_against_the_python_rule():
    """hub60-sized: lossy_python with inputs that change at round 6, per column."""
    from lossy_cases import hub60

    g = hub60()
    V, V2 = columns(g.n, 4, first=60), columns(g.n, 4, first=70)
    with fu.CollectAllLossyBatch(g, V, loss=0.3, seed=LOSS_SEED) as eng:
        eng.run(6)
        eng.set_values(V2)
        eng.run(5)
        for c in range(4):
            ra, rf = lossy_python(*g.arrays(), lambda r, c=c: (V if r < 6 else V2)[:, c], 11, hashed(0.3, LOSS_SEED, g.E))
            assert_same_bits(eng.estimates()[:, c], ra, ("estimates", c))
            assert_same_bits(eng.flows()[:, c], rf, ("flows", c))
    script = [("run", 6), ("values", V2), ("run", 5)]
    with fu.CollectAllChurnBatch(g, V) as eng:
        drive_churn(eng, script, churn_reference(g, V, script), ("churn",))


@pytest.mark.parametrize("engine", ["lossy", "churn"])
def test_error_trace_per_column(engine):
    """Targets = the estimates after the last round, column 1 shifted by 0.5, so the last check of
    column 0 is +0.0 and that of column 1 its shift; the wanted trace is numpy's max |a - target|
    over the estimates read back after every round of a first run. err_every 1 and 3; a NaN column raises only its own
    entries; under churn a dead decoy 2^20 off in column 0 does not enter."""
    g = tile_limit_graph()
    V = columns(g.n, 4, first=80)
    V[:, 3] = np.nan
    R = 6
    alive = np.ones(g.n, dtype=np.uint8)
    alive[[5, 300, 1500]] = 0

    def fresh():
        if engine == "lossy":
            return fu.CollectAllLossyBatch(g, V, loss=0.2, seed=5)
        eng = fu.CollectAllChurnBatch(g, V)
        eng.set_topology(alive)
        return eng

    with fresh() as eng:
        a_rounds = []
        for _ in range(R):
            eng.run(1)
            a_rounds.append(eng.estimates())
    tgt = a_rounds[-1].copy()
    tgt[:, 1] += 0.5
    tgt[:, 3] = 0.0
    on = np.ones(g.n, dtype=bool)
    if engine == "churn":
        on = alive != 0
        tgt[5, 0] += 2.0 ** 20  # a dead decoy
    want = np.stack([np.max(np.abs(a - tgt)[on], axis=0) for a in a_rounds])  # max propagates NaN
    assert np.isnan(want[:, 3]).all() and np.isfinite(want[:, :3]).all() and want[-1, 0] == 0.0
    assert abs(want[-1, 1] - 0.5) < 1e-9  # the shift, up to the rounding of a + 0.5
    assert (want[:, 0] < 2.0 ** 19).all()
    for every in (1, 3):
        with fresh() as eng:
            eng.set_targets(tgt)
            trace = eng.run(R, err_every=every)
            assert trace.shape == (R // every, 4)
            assert_same_bits(trace, want[every - 1::every], ("trace", every))
            assert_same_bits(eng.max_err(), want[-1], ("max_err", every))


@pytest.mark.parametrize("engine", ["lossy", "churn"])
def test_interleaved_with_a_scalar_handle(engine):
    g = tile_limit_graph()
    V = columns(g.n, 3, first=90)
    wide, alone = _pair(engine, g, V)
    if engine == "lossy":
        one = fu.CollectAllLossy(g, V[:, 1], loss=0.2, seed=5)
    else:
        one = fu.CollectAllChurn(g, V[:, 1])
        alive, up = random_masks(g, 0.15, 0.1, 9, keep=(tile_segment("heavy")[0],))
        one.set_topology(alive, up)
    with wide, alone, one:
        for _ in range(7):  # round-robin, one round each
            wide.run(1)
            one.run(1)
        alone.run(7)
        assert_same_bits(wide.estimates(), alone.estimates(), "interleaved against alone")
        assert_same_bits(wide.flows(), alone.flows())
        assert_same_bits(wide.estimates()[:, 1], one.estimates(), "the scalar handle's column")
        assert_same_bits(wide.flows()[:, 1], one.flows())


# ------------------------------------------------------------------------------------
# 7. a topology call before every round
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_round", [0, 1], ids=["even", "odd"])
def test_flapping_topology_at_four_columns(first_round):
    """flapping_case()'s column beside three others; started after `first_round` rounds so that
    the topology calls meet both buffer parities."""
    g, v, script, want = flapping_case()
    V = np.ascontiguousarray(np.stack([fu.uniform_values(g.n, seed=4), v, fu.uniform_values(g.n, seed=6), -v], axis=1))
    script = [("run", first_round)] + list(script) if first_round else list(script)
    steps = churn_reference(g, V, script)
    if not first_round:
        for q, s in enumerate(want.steps):  # the shared reference of the scalar flapping test
            assert_same_bits(steps[q].a[:, 1], s.a)
    with fu.CollectAllChurnBatch(g, V) as eng:
        drive_churn(eng, script, steps, ("flapping", first_round))


# ------------------------------------------------------------------------------------
# 8. degenerate shapes at K = 2
# ------------------------------------------------------------------------------------
def _empty(n):
    return np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32)


@pytest.mark.parametrize("engine", ["lossy", "churn"])
def test_degenerate_shapes(engine):
    cls = fu.CollectAllLossyBatch if engine == "lossy" else fu.CollectAllChurnBatch
    # one node: a = v from round 0 on; every readback with E = 0
    rp, col = _empty(1)
    V = np.array([[3.5, -2.0]])
    with cls(rowptr=rp, col=col, values=V) as eng:
        assert eng.flows().shape == (0, 2)
        assert_same_bits(eng.estimates(), np.zeros((1, 2)))
        eng.set_targets(V)
        trace = eng.run(3, err_every=1)
        assert_same_bits(eng.estimates(), V)
        assert_same_bits(trace, np.zeros((3, 2)))
        assert eng.flows().shape == (0, 2) and eng.rounds_done == 3
        assert eng.stats == ((0, 0) if engine == "lossy" else (1, 0))
        if engine == "churn":
            assert eng.slot_state().shape == (0,)
    # five isolated nodes, two of them dead (churn) / all firing (lossy)
    rp, col = _empty(5)
    V = columns(5, 2, first=3)
    with cls(rowptr=rp, col=col, values=V) as eng:
        want = V.copy()
        if engine == "churn":
            eng.set_topology(np.array([1, 0, 1, 0, 1], dtype=np.uint8))
            want[[1, 3]] = 0.0
            assert eng.stats == (3, 0)
        eng.run(2)
        assert_same_bits(eng.estimates(), want)
    # two nodes and one link
    rp, col, rev = np.array([0, 1, 2], dtype=np.int64), np.array([1, 0], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    V = columns(2, 2, first=5)
    with cls(rowptr=rp, col=col, rev=rev, values=V) as eng:
        eng.run(4)
        if engine == "lossy":
            ref = [lossy_python(rp, col, rev, V[:, c], 4, lambda r: np.ones(2, dtype=bool)) for c in range(2)]
            a, f = np.stack([x[0] for x in ref], axis=1), np.stack([x[1] for x in ref], axis=1)
        else:
            st = churn_reference(fu.Graph.from_edges(2, np.array([0]), np.array([1])), V, [("run", 4)])[0]
            a, f = st.a, st.f
            assert (eng.slot_state() == UP).all()
        assert_same_bits(eng.estimates(), a)
        assert_same_bits(eng.flows(), f)


def test_static_topology_is_ca_sync_on_the_live_subgraph():
    """A topology set before round 0 at K = 3: every column is the C oracle on the live subgraph."""
    g = tile_limit_graph()
    V = columns(g.n, 3, first=100)
    alive, up = random_masks(g, 0.2, 0.1, 3, keep=(tile_segment("heavy")[0],))
    with fu.CollectAllChurnBatch(g, V) as eng:
        eng.set_topology(alive, up)
        eng.run(6)
        a, f, s = eng.estimates(), eng.flows(), eng.slot_state()
    for c in range(3):
        check_static(g, alive, up, V[:, c], np.ascontiguousarray(a[:, c]), np.ascontiguousarray(f[:, c]), s, 6, ("column", c))
