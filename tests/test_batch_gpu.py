"""GPU parity of the batched collect-all engine (fu.CollectAllBatch, csrc/fu_batch.hip): K
value columns over one graph in one pass per round. The columns are independent scalar
runs, so every expected value comes from the C oracle called once per column
(coracle.ca_sync / ca_rounds) or from the golden fixtures, and every comparison is by bit
pattern (parity_util.assert_same_bits). The engine is never compared with itself.

The references are computed once and shared by the cases; no case changes them."""
import functools

import numpy as np
import pytest

import coracle
import fu
import oracle
from conftest import ca_sync_fixtures, load_npz
from parity_util import (FAMILIES, _batch_boundary_graph, _class_edge_graph, _width_graph, assert_same_bits,
                         count_neg_zero)

pytestmark = pytest.mark.gpu


def _oracle_stops(g_arrays, v, stops):
    """{r: (a, f)} after r rounds from zero for each r of the ascending `stops`."""
    refs, done = {}, 0
    a = f = None
    for r in stops:
        if a is None:
            a, f = coracle.ca_sync(*g_arrays, v, r, nthreads=16)
        else:
            coracle.ca_rounds(*g_arrays, v, r - done, a, f, nthreads=16)
        done = r
        refs[r] = (a.copy(), f.copy())
    return refs


def _check_columns(eng, refs_by_column, r, what):
    """Column c of the engine's estimates and flows against refs_by_column[c][r]."""
    a, f = eng.estimates(), eng.flows()
    assert a.shape == (eng.n, eng.K) and f.shape == (eng.E, eng.K)
    for c, refs in enumerate(refs_by_column):
        assert_same_bits(np.ascontiguousarray(a[:, c]), refs[r][0], what + (r, "column", c, "estimates"))
        assert_same_bits(np.ascontiguousarray(f[:, c]), refs[r][1], what + (r, "column", c, "flows"))


# ------------------------------------------------------------------------------------
# 1. golden fixtures
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,meta", ca_sync_fixtures())
def test_fixtures_in_the_middle_column(name, meta):
    """Every ca_sync fixture at K = 3 with its own values in column 1: that column equals the
    recorded last_avg and flows at every recorded round, and its neighbours (`sym`, `ints`)
    equal the oracle."""
    d = load_npz(meta["file"])
    rp, col = d["rowptr"], d["col"]
    rev = oracle.build_rev(rp, col)
    n = len(rp) - 1
    stops = [int(r) + 1 for r in d["rounds"]]
    sides = [FAMILIES["sym"](n, seed=1), FAMILIES["ints"](n, seed=2)]
    side_refs = [_oracle_stops((rp, col, rev), v, stops) for v in sides]
    eng = fu.CollectAllBatch(rowptr=rp, col=col, values=np.stack([sides[0], d["values"], sides[1]], axis=1))
    done = 0
    for k, r in enumerate(stops):
        eng.run(r - done)
        done = r
        assert eng.rounds_done == r
        fixture = {r: (np.ascontiguousarray(d["last_avg"][k], dtype=np.float64),
                       np.ascontiguousarray(d["flows"][k], dtype=np.float64))}
        _check_columns(eng, [side_refs[0], fixture, side_refs[1]], r, (name,))
    eng.close()


# ------------------------------------------------------------------------------------
# 2. row classes and column independence
# ------------------------------------------------------------------------------------
CLASS_STOPS = (1, 3, 8, 17)
CLASS_COLUMNS = sorted(FAMILIES) + ["uniform"]  # K = 8


@functools.lru_cache(maxsize=None)
def _class_graph():
    return _class_edge_graph(7)


@functools.lru_cache(maxsize=None)
def _class_refs(column):
    g = _class_graph()
    v = fu.uniform_values(g.n, seed=3) if column == "uniform" else FAMILIES[column](g.n, seed=3)
    return v, _oracle_stops(g.arrays(), v, CLASS_STOPS)


def test_row_class_inputs_reach_the_edges():
    """A condition on the inputs of the case below, from the oracle alone: `subn` reaches -0.0
    in estimates and flows, `huge` reaches both infinities and NaN."""
    _, refs = _class_refs("subn")
    assert count_neg_zero(refs[17][0]) > 0 and count_neg_zero(refs[17][1]) > 0
    _, refs = _class_refs("huge")
    f3, a17 = refs[3][1], refs[17][0]
    assert np.isposinf(f3).any() and np.isneginf(f3).any() and np.isnan(a17).any()
    for column in CLASS_COLUMNS:  # and nowhere else: a non-finite value in another column is a leak
        if column != "huge":
            _, refs = _class_refs(column)
            assert all(np.isfinite(refs[r][0]).all() and np.isfinite(refs[r][1]).all() for r in CLASS_STOPS)


def test_row_classes_eight_value_families_side_by_side():
    """Rows of every degree class (0 ... 12000, one star per class edge: register rows, the
    longer light rows and the block-per-row rows) with the seven value families and uniform
    values as the eight columns of one handle, after 1, 3, 8 and 17 rounds. `huge` overflows
    to +-inf and NaN in its own column only; `subn` produces -0.0."""
    g = _class_graph()
    cols = [_class_refs(c) for c in CLASS_COLUMNS]
    eng = fu.CollectAllBatch(g, np.stack([v for v, _ in cols], axis=1))
    done = 0
    for r in CLASS_STOPS:
        eng.run(r - done)
        done = r
        _check_columns(eng, [refs for _, refs in cols], r, ("classes",))
    a = eng.estimates()
    huge = CLASS_COLUMNS.index("huge")
    assert np.isnan(a[:, huge]).any() and np.isfinite(np.delete(a, huge, axis=1)).all()
    assert count_neg_zero(np.ascontiguousarray(a[:, CLASS_COLUMNS.index("subn")])) > 0
    eng.close()


# ------------------------------------------------------------------------------------
# 3. widths
# ------------------------------------------------------------------------------------
WIDTH_ROUNDS = 40


@functools.lru_cache(maxsize=None)
def _width_refs(c):
    """Column c of every width: uniform values for even c, 36 decades of both signs for odd c."""
    g = _width_graph()
    v = fu.uniform_values(g.n, seed=c) if c % 2 == 0 else FAMILIES["wide"](g.n, seed=c)
    return v, _oracle_stops(g.arrays(), v, (WIDTH_ROUNDS,))


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8, 16])
def test_every_width_each_column_equals_its_oracle_run(K):
    g = _width_graph()
    cols = [_width_refs(c) for c in range(K)]
    eng = fu.CollectAllBatch(g, np.stack([v for v, _ in cols], axis=1))
    eng.run(WIDTH_ROUNDS)
    _check_columns(eng, [refs for _, refs in cols], WIDTH_ROUNDS, ("width", K))
    eng.close()
    if K == 1:  # and the scalar engine computes the same (both against the oracle)
        v, refs = cols[0]
        one = fu.CollectAll(g, v)
        one.run(WIDTH_ROUNDS)
        assert_same_bits(one.estimates(), refs[WIDTH_ROUNDS][0], "CollectAll estimates")
        assert_same_bits(one.flows(), refs[WIDTH_ROUNDS][1], "CollectAll flows")
        one.close()


# ------------------------------------------------------------------------------------
# 3b. every width against every chunk edge and register boundary
# ------------------------------------------------------------------------------------
BOUNDARY_STOPS = (1, 2, 3, 4, 7)
# Sixteen columns, fixed once; a handle of width K takes the first K. `huge` is left out: its
# NaNs would hide a difference.
BOUNDARY_COLUMNS = [("uniform", "wide", "sym", "subn", "neg", "ints", "binade")[c % 7] for c in range(16)]


@functools.lru_cache(maxsize=None)
def _boundary_refs(c):
    g = _batch_boundary_graph()
    name = BOUNDARY_COLUMNS[c]
    v = fu.uniform_values(g.n, seed=40 + c) if name == "uniform" else FAMILIES[name](g.n, seed=40 + c)
    return v, _oracle_stops(g.arrays(), v, BOUNDARY_STOPS)


@pytest.mark.parametrize("K", range(1, 17))
def test_every_width_on_its_chunk_edges(K):
    """parity_util._batch_boundary_graph(): heavy rows of ce - 1, ce, ce + 1, 2 ce - 1, 2 ce and
    2 ce + 1 edges for the chunk ce = 2048 // K of every width (the widths that do not divide
    2048 included), and light rows on both sides of every group of four, of the register limit
    and of the heavy limit. Round 1 alone materialises f_0 on demand, rounds 2 and 3 compute
    the old flows without reading them, round 4 is the first to read the other flow buffer;
    then reset() and three rounds again."""
    g = _batch_boundary_graph()
    cols = [_boundary_refs(c) for c in range(K)]
    refs = [r for _, r in cols]
    eng = fu.CollectAllBatch(g, np.stack([v for v, _ in cols], axis=1))
    for r in BOUNDARY_STOPS:
        eng.run(r - eng.rounds_done)
        _check_columns(eng, refs, r, ("K", K))
    eng.reset()
    assert eng.rounds_done == 0
    eng.run(3)
    _check_columns(eng, refs, 3, ("K", K, "after reset"))
    eng.close()


# ------------------------------------------------------------------------------------
# 4. first rounds and reset
# ------------------------------------------------------------------------------------
def test_first_rounds_flows_each_round_and_reset():
    """Round 0 writes no flows and rounds 1 and 2 compute the old flows without reading them:
    the flows are all +0.0 before any round, and estimates and flows equal the oracle after
    each of rounds 1-5 (f_0 materialised on demand), also after a reset."""
    g = fu.Graph.rmat(12, 16, seed=4)
    assert g.max_deg > 64  # block-per-row rows too
    vs = [fu.uniform_values(g.n, seed=4), FAMILIES["sym"](g.n, seed=5), FAMILIES["subn"](g.n, seed=6),
          FAMILIES["wide"](g.n, seed=7)]
    refs = [_oracle_stops(g.arrays(), v, (1, 2, 3, 4, 5)) for v in vs]
    eng = fu.CollectAllBatch(g, np.stack(vs, axis=1))
    for attempt in range(2):
        assert eng.rounds_done == 0
        assert_same_bits(eng.flows(), np.zeros((g.E, 4)), ("before any round", attempt))
        for r in range(1, 6):
            eng.run(1)
            _check_columns(eng, refs, r, ("first rounds", attempt))
        eng.reset()
    eng.close()


# ------------------------------------------------------------------------------------
# 5. split invariance
# ------------------------------------------------------------------------------------
def test_split_runs_equal_one_run_through_the_oracle():
    """run(3); run(5) and run(8) both equal the oracle at round 8 (so they equal each other)."""
    g = fu.Graph.erdos_renyi(6_000, 24_000, seed=23)
    vs = [FAMILIES["neg"](g.n, seed=1), fu.uniform_values(g.n, seed=2), FAMILIES["binade"](g.n, seed=3)]
    refs = [_oracle_stops(g.arrays(), v, (8,)) for v in vs]
    split = fu.CollectAllBatch(g, np.stack(vs, axis=1))
    split.run(3)
    split.run(5)
    whole = fu.CollectAllBatch(g, np.stack(vs, axis=1))
    whole.run(8)
    for eng, what in ((split, "3 + 5"), (whole, "8")):
        assert eng.rounds_done == 8
        _check_columns(eng, refs, 8, (what,))
        eng.close()


# ------------------------------------------------------------------------------------
# 6. degenerate shapes
# ------------------------------------------------------------------------------------
def _check_csr(rp, col, rev, vs, rounds, what):
    refs = [{rounds: coracle.ca_sync(rp, col, rev, v, rounds)} for v in vs]
    eng = fu.CollectAllBatch(rowptr=rp, col=col, rev=rev, values=np.stack(vs, axis=1))
    eng.run(rounds)
    _check_columns(eng, refs, rounds, (what,))
    a = eng.estimates()
    eng.close()
    return a


def test_isolated_rows_signed_zero_and_subnormal():
    rp = np.array([0, 0, 1, 2, 2], dtype=np.int64)
    col = np.array([2, 1], dtype=np.int32)
    vs = [np.array([3.5, -0.0, 7.0, 1e-310]), np.array([-0.0, 5e-324, -5e-324, -0.0])]
    a = _check_csr(rp, col, np.array([1, 0], dtype=np.int32), vs, 5, "four nodes")
    assert a[3, 0] == 1e-310 and a[0, 0] == 3.5


def test_no_edges_and_one_node():
    no_col, no_rev = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    rp = np.zeros(6, dtype=np.int64)
    vs = [np.array([1.0, -2.5, 0.0, 1e300, 5e-324]), np.arange(5, dtype=np.float64)]
    _check_csr(rp, no_col, no_rev, vs, 4, "E = 0")
    _check_csr(np.zeros(2, dtype=np.int64), no_col, no_rev, [np.array([42.0]), np.array([-1e-310])], 3, "n = 1")


def test_sizes_off_every_tile():
    g = fu.Graph.random_regular(4098, 5, seed=11)
    vs = [fu.uniform_values(g.n, seed=c) for c in range(3)]
    _check_csr(g.rowptr, g.col, g.rev, vs, 12, "RR(4098, 5)")


# ------------------------------------------------------------------------------------
# 7. errors
# ------------------------------------------------------------------------------------
ERR_ROUNDS = 400


@functools.lru_cache(maxsize=None)
def _err_refs():
    g = fu.Graph.random_regular(4096, 8, seed=1)
    vs = [fu.uniform_values(g.n, seed=c) for c in range(2)]
    tgt = np.stack([fu.component_means(g.rowptr, g.col, v)[0] for v in vs], axis=1)
    trace = np.empty((ERR_ROUNDS, 2))
    last = []
    for c, v in enumerate(vs):
        a, f = coracle.ca_sync(*g.arrays(), v, 1)
        for r in range(ERR_ROUNDS):
            if r:
                coracle.ca_rounds(*g.arrays(), v, 1, a, f)
            trace[r, c] = np.max(np.abs(a - tgt[:, c]))
        last.append(a)
    return g, vs, tgt, trace, np.stack(last, axis=1)


def test_error_trace_and_max_err_per_column():
    """run(400, err_every=1) gives a (400, 2) trace whose every row is the oracle's
    max |a - target| per column; the last row is that of the engine's own estimates and
    equals max_err()."""
    g, vs, tgt, want, a_last = _err_refs()
    eng = fu.CollectAllBatch(g, np.stack(vs, axis=1))
    eng.set_targets(tgt)
    tr = eng.run(ERR_ROUNDS, err_every=1)
    assert tr.shape == (ERR_ROUNDS, 2)
    assert_same_bits(tr, want, "trace")
    est = eng.estimates()
    assert_same_bits(est, a_last, "estimates")
    assert_same_bits(tr[-1], np.max(np.abs(est - tgt), axis=0), "last row")
    assert_same_bits(eng.max_err(), want[-1], "max_err")
    assert eng.max_err().shape == (2,)
    assert eng.run(10, err_every=4).shape == (2, 2)
    eng.close()


def test_nan_stays_in_its_column():
    g, vs, tgt, want, _ = _err_refs()
    v1 = vs[1].copy()
    v1[17] = np.nan
    eng = fu.CollectAllBatch(g, np.stack([vs[0], v1], axis=1))
    eng.set_targets(tgt)
    tr = eng.run(ERR_ROUNDS, err_every=1)
    assert np.isnan(tr[:, 1]).all()
    assert_same_bits(np.ascontiguousarray(tr[:, 0]), np.ascontiguousarray(want[:, 0]), "column 0 beside the NaN")
    m = eng.max_err()
    assert np.isnan(m[1])
    assert_same_bits(m[:1], want[-1, :1], "max_err column 0")
    eng.close()
