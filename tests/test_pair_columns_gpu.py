"""fu.PairwiseSyncBatch (csrc/fu_pair.hip kp_exchange_cols and kp_heavy<Args, false>, lossless and lossy):
every column of a K-column run holds the bits of that column's own reference, which never runs
the engine: pair_cases.oracle_pair or pair_loss_cases.oracle_pair_loss (the C oracle's replay),
pair_loss_python where inputs and seeds change between runs, and the reference's value-domain
recordings. Every comparison is by bit pattern, on last averages, flows and caches; the
counters against the helpers' counts and a scalar handle's. The conditions that make the cases
meaningful are asserted in test_pair_columns_case_inputs.py."""
import numpy as np
import pytest

import fu
import vd_cases
from pair_cases import (CLASS_ROUNDS, LAST_SLOT_ROUNDS, LAST_SLOT_SEED, SEED, class_graph, dense66, oracle_pair, pair_count,
                        rr256_d8)
from pair_columns_cases import (BOUNDARY_ROUNDS, BOUNDARY_SEED, HEAVY_WIDTHS, LIGHT_WIDTHS, PARTIAL_CHUNK_RUNS, boundary_graph,
                                columns, ref_column, ref_column_loss)
from pair_loss_cases import (CLASS_P, LOSS_SEED, MASK_CLEARED_AT, fired_nodes, hashed, link_mask, loss_counts,
                             pair_loss_python)
from parity_util import assert_same_bits

pytestmark = pytest.mark.gpu

MATCHERS = [0, 1]


def _check(eng, refs, what):
    """refs[c] = (last, f, c) of column c."""
    est, fl, ca = eng.estimates(), eng.flows(), eng.cache()
    K = len(refs)
    assert est.shape == (eng.n, K) and fl.shape == (eng.E, K) and ca.shape == (eng.E, K), what
    for c, ref in enumerate(refs):
        assert_same_bits(est[:, c], ref[0], what + ("column", c, "last"))
        assert_same_bits(fl[:, c], ref[1], what + ("column", c, "flows"))
        assert_same_bits(ca[:, c], ref[2], what + ("column", c, "cache"))


def _refs(g, V, rounds, seed):
    return [ref_column(g, V[:, c], rounds, seed) for c in range(V.shape[1])]


def _refs_loss(g, V, rounds, seed, lost, tag):
    return [ref_column_loss(g, V[:, c], rounds, seed, lost, tag) for c in range(V.shape[1])]


def _columns_of(eng):
    from fu import _lib as L

    k = L.i32(0)
    L.call("fu_pair_get_columns", eng._h, k)
    return int(k.value)


# ------------------------------------------------------------------------------------
# 1. every width in the lane groups
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", LIGHT_WIDTHS)
def test_every_width_on_light_pairs(K):
    g = rr256_d8()
    V = columns(g.n, K)
    with fu.PairwiseSyncBatch(g, V, seed=SEED) as eng, fu.PairwiseSync(g, V[:, 0].copy(), seed=SEED) as one:
        assert _columns_of(eng) == K and eng.K == K and _columns_of(one) == 1
        for r in (1, 5, 40):
            eng.run(r - eng.rounds_done)
            _check(eng, _refs(g, V, r, SEED), ("K", K, "round", r))
        one.run(40)
        assert eng.stats == one.stats and eng.stats[0] == pair_count(*g.arrays(), SEED, 40)
        assert eng.loss_stats == one.loss_stats == (0, 0, eng.stats[0])
        assert eng.rounds_done == 40


# ------------------------------------------------------------------------------------
# 2. heavy pairs: the degree classes, the last slot, more pairs than blocks, the chunk edges
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("match", MATCHERS)
@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_every_degree_class(K, match):
    g = class_graph()
    V = columns(g.n, K)
    with fu.PairwiseSyncBatch(g, V, seed=SEED) as eng:
        eng.set_option("match", match)
        for r in (2, CLASS_ROUNDS):
            eng.run(r - eng.rounds_done)
            _check(eng, _refs(g, V, r, SEED), ("K", K, "match", match, "round", r))
        assert eng.stats[0] == pair_count(*g.arrays(), SEED, CLASS_ROUNDS)


@pytest.mark.parametrize("match", MATCHERS)
@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_listener_on_the_last_slot_of_the_hub(K, match):
    g = class_graph()
    V = columns(g.n, K)
    with fu.PairwiseSyncBatch(g, V, seed=LAST_SLOT_SEED) as eng:
        eng.set_option("match", match)
        eng.run(LAST_SLOT_ROUNDS)
        _check(eng, _refs(g, V, LAST_SLOT_ROUNDS, LAST_SLOT_SEED), ("K", K, "match", match))


@pytest.mark.parametrize("match", MATCHERS)
@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_more_heavy_pairs_than_blocks(K, match):
    g = dense66()
    V = columns(g.n, K)
    with fu.PairwiseSyncBatch(g, V, seed=SEED) as eng:
        eng.set_option("match", match)
        eng.run(3)
        _check(eng, _refs(g, V, 3, SEED), ("K", K, "match", match))
        assert eng.stats[0] == pair_count(*g.arrays(), SEED, 3) > 3 * 1024


@pytest.mark.parametrize("match", MATCHERS)
@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_the_chunk_edges_of_this_width(K, match):
    g = boundary_graph(K)
    V = columns(g.n, K)
    seed = BOUNDARY_SEED[K]
    with fu.PairwiseSyncBatch(g, V, seed=seed) as eng:
        eng.set_option("match", match)
        for r in (3, BOUNDARY_ROUNDS):
            eng.run(r - eng.rounds_done)
            _check(eng, _refs(g, V, r, seed), ("K", K, "match", match, "round", r))
        for _, s, rounds in PARTIAL_CHUNK_RUNS[K]:  # a pair on the final partial chunk of a row
            eng.set_seed(s)
            eng.reset()
            eng.run(rounds)
            _check(eng, _refs(g, V, rounds, s), ("K", K, "match", match, "seed", s))


# ------------------------------------------------------------------------------------
# 3. one column through the K-column entry points is the scalar handle
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lossy", [False, True])
@pytest.mark.parametrize("graph", [rr256_d8, class_graph])
def test_one_column_is_the_scalar_handle(graph, lossy):
    g = graph()
    v = fu.uniform_values(g.n, seed=3)
    kw = dict(seed=SEED, loss=CLASS_P, loss_seed=LOSS_SEED, link_mask=link_mask(g)) if lossy else dict(seed=SEED)
    with fu.PairwiseSync(g, v, **kw) as one, fu.PairwiseSyncBatch(g, v.reshape(-1, 1), **kw) as eng:
        assert _columns_of(eng) == 1
        for r in (1, 7, CLASS_ROUNDS):
            one.run(r - one.rounds_done)
            eng.run(r - eng.rounds_done)
            _check(eng, [(one.estimates(), one.flows(), one.cache())], (graph.__name__, lossy, "round", r))
            assert eng.stats == one.stats and eng.loss_stats == one.loss_stats
        if not lossy:
            _check(eng, [oracle_pair(*g.arrays(), v, CLASS_ROUNDS, SEED)[:3]], (graph.__name__, "oracle"))
        else:
            assert min(eng.loss_stats) > 0


# ------------------------------------------------------------------------------------
# 4. loss and a link mask
# ------------------------------------------------------------------------------------
def _check_counts(eng, g, seed, rounds, lost, what):
    m1, m2, full = loss_counts(*g.arrays(), seed, rounds, lost)
    assert eng.loss_stats == (m1, m2, full), what
    assert eng.stats == (m1 + m2 + full, g.n - len(fired_nodes(*g.arrays(), seed, rounds, lost))), what


@pytest.mark.parametrize("match", MATCHERS)
@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_loss_at_the_chunk_edges(K, match):
    g = boundary_graph(K)
    V = columns(g.n, K)
    seed = BOUNDARY_SEED[K]
    lost = hashed(CLASS_P, LOSS_SEED, g.E)
    with fu.PairwiseSyncBatch(g, V, seed=seed, loss=CLASS_P, loss_seed=LOSS_SEED) as eng:
        eng.set_option("match", match)
        for r in (2, BOUNDARY_ROUNDS):
            eng.run(r - eng.rounds_done)
            _check(eng, _refs_loss(g, V, r, seed, lost, "p"), ("K", K, "match", match, "round", r))
        _check_counts(eng, g, seed, BOUNDARY_ROUNDS, lost, (K, match))


@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_mask_set_then_cleared_mid_run(K):
    g = class_graph()
    V = columns(g.n, K)
    down = link_mask(g)
    lost = hashed(CLASS_P, LOSS_SEED, g.E, lambda r: down if r < MASK_CLEARED_AT else None)
    with fu.PairwiseSyncBatch(g, V, seed=SEED, loss=CLASS_P, loss_seed=LOSS_SEED, link_mask=down) as eng:
        eng.run(MASK_CLEARED_AT)
        _check(eng, _refs_loss(g, V, MASK_CLEARED_AT, SEED, lost, "p+mask"), ("K", K, "masked"))
        _check_counts(eng, g, SEED, MASK_CLEARED_AT, lost, (K, "masked"))
        eng.set_link_mask(None)
        eng.run(CLASS_ROUNDS - MASK_CLEARED_AT)
        _check(eng, _refs_loss(g, V, CLASS_ROUNDS, SEED, lost, "p+mask"), ("K", K, "cleared"))
        _check_counts(eng, g, SEED, CLASS_ROUNDS, lost, (K, "cleared"))


@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_loss_with_more_heavy_pairs_than_blocks(K):
    g = dense66()
    V = columns(g.n, K)
    lost = hashed(CLASS_P, LOSS_SEED, g.E)
    with fu.PairwiseSyncBatch(g, V, seed=SEED, loss=CLASS_P, loss_seed=LOSS_SEED) as eng:
        eng.run(3)
        _check(eng, _refs_loss(g, V, 3, SEED, lost, "p"), ("K", K))
        _check_counts(eng, g, SEED, 3, lost, K)


# ------------------------------------------------------------------------------------
# 5. splits and switches
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_split_run_equals_one_run(K):
    g = class_graph()
    V = columns(g.n, K)
    lost = hashed(CLASS_P, LOSS_SEED, g.E)
    kw = dict(seed=SEED, loss=CLASS_P, loss_seed=LOSS_SEED)
    with fu.PairwiseSyncBatch(g, V, **kw) as one, fu.PairwiseSyncBatch(g, V, **kw) as two:
        one.run(17)
        two.run(5)
        two.run(12)
        refs = _refs_loss(g, V, 17, SEED, lost, "p")
        _check(one, refs, ("K", K, "run(17)"))
        _check(two, refs, ("K", K, "run(5); run(12)"))
        assert one.loss_stats == two.loss_stats == loss_counts(*g.arrays(), SEED, 17, lost)


@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_values_seeds_and_loss_change_between_runs_then_reset(K):
    """Rounds 0-4 at (p, loss seed, matching seed) = (0.3, 5, 11), 5-9 at (0.6, 8, 11) with new
    values, 10-13 at (0.0, 8, 4) under a mask; reset() keeps the last settings and zeroes state and
    counters, so the rerun equals the oracle's run under them."""
    g = rr256_d8()
    Vs = [columns(g.n, K, seed=s) for s in (40, 70)]
    down = link_mask(g, seed=2)
    p = lambda r: 0.3 if r < 5 else 0.6 if r < 10 else 0.0  # noqa: E731
    ls = lambda r: 5 if r < 5 else 8  # noqa: E731
    ms = lambda r: 11 if r < 10 else 4  # noqa: E731
    lost = hashed(p, ls, g.E, lambda r: None if r < 10 else down)
    refs = [pair_loss_python(*g.arrays(), lambda r, c=c: (Vs[0] if r < 5 else Vs[1])[:, c], 14, ms, lost) for c in range(K)]
    with fu.PairwiseSyncBatch(g, Vs[0], seed=11, loss=0.3, loss_seed=5) as eng:
        eng.run(5)
        eng.set_loss(0.6, 8)
        eng.set_values(Vs[1])
        eng.run(5)
        eng.set_loss(0.0, 8)
        eng.set_seed(4)
        eng.set_link_mask(down)
        eng.run(4)
        _check(eng, refs, ("K", K, "three settings"))
        assert eng.loss_stats == loss_counts(*g.arrays(), ms, 14, lost)
        eng.reset()
        assert eng.rounds_done == 0 and eng.stats == (0, g.n) and eng.loss_stats == (0, 0, 0)
        assert not eng.estimates().any() and not eng.flows().any() and not eng.cache().any()
        eng.run(12)
        kept = hashed(0.0, 8, g.E, down)
        _check(eng, _refs_loss(g, Vs[1], 12, 4, kept, "mask, seed 8"), ("K", K, "after reset"))
        _check_counts(eng, g, 4, 12, kept, (K, "after reset"))


# ------------------------------------------------------------------------------------
# 6. the error reduction per column
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 16])
def test_max_err_and_trace_per_column(K):
    """class_graph: n * K elements span many blocks of the reduction. Every entry is the maximum
    recomputed on the host from estimates(), per column, before round 0 as well."""
    g = class_graph()
    V = columns(g.n, K)
    T = np.ascontiguousarray(np.stack([fu.component_means(g.rowptr, g.col, V[:, c].copy())[0] for c in range(K)], axis=1))
    T[7, K - 1] += 1e6 * 8.0 ** K  # one far target: the last column's entry comes from one element
    host = lambda eng: np.max(np.abs(eng.estimates() - T), axis=0)  # noqa: E731
    with fu.PairwiseSyncBatch(g, V, seed=SEED) as eng, fu.PairwiseSyncBatch(g, V, seed=SEED) as whole:
        eng.set_targets(T)
        whole.set_targets(T)
        e0 = eng.max_err()
        assert e0.shape == (K,)
        assert_same_bits(e0, np.max(np.abs(T), axis=0), ("K", K, "before round 0"))
        rows = []
        for _ in range(3):
            tr = eng.run(4, err_every=4)
            assert tr.shape == (1, K)
            assert_same_bits(tr[0], host(eng), ("K", K, "trace after", eng.rounds_done))
            assert_same_bits(eng.max_err(), host(eng), ("K", K, "max_err after", eng.rounds_done))
            rows.append(tr[0])
        tr = whole.run(12, err_every=4)
        assert tr.shape == (3, K)
        assert_same_bits(tr, np.stack(rows), ("K", K, "one run, three checks"))
        assert len({x.tobytes() for x in np.stack(rows).T}) == K  # the columns' entries differ


# ------------------------------------------------------------------------------------
# 7. the fp64 value domain beside finite columns
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", ["first", "last"])
@pytest.mark.parametrize("K", HEAVY_WIDTHS)
@pytest.mark.parametrize("family", vd_cases.RULE_FAMILIES)
def test_value_domain_column_beside_finite_columns(family, K, place):
    """The reference's recording (signed zeros and subnormals, or NaN and infinities) as one
    column: it comes out as recorded, NaN exactly where the recording has it, and every filler
    column holds the bits of its own oracle run."""
    d, g = vd_cases.rule("pair", family)
    n = len(d.values)
    fill = columns(n, K - 1, seed=90)
    at = 0 if place == "first" else K - 1
    V = np.ascontiguousarray(np.insert(fill, at, d.values, axis=1))
    assert V.shape == (n, K) and np.isfinite(fill).all()
    with fu.PairwiseSyncBatch(rowptr=g.rowptr, col=g.col, rev=g.rev, values=V, seed=g.seed) as eng:
        for q, stop in enumerate(g.stops):
            eng.run(stop - eng.rounds_done)
            refs = [oracle_pair(g.rowptr, g.col, g.rev, fill[:, c].copy(), stop, g.seed)[:3] for c in range(K - 1)]
            refs.insert(at, (d.last_avg[q], d.flows[q], d.estimates[q]))
            _check(eng, refs, (family, "K", K, place, "after", stop))
        if family == "special":
            assert np.isnan(eng.estimates()[:, at]).any()
        assert np.isfinite(np.delete(eng.estimates(), at, axis=1)).all()


# ------------------------------------------------------------------------------------
# 8. the command line
# ------------------------------------------------------------------------------------
def test_cli_bench_graph_with_pair_columns(capsys):
    from fu.__main__ import main

    argv = ["bench-graph", "er:n=2000,m=8000", "--rounds", "6", "--pairs", "--pair-seed", "4", "--pair-columns", "3"]
    assert main(argv) == 0
    line = capsys.readouterr().out.strip()
    g = fu.Graph.from_spec("er:n=2000,m=8000", seed=1)
    assert line.startswith(f"graph n={g.n} E={g.E} ") and " rounds=6 " in line
    assert line.endswith(f" pairs={pair_count(*g.arrays(), 4, 6)} columns=3")
    assert main(argv + ["--loss", "0.3", "--loss-seed", "9"]) == 0
    line = capsys.readouterr().out.strip()
    m1, m2, _ = loss_counts(*g.arrays(), 4, 6, hashed(0.3, 9, g.E))
    assert line.endswith(f" pairs={pair_count(*g.arrays(), 4, 6)} lost={m1 + m2} columns=3")
