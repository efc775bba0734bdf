"""fu.PairwiseSync (csrc/fu_pair.hip) against restatements that do not run it: the C oracle's
replay of a synthetic FIRE_PW / RECV trace (pair_cases.oracle_pair), and Python floats where the
inputs change. Every comparison is by bit pattern, on last averages, flows and caches.

The kernels' boundaries: a pair with a row above 64 slots leaves the 8-lane groups for one block
per pair, which stages rows in chunks of 1024 slots. pair_cases.class_graph() has star centres
of degrees 0, 1, 2, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025 and 2500."""
import functools

import numpy as np
import pytest

import fu
from lossy_cases import hub60
from pair_cases import (BOUNDARY_DEGREES, CLASS_DEGREES, CLASS_ROUNDS, LAST_SLOT_ROUNDS, LAST_SLOT_SEED, SEED, class_graph,
                        dense66, oracle_pair, pair_count, pair_python, roles, rr256_d8)
from parity_util import FAMILIES, assert_same_bits, count_neg_zero

pytestmark = pytest.mark.gpu

MATCHERS = [0, 1]  # fu_pair_set_option "match": proposers push / listeners scan


def _check(eng, ref, what):
    assert_same_bits(eng.estimates(), ref[0], what + ("last",))
    assert_same_bits(eng.flows(), ref[1], what + ("flows",))
    assert_same_bits(eng.cache(), ref[2], what + ("cache",))


def _nan_inf(n, seed):
    """Uniform values with one quiet NaN and one inf among them."""
    v = np.random.default_rng(seed).random(n)
    v[n // 3] = np.nan
    v[2 * n // 3] = np.inf
    return v


def _values(family, n):
    if family == "uniform":
        return fu.uniform_values(n, seed=3)
    v = (_nan_inf if family == "nan_inf" else FAMILIES[family])(n, seed=3)
    v[::7] = -0.0
    return v


@functools.lru_cache(maxsize=None)
def _class_ref(family, rounds, snaps=()):
    g = class_graph()
    return oracle_pair(*g.arrays(), _values(family, g.n), rounds, SEED, snaps=snaps)


# ------------------------------------------------------------------------------------
# 1. small graphs, round by round
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("match", MATCHERS)
def test_rr256_round_by_round_then_64(match):
    g = rr256_d8()
    v = fu.uniform_values(g.n, seed=0)
    with fu.PairwiseSync(g, v, seed=SEED) as eng:
        eng.set_option("match", match)
        for r in range(1, 9):
            eng.run(1)
            _check(eng, oracle_pair(*g.arrays(), v, r, SEED), ("round", r))
        eng.run(56)
        assert eng.rounds_done == 64
        _check(eng, oracle_pair(*g.arrays(), v, 64, SEED), ("round", 64))
        assert eng.stats[0] == pair_count(*g.arrays(), SEED, 64)


@pytest.mark.parametrize("match", MATCHERS)
def test_hub60(match):
    g = hub60()
    v = fu.uniform_values(g.n, seed=4)
    with fu.PairwiseSync(rowptr=g.rowptr, col=g.col, values=v, seed=SEED) as eng:  # rev built natively
        eng.set_option("match", match)
        for r in (1, 2, 30):
            eng.run(r - eng.rounds_done)
            _check(eng, oracle_pair(*g.arrays(), v, r, SEED), ("round", r))
    with fu.PairwiseSync(rowptr=g.rowptr, col=g.col, rev=g.rev, values=v, seed=SEED) as eng:  # the caller's rev
        eng.run(30)
        _check(eng, oracle_pair(*g.arrays(), v, 30, SEED), ("caller's rev",))


# ------------------------------------------------------------------------------------
# 2. every degree boundary
# ------------------------------------------------------------------------------------
def test_boundary_rows_take_both_roles():
    """A condition on the cases below, from the helper's matching alone: within CLASS_ROUNDS
    rounds every centre of degree >= 1 is matched, and those on either side of a boundary are
    initiator at least once and listener at least once."""
    g = class_graph()
    ini, lis = roles(*g.arrays(), SEED, CLASS_ROUNDS)
    for c, d in enumerate(CLASS_DEGREES):
        if d >= 1:
            assert c in ini or c in lis, d
        if d in BOUNDARY_DEGREES or d in (63, 1023, 2500):
            assert c in ini and c in lis, d


@pytest.mark.parametrize("match", MATCHERS)
def test_every_degree_boundary(match):
    g = class_graph()
    with fu.PairwiseSync(g, _values("uniform", g.n), seed=SEED) as eng:
        eng.set_option("match", match)
        for r in (1, 2, 7, CLASS_ROUNDS):
            eng.run(r - eng.rounds_done)
            _check(eng, _class_ref("uniform", r), ("match", match, "round", r))
        pairs = pair_count(*g.arrays(), SEED, CLASS_ROUNDS)
        never = g.n - len(set().union(*roles(*g.arrays(), SEED, CLASS_ROUNDS)))
        assert eng.stats == (pairs, never)
        assert never >= 1  # the centre of degree 0


# ------------------------------------------------------------------------------------
# 3. the fp64 value domain
# ------------------------------------------------------------------------------------
def test_value_domain_inputs_reach_the_edges():
    """From the oracle alone: `subn` reaches -0.0 in last averages and flows, `huge` reaches an
    infinity and NaN, `nan_inf` spreads its NaN while most nodes stay finite."""
    last, f, _, _ = _class_ref("subn", CLASS_ROUNDS)
    assert count_neg_zero(last) > 0 and count_neg_zero(f) > 0
    last, f, _, _ = _class_ref("huge", CLASS_ROUNDS)
    assert np.isinf(f).any() and np.isnan(last).any()
    last, _, _, _ = _class_ref("nan_inf", CLASS_ROUNDS)
    assert np.isnan(last).sum() > 1 and np.isfinite(last).any()


@pytest.mark.parametrize("family", ["subn", "huge", "nan_inf"])
def test_value_domain(family):
    g = class_graph()
    with fu.PairwiseSync(g, _values(family, g.n), seed=SEED) as eng:
        for r in (3, CLASS_ROUNDS):
            eng.run(r - eng.rounds_done)
            _check(eng, _class_ref(family, r), (family, "round", r))


# ------------------------------------------------------------------------------------
# 4. split runs, seed changes, reset, new inputs
# ------------------------------------------------------------------------------------
def test_split_run_equals_one_run():
    g = class_graph()
    v = _values("uniform", g.n)
    ref = oracle_pair(*g.arrays(), v, 17, SEED)
    with fu.PairwiseSync(g, v, seed=SEED) as one, fu.PairwiseSync(g, v, seed=SEED) as two:
        one.run(17)
        two.run(5)
        two.run(12)
        assert one.rounds_done == two.rounds_done == 17
        _check(one, ref, ("run(17)",))
        _check(two, ref, ("run(5); run(12)",))


def test_seed_changes_between_runs_then_reset():
    """Seed 3 for rounds 0-5, seed 0 for 6-11, seed 9 for 12-16: the round counter is absolute,
    so round 12 is element 12 of seed 9's stream. Then reset() and 12 rounds under seed 9."""
    g = class_graph()
    v = _values("uniform", g.n)

    def seed(r):
        return 3 if r < 6 else 0 if r < 12 else 9

    ref = oracle_pair(*g.arrays(), v, 17, seed)
    ref2 = oracle_pair(*g.arrays(), v, 12, 9)
    assert not np.array_equal(ref[0], oracle_pair(*g.arrays(), v, 17, 3)[0])
    with fu.PairwiseSync(g, v) as eng:
        for s, rounds in ((3, 6), (0, 6), (9, 5)):
            eng.set_seed(s)
            eng.run(rounds)
        _check(eng, ref, ("three seeds",))
        assert eng.stats[0] == pair_count(*g.arrays(), seed, 17)
        eng.reset()
        assert eng.rounds_done == 0 and eng.stats == (0, g.n)
        assert not eng.estimates().any() and not eng.flows().any() and not eng.cache().any()
        eng.run(12)
        _check(eng, ref2, ("after reset",))
        assert eng.stats[0] == pair_count(*g.arrays(), 9, 12)


def test_set_values_in_mid_run():
    g = hub60()
    vs = [fu.uniform_values(g.n, seed=s) for s in (4, 5, 6)]
    ref = pair_python(*g.arrays(), lambda r: vs[0] if r < 4 else vs[1] if r < 9 else vs[2], 14, SEED)
    with fu.PairwiseSync(g, vs[0], seed=SEED) as eng:
        eng.run(4)
        eng.set_values(vs[1])
        eng.run(5)
        eng.set_values(vs[2])
        eng.run(5)
        assert eng.rounds_done == 14
        _check(eng, ref, ("values replaced after rounds 4 and 9",))


# ------------------------------------------------------------------------------------
# 5. error trace and statistics
# ------------------------------------------------------------------------------------
def test_error_trace_max_err_and_stats():
    g = class_graph()
    v = _values("uniform", g.n)
    tgt, _ = fu.component_means(g.rowptr, g.col, v)
    _, _, _, snaps = _class_ref("uniform", CLASS_ROUNDS, snaps=tuple(range(CLASS_ROUNDS)))
    want = np.array([np.max(np.abs(snaps[r] - tgt)) for r in range(CLASS_ROUNDS)])
    with fu.PairwiseSync(g, v, seed=SEED) as eng:
        eng.set_targets(tgt)
        trace = eng.run(CLASS_ROUNDS, err_every=1)
        assert_same_bits(trace, want, "error trace")
        assert_same_bits(np.array([eng.max_err()]), want[-1:], "max_err")
        assert eng.stats[0] == pair_count(*g.arrays(), SEED, CLASS_ROUNDS)
        t2 = tgt.copy()
        t2[5] = np.nan  # one NaN target makes the maximum NaN
        eng.set_targets(t2)
        assert np.isnan(eng.max_err())
    with fu.PairwiseSync(g, v, seed=SEED) as eng:
        eng.set_targets(tgt)
        trace = eng.run(CLASS_ROUNDS, err_every=8)
        assert_same_bits(trace, want[7::8], "every 8th round")


def test_cli_bench_graph_with_pairs(capsys):
    """`python -m fu bench-graph SPEC --pairs --pair-seed S` (in process): the usual line plus
    pairs=<count>, the count being the helper's."""
    from fu.__main__ import main

    assert main(["bench-graph", "er:n=2000,m=8000", "--rounds", "6", "--pairs", "--pair-seed", "4"]) == 0
    line = capsys.readouterr().out.strip()
    g = fu.Graph.from_spec("er:n=2000,m=8000", seed=1)
    assert line.startswith(f"graph n={g.n} E={g.E} ") and " rounds=6 " in line and " max_err=" in line
    assert line.endswith(f" pairs={pair_count(*g.arrays(), 4, 6)}")


# ------------------------------------------------------------------------------------
# 6. edge shapes
# ------------------------------------------------------------------------------------
def test_one_node_two_nodes_no_edges_and_isolated_nodes():
    no_i32 = np.zeros(0, dtype=np.int32)
    with fu.PairwiseSync(rowptr=np.zeros(2, dtype=np.int64), col=no_i32, values=np.array([3.5])) as eng:  # n = 1
        eng.run(4)
        _check(eng, (np.zeros(1), np.zeros(0), np.zeros(0)), ("n = 1",))
        assert eng.stats == (0, 1) and eng.rounds_done == 4
    v = np.array([1.0, -2.5, -0.0, 1e300, 5e-324])
    with fu.PairwiseSync(rowptr=np.zeros(6, dtype=np.int64), col=no_i32, values=v) as eng:  # no edges at all
        eng.run(3)
        _check(eng, (np.zeros(5), np.zeros(0), np.zeros(0)), ("no edges",))
        assert eng.stats == (0, 5)
    rp, col, rev = np.array([0, 1, 2], dtype=np.int64), np.array([1, 0], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    v = np.array([1.0, 4.0])
    pairs = pair_count(rp, col, rev, 5, 12)
    assert 0 < pairs < 12  # the two nodes pair up when exactly one of them proposes
    with fu.PairwiseSync(rowptr=rp, col=col, values=v, seed=5) as eng:  # n = 2
        eng.run(12)
        _check(eng, pair_python(rp, col, rev, v, 12, 5), ("n = 2",))
        assert eng.stats == (pairs, 0)
    g = fu.Graph.from_edges(9, [0, 1, 4], [1, 2, 5])  # nodes 3, 6, 7, 8 have degree 0
    v = fu.uniform_values(g.n, seed=2)
    ref = pair_python(*g.arrays(), v, 20, SEED)
    assert np.count_nonzero(ref[0]) == 5  # every node with an edge has fired, no other
    with fu.PairwiseSync(g, v, seed=SEED) as eng:
        eng.run(20)
        _check(eng, ref, ("degree-0 nodes beside matched ones",))
        assert eng.stats == (pair_count(*g.arrays(), SEED, 20), 4)


# ------------------------------------------------------------------------------------
# 7. more heavy pairs than blocks, heavy rows paired with heavy rows
# ------------------------------------------------------------------------------------
DENSE_ROUNDS = 6


@functools.lru_cache(maxsize=None)
def _dense_ref(rounds):
    """On pair_cases.dense66() with `wide` values (36 decades of both signs: a misplaced -F1
    shows in the high bits), from the oracle."""
    g = dense66()
    return oracle_pair(*g.arrays(), _values("wide", g.n), rounds, SEED)


@pytest.mark.parametrize("match", MATCHERS)
def test_more_heavy_pairs_than_blocks_round_by_round(match):
    """Every row of dense66() has 66 slots, so every pair goes to the block-per-pair kernel with
    both rows above 64, and each of rounds 0-5 lists more than 1024 pairs (asserted in
    test_engine_case_inputs.py): the blocks take a second pair from the list."""
    g = dense66()
    with fu.PairwiseSync(g, _values("wide", g.n), seed=SEED) as eng:
        eng.set_option("match", match)
        for r in range(1, DENSE_ROUNDS + 1):
            eng.run(1)
            _check(eng, _dense_ref(r), ("match", match, "round", r))
            assert eng.stats[0] == pair_count(*g.arrays(), SEED, r), r
        never = g.n - len(set().union(*roles(*g.arrays(), SEED, DENSE_ROUNDS)))
        assert eng.stats == (pair_count(*g.arrays(), SEED, DENSE_ROUNDS), never)


def test_more_heavy_pairs_than_blocks_split_run():
    g = dense66()
    with fu.PairwiseSync(g, _values("wide", g.n), seed=SEED) as eng:
        eng.run(2)
        eng.run(4)
        assert eng.rounds_done == DENSE_ROUNDS
        _check(eng, _dense_ref(DENSE_ROUNDS), ("run(2); run(4)",))
        assert eng.stats[0] == pair_count(*g.arrays(), SEED, DENSE_ROUNDS)


@pytest.mark.parametrize("match", MATCHERS)
def test_listener_on_the_only_slot_of_its_second_chunk(match):
    """class_graph() at LAST_SLOT_SEED: in round LAST_SLOT_ROUNDS - 2 the centre of degree 1025
    listens on slot 1024 (asserted in test_engine_case_inputs.py), so -F1 takes the place of the
    one element of the row's second chunk. Checked before that round, after it and a round on."""
    g = class_graph()
    v = _values("wide", g.n)
    with fu.PairwiseSync(g, v, seed=LAST_SLOT_SEED) as eng:
        eng.set_option("match", match)
        for r in (LAST_SLOT_ROUNDS - 2, LAST_SLOT_ROUNDS - 1, LAST_SLOT_ROUNDS):
            eng.run(r - eng.rounds_done)
            _check(eng, oracle_pair(*g.arrays(), v, r, LAST_SLOT_SEED), ("match", match, "round", r))
        assert eng.stats[0] == pair_count(*g.arrays(), LAST_SLOT_SEED, LAST_SLOT_ROUNDS)


# ------------------------------------------------------------------------------------
# the rule itself: the reference's Peers over the recorded matching (tests/golden/)
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("match", MATCHERS)
def test_reference_peers_over_recorded_matching(match):
    """hub_mix (rows of 2101 and 130 slots among rows of at most 7) at the recorded seed, run from
    stop to stop: last averages, flows and caches are what the reference's own avg_and_send /
    on_receive left (make_golden.pw_sync), and the pair counter is the recorded matching's."""
    import rule_cases

    d = rule_cases.load("pair")
    with fu.PairwiseSync(rowptr=d.rowptr, col=d.col, rev=d.rev, values=d.values, seed=d.seed) as eng:
        eng.set_option("match", match)
        for q, stop in enumerate(d.stops):
            eng.run(stop - eng.rounds_done)
            _check(eng, (d.last_avg[q], d.flows[q], d.estimates[q]), ("reference peers", "match", match, "after", stop))
            assert eng.stats[0] == int(d.initiator[:stop].sum()), stop
