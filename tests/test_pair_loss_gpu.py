"""fu.PairwiseSync under message loss (csrc/fu_pair.hip, the lossy forms of kp_exchange and
kp_heavy) against restatements that do not run it: pair_loss_cases.oracle_pair_loss (the C
oracle's replay of a trace in which the lost messages are read by nobody), pair_loss_python where
inputs change or are non-finite, and the reference's own recording. Every comparison is by bit
pattern, on last averages, flows and caches; the counters against the helper's census. The
conditions that make the cases meaningful are asserted in test_pair_loss_case_inputs.py."""
import functools

import numpy as np
import pytest

import fu
import vd_cases
from pair_cases import (CLASS_ROUNDS, LAST_SLOT_ROUNDS, LAST_SLOT_SEED, SEED, class_graph, dense66, oracle_pair, pair_count,
                        rr256_d8)
from pair_loss_cases import (CLASS_P, CONV_P, CONV_ROUNDS, LOSS_SEED, MASK_CLEARED_AT, VD_ROUNDS, fired_nodes, hashed,
                             link_mask, load_recording, loss_counts, oracle_pair_loss, pair_loss_python)
from parity_util import assert_same_bits

pytestmark = pytest.mark.gpu

MATCHERS = [0, 1]


def _check(eng, ref, what):
    assert_same_bits(eng.estimates(), ref[0], what + ("last",))
    assert_same_bits(eng.flows(), ref[1], what + ("flows",))
    assert_same_bits(eng.cache(), ref[2], what + ("cache",))


def _check_counts(eng, g, seed, rounds, lost, what):
    m1, m2, full = loss_counts(*g.arrays(), seed, rounds, lost)
    assert eng.loss_stats == (m1, m2, full), what
    assert eng.stats == (m1 + m2 + full, g.n - len(fired_nodes(*g.arrays(), seed, rounds, lost))), what
    assert m1 + m2 + full == pair_count(*g.arrays(), seed, rounds)


def _uniform(g):
    return fu.uniform_values(g.n, seed=3)


# ------------------------------------------------------------------------------------
# 1. no loss is today's engine
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [rr256_d8, class_graph])
def test_no_loss_is_the_lossless_engine(graph):
    """set_loss(0.0, seed=5) and an all-zero mask run the lossy kernels with nothing to lose: the
    state and the statistics are a plain PairwiseSync's (and the oracle's), all pairs complete."""
    g = graph()
    v = _uniform(g)
    with fu.PairwiseSync(g, v, seed=SEED) as plain, fu.PairwiseSync(g, v, seed=SEED) as eng:
        eng.set_loss(0.0, seed=5)
        eng.set_link_mask(np.zeros(g.E, dtype=np.uint8))
        plain.run(40)
        eng.run(40)
        ref = oracle_pair(*g.arrays(), v, 40, SEED)
        _check(plain, ref, ("plain",))
        _check(eng, ref, ("p = 0, zero mask",))
        assert eng.stats == plain.stats
        assert eng.loss_stats == (0, 0, plain.stats[0]) and plain.loss_stats == (0, 0, plain.stats[0])


# ------------------------------------------------------------------------------------
# 2. the three outcomes
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("match", MATCHERS)
@pytest.mark.parametrize("p", [0.1, 0.5, 1.0])
def test_the_three_outcomes(p, match):
    g = rr256_d8()
    v = fu.uniform_values(g.n, seed=0)
    lost = hashed(p, LOSS_SEED, g.E)
    with fu.PairwiseSync(g, v, seed=SEED, loss=p, loss_seed=LOSS_SEED) as eng:
        eng.set_option("match", match)
        for r in (1, 2, 3, 60):
            eng.run(r - eng.rounds_done)
            _check(eng, oracle_pair_loss(*g.arrays(), v, r, SEED, lost), ("p", p, "match", match, "round", r))
            _check_counts(eng, g, SEED, r, lost, (p, match, r))
        if p == 1.0:  # every initiator fires alone, no listener ever fires
            ini = fired_nodes(*g.arrays(), SEED, 60, lost)
            assert eng.loss_stats[1:] == (0, 0) and eng.stats[1] == g.n - len(ini)


# ------------------------------------------------------------------------------------
# 3. degree boundaries, the last slot of a second chunk, more heavy pairs than blocks
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _class_ref(rounds):
    g = class_graph()
    return oracle_pair_loss(*g.arrays(), _uniform(g), rounds, SEED, hashed(CLASS_P, LOSS_SEED, g.E))


@pytest.mark.parametrize("match", MATCHERS)
def test_every_degree_boundary_under_loss(match):
    g = class_graph()
    lost = hashed(CLASS_P, LOSS_SEED, g.E)
    with fu.PairwiseSync(g, _uniform(g), seed=SEED, loss=CLASS_P, loss_seed=LOSS_SEED) as eng:
        eng.set_option("match", match)
        for r in (1, 2, 7, CLASS_ROUNDS):
            eng.run(r - eng.rounds_done)
            _check(eng, _class_ref(r), ("match", match, "round", r))
        _check_counts(eng, g, SEED, CLASS_ROUNDS, lost, match)


def test_listener_on_the_only_slot_of_its_second_chunk_under_loss():
    g = class_graph()
    v = _uniform(g)
    lost = hashed(CLASS_P, LOSS_SEED, g.E)
    with fu.PairwiseSync(g, v, seed=LAST_SLOT_SEED, loss=CLASS_P, loss_seed=LOSS_SEED) as eng:
        for r in (LAST_SLOT_ROUNDS - 2, LAST_SLOT_ROUNDS - 1, LAST_SLOT_ROUNDS):
            eng.run(r - eng.rounds_done)
            _check(eng, oracle_pair_loss(*g.arrays(), v, r, LAST_SLOT_SEED, lost), ("round", r))
        _check_counts(eng, g, LAST_SLOT_SEED, LAST_SLOT_ROUNDS, lost, "last slot")


@pytest.mark.parametrize("match", MATCHERS)
def test_more_heavy_pairs_than_blocks_under_loss(match):
    g = dense66()
    v = _uniform(g)
    lost = hashed(CLASS_P, LOSS_SEED, g.E)
    with fu.PairwiseSync(g, v, seed=SEED, loss=CLASS_P, loss_seed=LOSS_SEED) as eng:
        eng.set_option("match", match)
        for r in (1, 2, 3):
            eng.run(1)
            _check(eng, oracle_pair_loss(*g.arrays(), v, r, SEED, lost), ("match", match, "round", r))
            _check_counts(eng, g, SEED, r, lost, (match, r))


# ------------------------------------------------------------------------------------
# 4. the mask alone
# ------------------------------------------------------------------------------------
def test_mask_alone_then_cleared():
    """p = 0: the mask forces the outcomes (down both ways: m1 lost whoever initiates; down one
    way: m1 or m2 lost by direction). set_link_mask(None) after round 19 equals the reference with
    the mask dropped from round 20 on."""
    g = class_graph()
    v = _uniform(g)
    down = link_mask(g)
    lost = hashed(0.0, 0, g.E, lambda r: down if r < MASK_CLEARED_AT else None)
    with fu.PairwiseSync(g, v, seed=SEED, link_mask=down.astype(bool)) as eng:
        for r in (1, MASK_CLEARED_AT):
            eng.run(r - eng.rounds_done)
            _check(eng, oracle_pair_loss(*g.arrays(), v, r, SEED, lost), ("masked", r))
        _check_counts(eng, g, SEED, MASK_CLEARED_AT, lost, "masked")
        eng.set_link_mask(None)
        eng.run(CLASS_ROUNDS - MASK_CLEARED_AT)
        _check(eng, oracle_pair_loss(*g.arrays(), v, CLASS_ROUNDS, SEED, lost), ("cleared",))
        _check_counts(eng, g, SEED, CLASS_ROUNDS, lost, "cleared")


# ------------------------------------------------------------------------------------
# 5. splits and switches
# ------------------------------------------------------------------------------------
def test_split_run_equals_one_run():
    g = class_graph()
    v = _uniform(g)
    lost = hashed(CLASS_P, LOSS_SEED, g.E)
    ref = oracle_pair_loss(*g.arrays(), v, 17, SEED, lost)
    kw = dict(seed=SEED, loss=CLASS_P, loss_seed=LOSS_SEED)
    with fu.PairwiseSync(g, v, **kw) as one, fu.PairwiseSync(g, v, **kw) as two:
        one.run(17)
        two.run(5)
        two.run(12)
        _check(one, ref, ("run(17)",))
        _check(two, ref, ("run(5); run(12)",))
        assert one.loss_stats == two.loss_stats == loss_counts(*g.arrays(), SEED, 17, lost)


def test_loss_seed_and_values_change_between_runs_then_reset():
    """Rounds 0-4 at (p, loss seed, matching seed) = (0.3, 5, 11), 5-9 at (0.6, 8, 11) with new
    values, 10-13 at (0.0, 8, 4) under a mask. reset() keeps the last p, seeds and mask and zeroes
    the counters, so the rerun equals a fresh handle's run under them."""
    g = rr256_d8()
    vs = [fu.uniform_values(g.n, seed=s) for s in (4, 5)]
    down = link_mask(g, seed=2)
    p = lambda r: 0.3 if r < 5 else 0.6 if r < 10 else 0.0  # noqa: E731
    ls = lambda r: 5 if r < 5 else 8  # noqa: E731
    ms = lambda r: 11 if r < 10 else 4  # noqa: E731
    lost = hashed(p, ls, g.E, lambda r: None if r < 10 else down)
    ref = pair_loss_python(*g.arrays(), lambda r: vs[0] if r < 5 else vs[1], 14, ms, lost)
    with fu.PairwiseSync(g, vs[0], seed=11, loss=0.3, loss_seed=5) as eng:
        eng.run(5)
        eng.set_loss(0.6, 8)
        eng.set_values(vs[1])
        eng.run(5)
        eng.set_loss(0.0, 8)
        eng.set_seed(4)
        eng.set_link_mask(down)
        eng.run(4)
        _check(eng, ref, ("three settings",))
        assert eng.loss_stats == loss_counts(*g.arrays(), ms, 14, lost)
        eng.reset()
        assert eng.rounds_done == 0 and eng.stats == (0, g.n) and eng.loss_stats == (0, 0, 0)
        assert not eng.estimates().any() and not eng.flows().any() and not eng.cache().any()
        eng.run(12)
        kept = hashed(0.0, 8, g.E, down)
        ref2 = oracle_pair_loss(*g.arrays(), vs[1], 12, 4, kept)
        _check(eng, ref2, ("after reset",))
        _check_counts(eng, g, 4, 12, kept, "after reset")
        with fu.PairwiseSync(g, vs[1], seed=4, loss=0.0, loss_seed=8, link_mask=down) as fresh:
            fresh.run(12)
            _check(fresh, ref2, ("fresh handle",))
            assert fresh.loss_stats == eng.loss_stats and fresh.stats == eng.stats


def test_two_handles_interleaved_round_by_round():
    g = rr256_d8()
    v = fu.uniform_values(g.n, seed=0)
    with fu.PairwiseSync(g, v, seed=SEED, loss=0.1, loss_seed=LOSS_SEED) as a, \
            fu.PairwiseSync(g, v, seed=SEED, loss=0.5, loss_seed=LOSS_SEED) as b:
        for _ in range(12):
            a.run(1)
            b.run(1)
        for eng, p in ((a, 0.1), (b, 0.5)):
            lost = hashed(p, LOSS_SEED, g.E)
            _check(eng, oracle_pair_loss(*g.arrays(), v, 12, SEED, lost), ("interleaved", p))
            _check_counts(eng, g, SEED, 12, lost, p)


# ------------------------------------------------------------------------------------
# 6. the fp64 value domain
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", vd_cases.RULE_FAMILIES)
def test_value_domain_under_loss(family):
    """hub_mix with signed zeros and subnormals (`subn`) and non-finite inputs (`special`): a lost
    m1 leaves (f + a) - c standing where the lossless exchange overwrites it, so the sign of a
    zero and the place of a NaN follow the Python floats slot by slot."""
    d, g = vd_cases.rule("pair", family)
    lost = hashed(CLASS_P, LOSS_SEED, g.E)
    with fu.PairwiseSync(rowptr=g.rowptr, col=g.col, rev=g.rev, values=d.values, seed=g.seed, loss=CLASS_P,
                         loss_seed=LOSS_SEED) as eng:
        for r in (3, VD_ROUNDS):
            eng.run(r - eng.rounds_done)
            _check(eng, pair_loss_python(g.rowptr, g.col, g.rev, d.values, r, g.seed, lost), (family, "round", r))
        assert eng.loss_stats == loss_counts(g.rowptr, g.col, g.rev, g.seed, VD_ROUNDS, lost)


# ------------------------------------------------------------------------------------
# 7. the reference's recording
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("match", MATCHERS)
def test_reference_peers_with_lost_messages_dropped(match):
    """The engine at the fixture's seeds, p and mask against what the reference's own
    avg_and_send / on_receive left at stops 5, 20 and 40 (make_pair_lossy_golden.py)."""
    d = load_recording()
    with fu.PairwiseSync(rowptr=d.rowptr, col=d.col, rev=d.rev, values=d.values, seed=d.seed, loss=d.p,
                         loss_seed=d.loss_seed, link_mask=d.down) as eng:
        eng.set_option("match", match)
        for q, stop in enumerate(d.stops):
            eng.run(stop - eng.rounds_done)
            _check(eng, (d.last_avg[q], d.flows[q], d.estimates[q]), ("reference peers", "match", match, "after", stop))
            assert eng.stats[0] == int(d.initiator[:stop].sum()), stop
        assert eng.loss_stats == (2363, 1536, 4504)


# ------------------------------------------------------------------------------------
# 8. error trace and convergence
# ------------------------------------------------------------------------------------
def test_error_trace_and_convergence():
    """rr256_d8 at p = 0.1, err_every = 8 over CONV_ROUNDS rounds: the trace is the reference's,
    bit for bit (whose last entry is below 1e-6 of the first error: test_pair_loss_case_inputs)."""
    g = rr256_d8()
    v = fu.uniform_values(g.n, seed=0)
    tgt, _ = fu.component_means(g.rowptr, g.col, v)
    lost = hashed(CONV_P, LOSS_SEED, g.E)
    at = tuple(range(7, CONV_ROUNDS, 8))
    last, f, c, sn = oracle_pair_loss(*g.arrays(), v, CONV_ROUNDS, SEED, lost, snaps=at)
    want = np.array([np.max(np.abs(sn[r] - tgt)) for r in at])
    with fu.PairwiseSync(g, v, seed=SEED, loss=CONV_P, loss_seed=LOSS_SEED) as eng:
        eng.set_targets(tgt)
        trace = eng.run(CONV_ROUNDS, err_every=8)
        assert_same_bits(trace, want, "error trace")
        _check(eng, (last, f, c), ("after", CONV_ROUNDS))
        assert_same_bits(np.array([eng.max_err()]), np.array([np.max(np.abs(last - tgt))]), "max_err")
        _check_counts(eng, g, SEED, CONV_ROUNDS, lost, "convergence")


def test_cli_bench_graph_with_pairs_and_loss(capsys):
    from fu.__main__ import main

    argv = ["bench-graph", "er:n=2000,m=8000", "--rounds", "6", "--pairs", "--pair-seed", "4", "--loss", "0.3", "--loss-seed", "9"]
    assert main(argv) == 0
    line = capsys.readouterr().out.strip()
    g = fu.Graph.from_spec("er:n=2000,m=8000", seed=1)
    m1, m2, _ = loss_counts(*g.arrays(), 4, 6, hashed(0.3, 9, g.E))
    assert line.startswith(f"graph n={g.n} E={g.E} ") and " rounds=6 " in line
    assert line.endswith(f" pairs={pair_count(*g.arrays(), 4, 6)} lost={m1 + m2}") and m1 > 0 and m2 > 0
