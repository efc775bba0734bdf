"""fu.PairwiseSync and fu.PairwiseSyncBatch under a topology (csrc/fu_pair.hip: kp_topology,
kp_pick, kp_scan_live and the <Topo<..>> instantiations of the exchange kernels) against
restatements that do not run them: the reference's two recordings, a plain PairwiseSync on the
live subgraph, and pair_churn_cases.pair_churn_python. Every comparison is by bit pattern. The
conditions that make the cases meaningful are asserted in test_pair_churn_case_inputs.py."""
import functools

import numpy as np
import pytest

import fu
import pair_churn_cases as pc
from fu import _lib as L
from lossy_cases import tile_limit_graph
from pair_cases import SEED, rr256_d8
from pair_loss_cases import LOSS_SEED, hashed, link_mask
from parity_util import assert_same_bits

pytestmark = pytest.mark.gpu

MATCHERS = [0, 1]


def _check(eng, ref, what, col=None):
    pick = (lambda x: x) if col is None else (lambda x: np.ascontiguousarray(x[:, col]))
    assert_same_bits(pick(eng.estimates()), ref[0], what + ("last",))
    assert_same_bits(pick(eng.flows()), ref[1], what + ("flows",))
    assert_same_bits(pick(eng.cache()), ref[2], what + ("cache",))


def _run_script(eng, script, rounds, stops=()):
    """Run `rounds` rounds with the script's topology calls; yields at the stops."""
    at = sorted(set(script) | set(stops) | {rounds})
    for r in at:
        if r > rounds:
            break
        eng.run(r - eng.rounds_done)
        if r in stops or r == rounds:
            yield r
        if r in script and r < rounds:
            eng.set_topology(*script[r])


# ------------------------------------------------------------------------------------
# 1. the reference's recordings
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("match", MATCHERS)
@pytest.mark.parametrize("run", [0, 1])
def test_handle_equals_the_recording(run, match):
    R = pc.load_recording()
    kw = {"loss": R.p, "loss_seed": R.loss_seed} if run else {}
    with fu.PairwiseSync(rowptr=R.rowptr, col=R.col, rev=R.rev, values=R.values, seed=R.seed, **kw) as eng:
        eng.set_option("match", match)
        for r in _run_script(eng, R.script, 40, R.stops):
            q = R.stops.index(r)
            _check(eng, (R.last_avg[run][q], R.flows[run][q], R.estimates[run][q]), ("run", run, "match", match, "round", r))
        pairs = int((R.mate >= 0).sum()) // 2
        assert eng.stats[0] == pairs and sum(eng.loss_stats) == pairs
        assert (eng.loss_stats[0] > 0 and eng.loss_stats[1] > 0) if run else eng.loss_stats[:2] == (0, 0)


# ------------------------------------------------------------------------------------
# 2. a static topology is PairwiseSync on the live subgraph
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _static():
    """The class graph under its round-20 topology, its live subgraph, and per column of
    class_values(16) a plain PairwiseSync run of 24 rounds on the subgraph, slots mapped back."""
    g = pc.class_graph()
    alive, up = pc.class_script()[20]
    live = pc.live_np(g.rowptr, g.col, alive, up)
    rp2, col2, slots = pc.subgraph(g.rowptr, g.col, live)
    rev2 = pc.sub_rev(g.rev, live, slots)
    v = pc.class_values(16)
    refs = []
    for c in range(16):
        with fu.PairwiseSync(rowptr=rp2, col=col2, rev=rev2, values=v[:, c], seed=SEED) as sub:
            sub.run(24)
            f, ca = np.zeros(g.E), np.zeros(g.E)
            f[slots], ca[slots] = sub.flows(), sub.cache()
            refs.append((sub.estimates(), f, ca, sub.stats))
    return g, alive, up, v, refs


@pytest.mark.parametrize("match", MATCHERS)
def test_static_topology_is_the_live_subgraph_scalar(match):
    g, alive, up, v, refs = _static()
    with fu.PairwiseSync(g, v[:, 0], seed=SEED) as eng:
        eng.set_option("match", match)
        eng.set_topology(alive, up)
        eng.run(24)
        _check(eng, refs[0], ("scalar", match))
        assert eng.stats == refs[0][3]


@pytest.mark.parametrize("K", pc.K_CASES)
def test_static_topology_is_the_live_subgraph_columns(K):
    g, alive, up, v, refs = _static()
    with fu.PairwiseSyncBatch(g, np.ascontiguousarray(v[:, :K]), seed=SEED) as eng:
        eng.set_topology(alive, up)
        eng.run(24)
        for c in range(K):
            _check(eng, refs[c], ("K", K, "column", c), col=c)
        assert eng.stats == refs[0][3]


# ------------------------------------------------------------------------------------
# 3. the scripted runs equal the restatement
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _class_ref(col, stop, lossy):
    g = pc.class_graph()
    v = pc.class_values(16)[:, col]
    lost = hashed(0.3, LOSS_SEED, g.E) if lossy else None
    return pc.pair_churn_python(*g.arrays(), v, stop, SEED, pc.class_script(), lost=lost)


@pytest.mark.parametrize("match", MATCHERS)
def test_class_script_scalar(match):
    g = pc.class_graph()
    with fu.PairwiseSync(g, pc.class_values(16)[:, 0], seed=SEED) as eng:
        eng.set_option("match", match)
        for r in _run_script(eng, pc.class_script(), pc.CLASS_ROUNDS, (10, 20, 21, 30, 31)):
            _check(eng, _class_ref(0, r, False), ("match", match, "round", r))


@pytest.mark.parametrize("K", pc.K_CASES)
def test_class_script_columns(K):
    g = pc.class_graph()
    cols = sorted({0, 1, K - 1})
    with fu.PairwiseSyncBatch(g, np.ascontiguousarray(pc.class_values(16)[:, :K]), seed=SEED) as eng:
        for r in _run_script(eng, pc.class_script(), pc.CLASS_ROUNDS, (21, 31)):
            for c in cols:
                _check(eng, _class_ref(c, r, False), ("K", K, "column", c, "round", r), col=c)


def test_class_script_under_loss_and_mask():
    """Loss and mask compose with the topology: the decisions stay on the caller's slots; a
    half-healed link that is dropped loses both ends' cells; loss_stats sum to the pairs."""
    g = pc.class_graph()
    with fu.PairwiseSync(g, pc.class_values(16)[:, 0], seed=SEED, loss=0.3, loss_seed=LOSS_SEED) as eng, \
            fu.PairwiseSyncBatch(g, np.ascontiguousarray(pc.class_values(16)[:, :3]), seed=SEED, loss=0.3,
                                 loss_seed=LOSS_SEED) as cols:
        for r in _run_script(eng, pc.class_script(), pc.CLASS_ROUNDS, (20, 21, 31)):
            _check(eng, _class_ref(0, r, True), ("loss", "round", r))
        for r in _run_script(cols, pc.class_script(), pc.CLASS_ROUNDS):
            for c in range(3):
                _check(cols, _class_ref(c, r, True), ("loss", "column", c), col=c)
        for e in (eng, cols):
            assert sum(e.loss_stats) == e.stats[0] and min(e.loss_stats) > 0
        assert eng.stats == cols.stats and eng.loss_stats == cols.loss_stats
    g = rr256_d8()
    v = fu.uniform_values(g.n, seed=3)
    down = link_mask(g)
    script = {6: pc.random_topology(g, 5), 12: (None, None)}
    lost = hashed(0.0, 0, g.E, down=down)
    with fu.PairwiseSync(g, v, seed=SEED, link_mask=down) as eng:
        for r in _run_script(eng, script, 20, (6, 7, 12)):
            _check(eng, pc.pair_churn_python(*g.arrays(), v, r, SEED, script, lost=lost), ("mask", "round", r))
        assert sum(eng.loss_stats) == eng.stats[0] and min(eng.loss_stats[:2]) > 0


# ------------------------------------------------------------------------------------
# 4. a topology call before every round; both matching forms
# ------------------------------------------------------------------------------------
def test_a_topology_before_every_round_both_matchers():
    g = tile_limit_graph()
    v = fu.uniform_values(g.n, seed=3)
    script = {r: pc.random_topology(g, seed=100 + r) for r in range(10)}
    ref = pc.pair_churn_python(*g.arrays(), v, 10, SEED, script)
    got = []
    for match in MATCHERS:
        with fu.PairwiseSync(g, v, seed=SEED) as eng:
            eng.set_option("match", match)
            for r in range(10):
                eng.set_topology(*script[r])
                live = fu.churn_live(g, *script[r])
                assert eng.topology_stats == (int(np.count_nonzero(script[r][0])), int(live.sum()))
                assert np.array_equal(eng.slot_live(), live)
                eng.run(1)
            _check(eng, ref, ("match", match))
            got.append((eng.estimates(), eng.flows(), eng.cache(), eng.stats))
    for q in range(3):
        assert_same_bits(got[0][q], got[1][q], ("forms", q))
    assert got[0][3] == got[1][3]


# ------------------------------------------------------------------------------------
# 5. run lengths, reset, queueing
# ------------------------------------------------------------------------------------
def test_run_17_is_5_then_12_across_an_event_and_reset_keeps_the_topology():
    g = rr256_d8()
    v = fu.uniform_values(g.n, seed=3)
    t1, t2 = pc.random_topology(g, 1), pc.random_topology(g, 2)
    with fu.PairwiseSync(g, v, seed=SEED) as a, fu.PairwiseSync(g, v, seed=SEED) as b:
        for e, parts in ((a, [(17,), (9,)]), (b, [(5, 12), (4, 5)])):
            e.set_topology(*t1)
            for p in parts[0]:
                e.run(p)  # not synchronised: the topology call below queues behind these rounds
            e.set_topology(*t2)
            for p in parts[1]:
                e.run(p)
        ref = pc.pair_churn_python(*g.arrays(), v, 26, SEED, {0: t1, 17: t2})
        _check(a, ref, ("17 + 9",))
        _check(b, ref, ("5 + 12 + 4 + 5",))
        assert a.stats == b.stats
        a.reset()
        assert a.rounds_done == 0 and a.stats[0] == 0
        assert a.topology_stats == (int(np.count_nonzero(t2[0])), int(fu.churn_live(g, *t2).sum()))
        assert np.array_equal(a.slot_live(), fu.churn_live(g, *t2))
        assert not a.flows().any() and not a.cache().any() and not a.estimates().any()
        a.run(9)
        _check(a, pc.pair_churn_python(*g.arrays(), v, 9, SEED, {0: t2}), ("after reset",))


def test_all_ones_topology_and_an_untouched_neighbour_handle():
    """set_topology() with both None on a fresh handle is PairwiseSync bit for bit (through the
    topology kernels), and a handle that never gets a topology call, interleaved with one that
    has one, still is."""
    g = pc.class_graph()
    v = pc.class_values(16)[:, 0]
    with fu.PairwiseSync(g, v, seed=SEED) as plain:
        plain.run(24)
        ref = (plain.estimates(), plain.flows(), plain.cache())
        stats = plain.stats
    with fu.PairwiseSync(g, v, seed=SEED) as none, fu.PairwiseSync(g, v, seed=SEED) as ones, \
            fu.PairwiseSync(g, v, seed=SEED) as churned:
        ones.set_topology()
        assert ones.topology_stats == (g.n, g.E) == none.topology_stats and ones.slot_live().all() and none.slot_live().all()
        for r in range(0, 24, 4):
            churned.set_topology(*pc.random_topology(g, 7 + r))
            for e in (none, churned, ones):
                e.run(4)
        _check(none, ref, ("no topology call",))
        _check(ones, ref, ("all ones",))
        assert none.stats == stats and ones.stats == stats
    vk = np.ascontiguousarray(pc.class_values(16)[:, :3])
    with fu.PairwiseSyncBatch(g, vk, seed=SEED) as cols:
        cols.set_topology(np.full(g.n, 7, dtype=np.uint8), None)
        cols.run(24)
        _check(cols, ref, ("K = 3, all ones",), col=0)


# ------------------------------------------------------------------------------------
# 6. the error over the alive nodes, and convergence
# ------------------------------------------------------------------------------------
def test_convergence_trace_equals_the_restatement():
    g = pc.conv_graph()
    v, script = pc.conv_values(), pc.conv_script()
    errs = []
    pc.pair_churn_python(*g.arrays(), v, pc.CONV_ROUNDS, SEED, script, err=(pc.conv_targets, errs))
    with fu.PairwiseSync(g, v, seed=SEED) as eng:
        got = []
        for b, e in zip((0,) + pc.CONV_EVENTS, pc.CONV_EVENTS + (pc.CONV_ROUNDS,)):
            if b in script:
                eng.set_topology(*script[b])
            eng.set_targets(pc.conv_targets(b))
            got.append(eng.run(e - b, err_every=pc.CONV_EVERY))
        got = np.concatenate(got)
        want = np.array(errs[pc.CONV_EVERY - 1::pc.CONV_EVERY])
        assert_same_bits(got, want, ("trace",))
        assert_same_bits(np.array([eng.max_err()]), want[-1:], ("max_err",))
        # mass over the alive nodes
        a, u = script[pc.CONV_EVENTS[-1]]
        live = fu.churn_live(g, a, u).astype(bool)
        f = eng.flows()
        assert not f[~live].any() and not eng.cache()[~live].any()
        assert np.array_equal(f[live], -f[np.asarray(g.rev)][live])
        src = np.repeat(np.arange(g.n), np.diff(g.rowptr))
        est = v - np.bincount(src, weights=f, minlength=g.n)
        assert abs(est[a != 0].sum() - v[a != 0].sum()) < 1e-9 * v.sum()


def test_error_runs_over_the_alive_nodes_only():
    """A dead decoy 2^20 off and a NaN on a dead node do not show, for one column and for K."""
    g = rr256_d8()
    v = fu.uniform_values(g.n, seed=3)
    alive = np.ones(g.n, dtype=np.uint8)
    alive[[3, 200]] = 0
    tgt = fu.churn_targets(g, v, alive)
    for K in (None, 3):
        vv = v if K is None else np.stack([v] * K, axis=1)
        tt = tgt.copy() if K is None else np.stack([tgt] * K, axis=1)
        cls = fu.PairwiseSync if K is None else fu.PairwiseSyncBatch
        with cls(g, vv, seed=SEED) as eng, cls(g, vv, seed=SEED) as clean:
            for e in (eng, clean):
                e.set_topology(alive=alive)
            clean.set_targets(tt)
            want = clean.run(8, err_every=4)
            bad = tt.copy()
            bad[3] = bad[3] + 2.0 ** 20
            bad[200] = np.nan
            eng.set_targets(bad)
            got = eng.run(8, err_every=4)
            assert_same_bits(got, want, ("trace", K))
            assert_same_bits(np.atleast_1d(eng.max_err()), np.atleast_1d(clean.max_err()), ("max_err", K))
            assert np.all(np.atleast_1d(eng.max_err()) < 100.0)
            eng.set_topology()  # everyone alive again: the decoys show
            assert np.all(np.isnan(np.atleast_1d(eng.max_err())))
            eng.set_topology(alive=np.zeros(g.n, dtype=np.uint8))
            assert_same_bits(np.atleast_1d(eng.max_err()), np.zeros(K or 1), ("none alive", K))
            assert eng.topology_stats == (0, 0)


# ------------------------------------------------------------------------------------
# 7. degenerate shapes, mask bytes, the command line
# ------------------------------------------------------------------------------------
def test_degenerate_shapes():
    # one node
    with fu.PairwiseSync(rowptr=[0, 0], col=np.zeros(0, np.int32), values=[2.0]) as eng:
        eng.set_topology()
        assert eng.topology_stats == (1, 0) and eng.slot_live().shape == (0,)
        eng.set_topology(alive=[0])
        eng.run(3)
        assert eng.topology_stats == (0, 0) and eng.stats == (0, 1)
    # five isolated nodes, two dead
    with fu.PairwiseSync(rowptr=[0] * 6, col=np.zeros(0, np.int32), values=np.arange(5.0)) as eng:
        eng.set_topology(alive=[1, 0, 1, 0, 1])
        eng.run(3)
        assert eng.topology_stats == (3, 0) and eng.stats == (0, 5) and not eng.estimates().any()
    # two nodes, one link: down, then up again
    with fu.PairwiseSync(rowptr=[0, 1, 2], col=[1, 0], values=[1.0, 3.0], seed=SEED) as eng:
        eng.run(8)
        assert eng.estimates().tolist() == [2.0, 2.0] and eng.flows().tolist() == [-1.0, 1.0]
        eng.set_topology(link_up=[0, 0])
        assert eng.topology_stats == (2, 0) and not eng.flows().any() and not eng.cache().any()
        pairs = eng.stats[0]
        eng.run(8)
        assert eng.stats[0] == pairs and eng.estimates().tolist() == [2.0, 2.0]
        eng.set_topology(alive=[1, 1])
        eng.run(8)
        assert eng.stats[0] > pairs and eng.flows().tolist() == [-1.0, 1.0] and eng.topology_stats == (2, 2)
    # 1000 nodes and one link: the node count of a grid sized by the slots alone would stop at 256
    rp = np.zeros(1001, dtype=np.int64)
    rp[501:] = 1
    rp[901:] = 2
    alive = np.ones(1000, dtype=np.uint8)
    alive[::3] = 0
    alive[[500, 900]] = 1
    with fu.PairwiseSync(rowptr=rp, col=[900, 500], values=np.arange(1000.0), seed=SEED) as eng:
        eng.set_topology(alive=alive)
        assert eng.topology_stats == (int(alive.sum()), 2)
        eng.run(8)
        _check(eng, pc.pair_churn_python(rp, [900, 500], [1, 0], np.arange(1000.0), 8, SEED, {0: (alive, None)}), ("one link",))
        assert eng.stats[0] > 0 and eng.stats[1] == 998
        alive[900] = 0
        eng.set_topology(alive=alive)
        assert eng.topology_stats == (int(alive.sum()), 0) and not eng.flows().any()


def test_mask_bytes_other_than_0_and_1_through_the_c_entry_point():
    g = rr256_d8()
    v = fu.uniform_values(g.n, seed=3)
    alive, up = pc.random_topology(g, 3)
    rng = np.random.default_rng(1)
    a2 = (alive * rng.integers(1, 256, g.n)).astype(np.uint8)
    u2 = (up * np.uint8(0x80)).astype(np.uint8)
    assert set(np.unique(a2)) - {0, 1} and np.array_equal(a2 != 0, alive != 0)
    with fu.PairwiseSync(g, v, seed=SEED) as eng:
        L.call("fu_pair_set_topology", eng._h, L.ptr(a2), L.ptr(u2))
        eng.run(12)
        _check(eng, pc.pair_churn_python(*g.arrays(), v, 12, SEED, {0: (alive, up)}), ("bytes",))
        assert np.array_equal(eng.slot_live(), fu.churn_live(g, alive, up)) and set(np.unique(eng.slot_live())) <= {0, 1}


def test_cli_line(capsys):
    from fu.__main__ import main

    assert main(["bench-graph", "er:n=2000,m=8000", "--rounds", "40", "--pairs", "--pair-seed", "4", "--pair-churn", "0.1",
                 "--churn-seed", "3", "--pair-columns", "2", "--loss", "0.1"]) == 0
    line = capsys.readouterr().out.strip()
    dead = int((fu.uniform_values(2000, seed=3, lo=0.0, hi=1.0) < 0.1).sum())
    assert f" alive={2000 - dead} lost=" in line and " pairs=" in line and line.endswith(" columns=2")
