"""The conditions of the pairwise-under-churn cases (tests/test_pair_churn_gpu.py), asserted on
the host: the restatement equals both recordings of the reference, the host matching under a
topology equals a Python-int restatement and the plain matching of the live subgraph, and the
case inputs hold what the GPU tests are there to reach."""
import numpy as np
import pytest

import fu
import pair_churn_cases as pc
from pair_cases import SEED, pair_python, rr256_d8
from pair_loss_cases import hashed, pair_loss_python
from parity_util import assert_same_bits


# ------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [0, 1])
def test_restatement_equals_the_recording(run):
    """Round by round: the state after 10, 20, 30 and 40 rounds, each stop a run from zero."""
    R = pc.load_recording()
    assert R.python.startswith("3.10") and R.stops == [10, 20, 30, 40] and R.events == [10, 20, 30]
    assert not R.alive[0][1] and R.alive[2].all() and R.link_up[2].all() and not R.link_up[1].all()
    lost = (lambda r: R.lost[r]) if run else None
    for q, stop in enumerate(R.stops):
        got = pc.pair_churn_python(R.rowptr, R.col, R.rev, R.values, stop, R.seed, R.script, lost=lost)
        assert_same_bits(got[0], R.last_avg[run][q], ("last", run, stop))
        assert_same_bits(got[1], R.flows[run][q], ("flows", run, stop))
        assert_same_bits(got[2], R.estimates[run][q], ("estimates", run, stop))
    assert not np.array_equal(R.last_avg[0][3], R.last_avg[1][3])


def test_recorded_matchings_are_the_host_helpers():
    R = pc.load_recording()
    for r in range(40):
        a, u = pc.topology_at(R.script, r, R.n, R.E)
        mate, ini = fu.pair_matching((R.rowptr, R.col), R.seed, r, alive=a, link_up=u)
        assert np.array_equal(mate, R.mate[r]) and np.array_equal(ini, R.initiator[r]), r
        assert np.array_equal(fu.pair_lost(R.loss_seed, r, 0, R.E, R.p).astype(bool), R.lost[r]), r
    # both hubs are matched under every topology in which they are alive
    for h, spans in ((0, [(0, 10), (10, 20), (20, 30), (30, 40)]), (1, [(0, 10), (30, 40)])):
        for b, e in spans:
            assert (R.mate[b:e, h] >= 0).any(), (h, b)
    assert (R.mate[10:30, 1] < 0).all()  # dead


def test_without_a_script_it_is_the_plain_restatement():
    g = rr256_d8()
    v = fu.uniform_values(g.n, seed=3)
    a = pc.pair_churn_python(*g.arrays(), v, 12, SEED, {})
    b = pair_python(*g.arrays(), v, 12, SEED)
    lost = hashed(0.3, 5, g.E)
    c = pc.pair_churn_python(*g.arrays(), v, 12, SEED, {}, lost=lost)
    d = pair_loss_python(*g.arrays(), v, 12, SEED, lost)
    for q in range(3):
        assert_same_bits(a[q], b[q], ("plain", q))
        assert_same_bits(c[q], d[q], ("loss", q))


# ------------------------------------------------------------------------------------
# the host matching
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [pc.class_graph, rr256_d8])
def test_host_matching_equals_python_ints_and_the_live_subgraph(graph):
    g = graph()
    rp, col, rev = g.arrays()
    src = np.repeat(np.arange(g.n), np.diff(rp))
    for seed, r in ((SEED, 0), (SEED, 7), (0xFEDCBA9876543210, 2 ** 31)):
        alive, up = pc.random_topology(g, seed=r % 97 + 1)
        live = pc.live_np(rp, col, alive, up)
        assert np.array_equal(live, fu.churn_live(g, alive, up).astype(bool))
        mate, ini = fu.pair_matching(g, seed, r, alive=alive, link_up=up)
        m_py, i_py, slot = pc.matching_live_py(rp, col, live, seed, r)
        assert mate.tolist() == m_py and ini.tolist() == i_py
        # a matching, over live slots and alive nodes only
        on = np.flatnonzero(mate >= 0)
        assert len(on) > 0 and np.array_equal(mate[mate[on]], on) and alive[on].all()
        assert (ini[on] + ini[mate[on]] == 1).all()
        for i in np.flatnonzero(ini):
            assert live[slot[i]] and src[slot[i]] == i and col[slot[i]] == mate[i]
        # the plain matching of the live subgraph
        rp2, col2, _ = pc.subgraph(rp, col, live)
        m2, i2 = fu.pair_matching((rp2, col2), seed, r)
        assert np.array_equal(mate, m2) and np.array_equal(ini, i2)
        # all ones, given or not, is the matching without a topology
        m0, i0 = fu.pair_matching(g, seed, r)
        for kw in ({"alive": np.ones(g.n, np.uint8)}, {"link_up": np.ones(g.E, np.uint8)}, {"alive": None, "link_up": None}):
            m1, i1 = fu.pair_matching(g, seed, r, **kw)
            assert np.array_equal(m0, m1) and np.array_equal(i0, i1)
        assert not np.array_equal(m0, mate)


# ------------------------------------------------------------------------------------
# what the class script reaches
# ------------------------------------------------------------------------------------
def _class_pairs():
    g = pc.class_graph()
    rp, col, rev = g.arrays()
    out = []
    for r in range(pc.CLASS_ROUNDS):
        live = pc.live_at(rp, col, pc.class_script(), r)
        out.append((live, pc.pairs_live(rp, col, rev, live, SEED, r)))
    return g, out


def test_class_script_reaches_every_edge():
    g, rounds = _class_pairs()
    rp = np.asarray(g.rowptr, dtype=np.int64)
    deg = np.diff(rp)
    k = len(pc.CLASS_DEGREES)
    script = pc.class_script()
    assert sorted(script) == list(pc.CLASS_EVENTS)
    a10, a30 = script[10][0], script[30][0]
    assert not a10[pc.DEAD_HEAVY] and deg[pc.DEAD_HEAVY] == 2500 and a30 is None  # a dead heavy row, re-added
    assert (a10[k:] == 0).sum() > 50
    # matched pairs at every degree edge, as initiator or listener, while the row has dropped slots
    need = set(pc.EDGE_DEGREES) | set(pc.COLS_EDGE_DEGREES)
    seen_i, seen_j = set(), set()
    first_pick = last_pick = only_last = readded = False
    for r, (live, pairs) in enumerate(rounds):
        ldeg = np.add.reduceat(live.astype(np.int64), rp[:-1][deg > 0])
        full = np.zeros(g.n, dtype=np.int64)
        full[deg > 0] = ldeg
        for i, s, j, t in pairs:
            for node, seen in ((i, seen_i), (j, seen_j)):
                if full[node] < deg[node]:
                    seen.add(int(deg[node]))
            ks = rp[i] + s
            if not live[rp[i]] and not live[rp[i + 1] - 1]:  # first and last CSR slot dropped
                mine = np.flatnonzero(live[rp[i]:rp[i + 1]]) + rp[i]
                first_pick |= ks == mine[0] and len(mine) > 1
                last_pick |= ks == mine[-1] and len(mine) > 1
            if pc.ONLY_LAST in (i, j) and r >= 20:
                only_last = True
            if r >= 30 and (not a10[i] or not a10[j]):
                readded = True
            assert r < 10 or r >= 30 or (a10[i] and a10[j])  # a dead node is in no pair
    assert need <= (seen_i | seen_j), sorted(need - (seen_i | seen_j))
    assert set(pc.EDGE_DEGREES) <= seen_j and {64, 65} <= seen_i, (sorted(seen_i), sorted(seen_j))
    assert first_pick and last_pick and only_last and readded
    # the row with one live slot, its last; the alive row with none
    live20 = rounds[20][0]
    row = live20[rp[pc.ONLY_LAST]:rp[pc.ONLY_LAST + 1]]
    assert row.sum() == 1 and row[-1] and script[20][0][pc.ONLY_LAST]
    assert not live20[rp[pc.NO_LIVE]:rp[pc.NO_LIVE + 1]].any() and script[20][0][pc.NO_LIVE]
    assert all(pc.NO_LIVE not in (i, j) for _, pairs in rounds[20:] for i, _, j, _ in pairs)
    # dropped slots on both sides of each edge: every centre of degree >= 8 lost its first and last slot
    for c, d in enumerate(pc.CLASS_DEGREES):
        if d >= 8 and c != pc.DEAD_HEAVY:
            assert not live20[rp[c]] and not live20[rp[c + 1] - 1] and live20[rp[c]:rp[c + 1]].any()
    # the heavy centre is matched again after it came back
    assert any(pc.DEAD_HEAVY in (i, j) for _, pairs in rounds[30:] for i, _, j, _ in pairs)
    assert not any(pc.DEAD_HEAVY in (i, j) for _, pairs in rounds[10:30] for i, _, j, _ in pairs)


def test_tile_limit_topologies_change_the_matching():
    from lossy_cases import tile_limit_graph

    g = tile_limit_graph()
    rp, col, rev = g.arrays()
    sizes = set()
    for r in range(10):
        alive, up = pc.random_topology(g, seed=100 + r)
        live = pc.live_np(rp, col, alive, up)
        assert 0 < live.sum() < g.E
        sizes.add(len(pc.pairs_live(rp, col, rev, live, SEED, r)))
    assert min(sizes) > 0


# ------------------------------------------------------------------------------------
# the convergence run
# ------------------------------------------------------------------------------------
def test_convergence_run_length():
    """On the small connected graph the restatement's error over the alive nodes, against
    churn_targets, is below 1e-9 of its value at the last event after CONV_ROUNDS rounds; the
    alive nodes of the last topology are one component, so the target is one mean."""
    g = pc.conv_graph()
    script = pc.conv_script()
    a, u = pc.topology_at(script, pc.CONV_ROUNDS, g.n, g.E)
    assert 0 < (a == 0).sum() < g.n // 5 and (u == 0).sum() > 0
    tgt = fu.churn_targets(g, pc.conv_values(), a, u)
    assert len(set(tgt[a != 0].tolist())) == 1
    errs = []
    pc.pair_churn_python(*g.arrays(), pc.conv_values(), pc.CONV_ROUNDS, SEED, script, err=(pc.conv_targets, errs))
    at_event = errs[pc.CONV_EVENTS[-1]]
    assert at_event > 1.0
    assert errs[-1] < 1e-9 * at_event, (errs[-1], at_event)
    assert errs[pc.CONV_ROUNDS // 2] > errs[-1]
    # mass: sum over the alive of (v - sum of live flows) is the sum of the alive values
    last, f, c = pc.pair_churn_python(*g.arrays(), pc.conv_values(), 200, SEED, script)
    live = pc.live_np(g.rowptr, g.col, a, u)
    assert not f[~live].any() and not c[~live].any()
    assert np.array_equal(f[live], -f[np.asarray(g.rev)][live])
