"""Several handles alive on one device at once. Every handle runs on a hipStreamNonBlocking
stream of its own, while the *_create calls upload and zero-fill through the null stream and the
*_destroy calls free memory: nothing orders one handle's calls against another handle's queued
rounds. Creating, running, resetting, reading back and destroying a handle must leave every other
handle's bits alone.

Each handle is compared with its own reference (coracle.ca_sync, lossy_cases.oracle_lossy,
pair_cases.oracle_pair, churn_cases.churn_python, coracle.replay), never with another handle, by
bit pattern. The graphs are ER(6000, 24000) and RMAT(12, 16): small enough for cheap references,
with heavy rows, several tiles and more than one block per XCD slot; the churn handle, whose
reference is Python, runs on lossy_cases.tile_limit_graph() (2641 nodes, one heavy row). At most 8 handles are open at any time; everything
runs in this process."""
import functools

import numpy as np
import pytest

import coracle
import fu
from churn_cases import churn_python, random_masks, tile_limit_graph, tile_segment
from lossy_cases import hashed, oracle_lossy
from pair_cases import oracle_pair
from parity_util import FAMILIES, assert_same_bits

pytestmark = pytest.mark.gpu

SEED = 11
LOSS = 0.25


@functools.lru_cache(maxsize=None)
def _er():
    return fu.Graph.erdos_renyi(6_000, 24_000, seed=23)


@functools.lru_cache(maxsize=None)
def _rmat():
    g = fu.Graph.rmat(12, 16, seed=4)
    assert g.max_deg > 256  # block-per-row rows
    return g


GRAPHS = {"er": _er, "rmat": _rmat}


@functools.lru_cache(maxsize=None)
def _ca_ref(graph, family, seed, rounds):
    """(v, a, f) after `rounds` collect-all rounds from zero, from the C oracle."""
    g = GRAPHS[graph]()
    v = FAMILIES[family](g.n, seed=seed)
    a, f = coracle.ca_sync(*g.arrays(), v, rounds, nthreads=16)
    return v, a, f


def _check_ca(eng, ref, what):
    assert_same_bits(eng.estimates(), ref[1], what + ("estimates",))
    assert_same_bits(eng.flows(), ref[2], what + ("flows",))


def _check_batch(eng, refs, what):
    a, f = eng.estimates(), eng.flows()
    for c, ref in enumerate(refs):
        assert_same_bits(np.ascontiguousarray(a[:, c]), ref[1], what + ("column", c, "estimates"))
        assert_same_bits(np.ascontiguousarray(f[:, c]), ref[2], what + ("column", c, "flows"))


# ------------------------------------------------------------------------------------
# 1. four engine types, rounds queued in turn
# ------------------------------------------------------------------------------------
def test_four_engine_types_round_robin():
    """CollectAll (stage, RMAT), CollectAllBatch (K = 2, ER), CollectAllLossy (p = 0.25, RMAT) and
    PairwiseSync (ER), each with values of its own: run(1) on each in turn, 12 turns, with no
    synchronize() in between; then every handle equals its own reference after 12 rounds. A
    CollectAllChurn handle (tile_limit_graph) takes the fifth place in every turn, with a
    set_topology (which waits for its own stream only) between its turns 4 and 5 and another
    between 9 and 10."""
    rounds = 12
    er, rmat = _er(), _rmat()
    one = _ca_ref("rmat", "sym", 1, rounds)
    cols = [_ca_ref("er", "wide", 2, rounds), _ca_ref("er", "sym", 3, rounds)]
    v_lossy = FAMILIES["wide"](rmat.n, seed=4)
    lossy_ref = oracle_lossy(*rmat.arrays(), v_lossy, rounds, hashed(LOSS, SEED, rmat.E))
    v_pair = FAMILIES["sym"](er.n, seed=5)
    pair_ref = oracle_pair(*er.arrays(), v_pair, rounds, SEED)
    ca = fu.CollectAll(rmat, one[0], kernel="stage")
    batch = fu.CollectAllBatch(er, np.stack([c[0] for c in cols], axis=1))
    lossy = fu.CollectAllLossy(rmat, v_lossy, loss=LOSS, seed=SEED)
    pair = fu.PairwiseSync(er, v_pair, seed=SEED)
    tg = tile_limit_graph()
    v_churn = FAMILIES["sym"](tg.n, seed=6)
    topo = {5: random_masks(tg, 0.2, 0.1, 31, keep=(tile_segment("heavy")[0],)), 10: random_masks(tg, 0.1, 0.2, 32)}
    script = [("run", 5), ("topology",) + topo[5], ("run", 5), ("topology",) + topo[10], ("run", 2)]
    churn_ref = churn_python(*tg.arrays(), v_churn, script)
    churn = fu.CollectAllChurn(tg, v_churn)
    engines = (ca, batch, lossy, pair)
    for turn in range(rounds):
        for eng in engines:
            eng.run(1)
        if turn in topo:
            churn.set_topology(*topo[turn])
        churn.run(1)
    assert [eng.rounds_done for eng in engines] == [rounds] * 4 and churn.rounds_done == rounds
    _check_ca(ca, one, ("CollectAll",))
    _check_batch(batch, cols, ("CollectAllBatch",))
    assert_same_bits(lossy.estimates(), lossy_ref[0], "CollectAllLossy estimates")
    assert_same_bits(lossy.flows(), lossy_ref[1], "CollectAllLossy flows")
    assert_same_bits(pair.estimates(), pair_ref[0], "PairwiseSync last")
    assert_same_bits(pair.flows(), pair_ref[1], "PairwiseSync flows")
    assert_same_bits(pair.cache(), pair_ref[2], "PairwiseSync cache")
    assert_same_bits(churn.estimates(), churn_ref.a, "CollectAllChurn estimates")
    assert_same_bits(churn.flows(), churn_ref.f, "CollectAllChurn flows")
    assert np.array_equal(churn.slot_state(), churn_ref.state)
    assert churn.stats == (churn_ref.steps[-1].alive_nodes, churn_ref.steps[-1].live_slots)
    for eng in engines + (churn,):
        eng.close()


# ------------------------------------------------------------------------------------
# 2. handles created and destroyed beside queued rounds
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("b_graph", ["rmat", "er"])
def test_create_and_destroy_beside_queued_rounds(b_graph):
    """A (CollectAll, RMAT) has run(200) queued and is not synchronised. B is created (on A's
    graph, or on another), runs 5 rounds, is read back and closed; C (a batch handle) is created,
    runs 7 rounds and stays open; then A is read. A equals the oracle at round 200, B at 5, C
    at 7."""
    ref_a = _ca_ref("rmat", "wide", 6, 200)
    ref_b = _ca_ref(b_graph, "sym", 7, 5)
    cols = [_ca_ref("er", "sym", 8, 7), _ca_ref("er", "wide", 9, 7)]
    a = fu.CollectAll(_rmat(), ref_a[0], kernel="recon")
    a.run(200)
    b = fu.CollectAll(GRAPHS[b_graph](), ref_b[0], kernel="recon")
    b.run(5)
    _check_ca(b, ref_b, ("B", b_graph))
    b.close()
    c = fu.CollectAllBatch(_er(), np.stack([x[0] for x in cols], axis=1))
    c.run(7)
    assert a.rounds_done == 200
    _check_ca(a, ref_a, ("A beside B on", b_graph))
    _check_batch(c, cols, ("C",))
    c.close()
    a.close()


# ------------------------------------------------------------------------------------
# 3. reset and readback beside another handle's rounds
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["collectall", "batch"])
def test_reset_and_readback_beside_queued_rounds(kind):
    """A (CollectAll with the staged kernel, or a batch handle) has run(100) queued. B (the same
    type and graph, other values) runs run(3); flows(); reset(); run(2); estimates(). Then A runs
    run(1). A equals its reference at round 101, B at round 3 (the flows read in between) and at
    round 2."""
    g = _rmat()
    va, vb = FAMILIES["sym"](g.n, seed=10), FAMILIES["wide"](g.n, seed=11)
    if kind == "collectall":
        def make(v):
            return fu.CollectAll(g, v, kernel="stage")

        def ref(v, r):
            return coracle.ca_sync(*g.arrays(), v, r, nthreads=16)
    else:
        def make(v):
            return fu.CollectAllBatch(g, np.stack([v, -v], axis=1))

        def ref(v, r):
            cols = [coracle.ca_sync(*g.arrays(), x, r, nthreads=16) for x in (v, -v)]
            return np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1)
    a, b = make(va), make(vb)
    a.run(100)
    b.run(3)
    assert_same_bits(b.flows(), ref(vb, 3)[1], (kind, "B flows at 3"))
    b.reset()
    b.run(2)
    assert_same_bits(b.estimates(), ref(vb, 2)[0], (kind, "B estimates at 2"))
    a.run(1)
    assert a.rounds_done == 101 and b.rounds_done == 2
    a_ref = ref(va, 101)
    assert_same_bits(a.estimates(), a_ref[0], (kind, "A estimates at 101"))
    assert_same_bits(a.flows(), a_ref[1], (kind, "A flows at 101"))
    assert_same_bits(b.flows(), ref(vb, 2)[1], (kind, "B flows at 2"))
    a.close()
    b.close()


# ------------------------------------------------------------------------------------
# 4. two replays of one trace
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["collectall", "pairwise"])
def test_two_replays_of_one_trace_alternating(mode):
    """A persistent and a per-tick Replay over one Trace object (RR-4096, 80 ticks, tie order
    rand:3: the trace of test_value_domain.test_replay_value_families), with values of their own:
    each runs to tick 40 and then to tick 80, in turn. Both equal coracle.replay at tick 80."""
    g = fu.Graph.random_regular(4096, 8, seed=1)
    tr = fu.Trace(g.rowptr, g.col, mode, 80, "rand:3")
    t = tr.arrays()
    vs = [FAMILIES["sym"](tr.n, seed=12), FAMILIES["wide"](tr.n, seed=13)]
    reps = [fu.Replay(tr, vs[0], persistent=True), fu.Replay(tr, vs[1], persistent=False)]
    for tick in (40, 80):
        for rep in reps:
            rep.run(tick)
    for k, rep in enumerate(reps):
        want = coracle.replay(t["rowptr"], vs[k], t["tick_task_off"], t["tasks"], t["events"], t["out_ids"], tr.n_msgs)
        got = rep.state()
        for name, x, y in zip(("last", "flows", "est"), got, want):
            assert_same_bits(x, y, (mode, "persistent" if k == 0 else "per tick", name))
    for rep in reps:
        rep.close()
