"""The rules of the lossy, pair and churn engines against the reference's own Peer methods.

tests/golden/rule_{lossy,pair,churn}_hub_mix.npz were made by make_golden.py's ca_lossy_sync,
pw_sync and ca_churn_sync, which drive `Peer.on_receive / tick / avg_and_send` of the reference
and restate none of their arithmetic. Here every restatement that the GPU tests of the three
engines compare with (lossy_cases, pair_cases, churn_cases) must give those recordings by bit
pattern at every stop, the engines' host-only decisions (fu.lossy_delivered, fu.pair_matching,
fu.churn_live) must give the recorded masks, matchings and live slots, and the recorded inputs
must reach what they were picked to reach. No GPU; tests/golden/ only."""
import numpy as np
import pytest

import fu
from churn_cases import churn_python
from lossy_cases import lossy_python, oracle_lossy
from pair_cases import Recorded, oracle_pair, pair_python
from parity_util import assert_same_bits
from rule_cases import DOWN, FRESH, UP, churn_script, churn_states_after_events, load, row


# ------------------------------------------------------------------------------------
# the graph
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lossy", "pair", "churn"])
def test_hub_mix(kind):
    d = load(kind)
    deg = np.diff(d.rowptr)
    assert (d.n, d.E) == (2400, 6860) and deg[0] == 2101 and deg[1] == 130
    assert int(deg[2:].max()) < 64 and not deg[2350:].any() and (deg[2:2102] >= 1).all()
    assert int(deg.sum()) - 2 * (1 + 2100 + 129) == 2 * 1200  # the random links, none of them twice
    assert list(d.col[row(d, 0)]) == list(range(1, 2102)) and list(d.col[row(d, 1)]) == [0] + list(range(2, 131))
    for i in range(d.n):
        assert (np.diff(d.col[row(d, i)]) > 0).all()  # rows sorted by id
    g = fu.Graph.from_csr(d.rowptr, d.col)
    assert np.array_equal(g.rev, d.rev)
    assert ((d.values >= 0) & (d.values < 100)).all()
    a = load("lossy")
    assert all(np.array_equal(getattr(a, k), getattr(d, k)) for k in ("rowptr", "col", "values"))


# ------------------------------------------------------------------------------------
# lossy
# ------------------------------------------------------------------------------------
def test_lossy_mask_is_the_engines_decision():
    d = load("lossy")
    assert d.loss == 0.25 and d.stops == [3, 12, 30] and len(d.delivered) == 30
    assert not d.delivered[0].any()
    assert np.array_equal(d.down != 0, d.down[d.rev] != 0)
    links_down = int((d.down != 0).sum()) // 2
    assert 0.03 * d.E / 2 <= links_down <= 0.07 * d.E / 2
    for r in range(1, 30):
        want = fu.lossy_delivered(d.seed, r, 0, d.E, d.loss).astype(bool) & (d.down == 0)
        assert np.array_equal(d.delivered[r], want), r


def test_lossy_inputs():
    d = load("lossy")
    D = d.delivered[1:]
    for hub, edge in ((0, 2048), (1, 128)):
        r = D[:, row(d, hub)]
        lo, hi = r[:, :edge], r[:, edge:]
        both = (~lo).any(1) & (~hi).any(1) & lo.any(1) & hi.any(1)
        assert both.any(), hub  # one round loses and receives on each side of the edge
    deg = np.diff(d.rowptr)
    src = np.repeat(np.arange(d.n), deg)
    got = np.stack([np.bincount(src, weights=x, minlength=d.n) for x in D])  # delivered per node and round
    assert ((got == 0) & (deg >= 1)).any() and ((got == 0) & (deg >= 2)).any()  # a node loses every message
    assert ((got == deg) & (deg >= 2)).any()  # a node loses none
    twice = ~D[:-1] & ~D[1:]
    assert (twice & (d.down == 0)).any()  # lost twice running by the hash alone: the stored pair is a timeout product
    assert (twice[:, row(d, 0)]).any() and (twice[:, row(d, 1)]).any()


@pytest.mark.parametrize("restatement", ["python", "coracle"])
def test_lossy_restatements_equal_the_reference(restatement):
    d = load("lossy")
    delivered = lambda r: d.delivered[r]  # noqa: E731
    for q, stop in enumerate(d.stops):
        if restatement == "python":
            a, f = lossy_python(d.rowptr, d.col, d.rev, d.values, stop, delivered)
        else:
            a, f, _ = oracle_lossy(d.rowptr, d.col, d.rev, d.values, stop, delivered)
        assert_same_bits(a, d.last_avg[q], (restatement, stop, "estimates"))
        assert_same_bits(f, d.flows[q], (restatement, stop, "flows"))


# ------------------------------------------------------------------------------------
# pair
# ------------------------------------------------------------------------------------
def test_pair_matching_is_the_engines():
    d = load("pair")
    assert d.stops == [5, 20, 40] and d.mate.shape == (40, d.n) and d.initiator.shape == (40, d.n)
    for r in range(40):
        mate, ini = fu.pair_matching((d.rowptr, d.col), d.seed, r)
        assert np.array_equal(mate, d.mate[r]) and np.array_equal(ini, d.initiator[r]), r


def test_pair_inputs():
    d = load("pair")
    rec = Recorded(d.mate, d.initiator)
    pairs = [p for r in range(40) for p in rec.pairs(d.rowptr, d.col, d.rev, r)]
    for hub in (0, 1):
        assert sum(i == hub for i, _, _, _ in pairs) >= 3, hub
        assert sum(j == hub for _, _, j, _ in pairs) >= 3, hub
    ts = [t for _, _, j, t in pairs if j == 0]
    assert min(ts) < 1024 <= max(ts)  # node 0 answers in both 1024-slot chunks
    ss = [s for i, s, _, _ in pairs if i == 0]
    assert min(ss) < 1024 <= max(ss)
    assert any(t >= 64 for _, _, j, t in pairs if j == 1) or any(s >= 64 for i, s, _, _ in pairs if i == 1)


@pytest.mark.parametrize("restatement", ["python", "coracle"])
def test_pair_restatements_equal_the_reference(restatement):
    d = load("pair")
    rec = Recorded(d.mate, d.initiator)
    fn = pair_python if restatement == "python" else oracle_pair
    for q, stop in enumerate(d.stops):
        last, f, c = fn(d.rowptr, d.col, d.rev, d.values, stop, rec)[:3]
        assert_same_bits(last, d.last_avg[q], (restatement, stop, "last"))
        assert_same_bits(f, d.flows[q], (restatement, stop, "flows"))
        assert_same_bits(c, d.estimates[q], (restatement, stop, "cache"))


# ------------------------------------------------------------------------------------
# churn
# ------------------------------------------------------------------------------------
def test_churn_live_slots_are_the_engines():
    d = load("churn")
    assert d.stops == [8, 16, 24, 32] and d.event_rounds == [0, 8, 16, 24]
    assert d.alive[0].all() and d.link_up[0].all() and d.alive[3].all() and d.link_up[3].all()
    for e in range(4):
        live = fu.churn_live((d.rowptr, d.col, d.rev), d.alive[e], d.link_up[e]).astype(bool)
        assert np.array_equal(live, d.live[e]), e
        before = d.live[e - 1] if e else np.zeros(d.E, dtype=bool)
        assert np.array_equal(d.fresh[e], live & ~before), e  # the entries the driver created


def test_churn_inputs():
    d = load("churn")
    st = churn_states_after_events(d)
    dead8, dead16 = d.alive[1] == 0, d.alive[2] == 0
    assert 0.07 * d.n <= dead8.sum() <= 0.13 * d.n and dead8[1] and not dead8[0]
    assert dead16[0] and not dead16[1] and (dead16 & ~dead8).sum() >= 0.05 * d.n and not (dead16 & dead8).any()
    cut8 = int((d.link_up[1] == 0).sum()) // 2
    assert 0.03 * d.E / 2 <= cut8 <= 0.08 * d.E / 2 and d.link_up[2].all()
    r0, r1 = row(d, 0), row(d, 1)
    assert (d.link_up[1][r0[[2046, 2047, 2048, 2100]]] == 0).all() and d.alive[1][d.col[r0[[2046, 2047, 2048, 2100]]]].all()
    # before round 16: node 1's live slots are FRESH, on both sides of slot 128, while node 0's are DOWN
    assert (st[2][r0] == DOWN).all()
    s1 = st[2][r1]
    assert set(s1.tolist()) == {DOWN, FRESH} and (s1 == FRESH).sum() >= 100 and (s1[128:] == FRESH).any() and s1[0] == DOWN
    # an alive node without a live slot in rounds 8-15
    deg_live = np.bincount(np.repeat(np.arange(d.n), np.diff(d.rowptr)), weights=d.live[1], minlength=d.n)
    assert ((deg_live == 0) & (d.alive[1] != 0) & (np.diff(d.rowptr) >= 2)).any()
    # UP -> DOWN -> FRESH -> UP: live in rounds 0-7, not in 8-15, fresh at 16 or at 24
    assert (d.live[0] & ~d.live[1] & d.fresh[2]).any() and (d.live[0] & ~d.live[1] & ~d.live[2] & d.fresh[3]).any()
    assert (st[1][r0[:2048]] == DOWN).any() and (st[1][r0[2048:]] == DOWN).any() and (st[1][r0] == UP).sum() > 1500
    assert (st[3][r0] == FRESH).all()


def test_churn_restatement_equals_the_reference():
    d = load("churn")
    res = churn_python(d.rowptr, d.col, d.rev, d.values, churn_script(d, 32))
    for q, stop in enumerate(d.stops):
        assert_same_bits(res.a_rounds[stop - 1], d.last_avg[q], (stop, "estimates"))
        assert_same_bits(res.f_rounds[stop - 1], d.flows[q], (stop, "flows"))
    e = 0
    for step, got in zip(churn_script(d, 32), res.steps):
        if step[0] == "topology":
            e += 1
            assert np.array_equal(got.state, churn_states_after_events(d)[e]), e
            assert (got.alive_nodes, got.live_slots) == (int((d.alive[e] != 0).sum()), int(d.live[e].sum()))
