"""The oracles and restatements against the reference's own Peer code on the fp64 value domain.

tests/golden/vd_*.npz (vd_cases) were made by make_golden.value_domain_fixtures: the reference's
`Peer.on_receive / tick / avg_and_send` on signed zeros, subnormals, values that overflow and
non-finite inputs, through the generation-synchronous driver, the lossy, pair and churn drivers and
the tick emulation. Every oracle that a GPU test compares with (oracle.ca_sync, coracle.ca_sync /
ca_rounds, lossy_python, oracle_lossy, pair_python, oracle_pair, churn_python, oracle.replay_trace,
coracle.replay) must give those recordings by bit pattern, and the recordings must reach what they
were made to reach: the conditions below are on the reference's output, read from the files alone.
No GPU.

What the reference makes of the hand-derived cases (all of them as the restatements had them):
an isolated node with input -0.0 holds +0.0 (CA:106 sum() of nothing is int 0, CA:107 -0.0 - 0 =
-0.0, CA:113 (-0.0 + 0.0) / 1 = +0.0), one with 5e-324, -5e-324, +inf or NaN holds its input; a
churn node without a live slot does the same in every round it is alive."""
import os

import numpy as np
import pytest

import coracle
import oracle
import vd_cases
from churn_cases import churn_python
from conftest import GOLDEN, load_manifest, trace_events_as_log
from lossy_cases import lossy_python, oracle_lossy
from pair_cases import Recorded, oracle_pair, pair_python
from parity_util import assert_same_bits
from rule_cases import churn_script
from vd_cases import CA_FAMILIES, RULE_FAMILIES, RULE_KINDS, TICK_CASES, counts, is_neg_zero

MAX_FIXTURE_BYTES = 452_000  # make_golden.MAX_FIXTURE_BYTES


# ------------------------------------------------------------------------------------
# the files
# ------------------------------------------------------------------------------------
def _entries():
    m = vd_cases.manifest()
    return [e for part in ("ca", "rule", "tick") for e in m[part].values()]


def test_manifest_lists_exactly_the_files_present():
    m = vd_cases.manifest()
    assert sorted(m["ca"]) == sorted(CA_FAMILIES)
    assert sorted(m["rule"]) == sorted(f"{k}_{f}" for k in RULE_KINDS for f in RULE_FAMILIES)
    assert sorted(m["tick"]) == sorted(f"{g}_{mode}" for g, mode in TICK_CASES)
    listed = sorted(e["file"] for e in _entries())
    assert listed == sorted(fn for fn in os.listdir(GOLDEN) if fn.startswith("vd_"))
    earlier = load_manifest()
    assert not set(listed) & {e["file"] for e in earlier["ca_sync"].values()} and not set(listed) & set(earlier["tick"].values())
    for fn in listed:
        assert os.path.getsize(os.path.join(GOLDEN, fn)) <= MAX_FIXTURE_BYTES, fn


def test_every_float_is_stored_as_bits():
    for e in _entries():
        d = np.load(os.path.join(GOLDEN, e["file"]), allow_pickle=False)
        for k in d.files:
            assert d[k].dtype.kind in "iuU", (e["file"], k, d[k].dtype)
            assert (d[k].dtype == np.uint64) == (k in vd_cases.FLOATS), (e["file"], k)


def test_manifest_counts_are_the_files():
    m = vd_cases.manifest()
    for family in CA_FAMILIES:
        d = vd_cases.ca(family)
        want = {str(s): {"estimates": counts(d.last_avg[q]), "flows": counts(d.flows[q])} for q, s in enumerate(d.stops)}
        got = {str(int(r) + 1): c for r, c in m["ca"][family]["counts"].items()}  # the manifest keys are the round keys
        assert got == want, family
    for kind in RULE_KINDS:
        for family in RULE_FAMILIES:
            d, _ = vd_cases.rule(kind, family)
            want = {str(s): {"estimates": counts(d.last_avg[q]), "flows": counts(d.flows[q])} for q, s in enumerate(d.stops)}
            assert m["rule"][f"{kind}_{family}"]["counts"] == want, (kind, family)


# ------------------------------------------------------------------------------------
# the inputs
# ------------------------------------------------------------------------------------
def test_family_inputs():
    d = vd_cases.ca("subn")
    k = d.values / 5e-324
    assert (k == np.round(k)).all() and (np.abs(k) <= 50).all() and (k < 0).any() and (k > 0).any()
    z = d.values == 0.0
    assert is_neg_zero(d.values[z]).any() and (~is_neg_zero(d.values[z])).any() and sorted(d.planted) == sorted(np.flatnonzero(z))
    d = vd_cases.ca("huge")
    assert (np.abs(d.values) <= 1.7e308).all() and (np.abs(d.values) > 1e308).sum() > 500 and (d.values < 0).any()
    d = vd_cases.ca("wide")
    assert (np.abs(d.values) >= 2.0 ** -60).all() and (np.abs(d.values) <= 2.0 ** 60).all()
    assert (np.abs(d.values) < 2.0 ** -50).any() and (np.abs(d.values) > 2.0 ** 50).any() and (d.values < 0).any()


def _hub_component(d):
    seen = np.zeros(d.n, dtype=bool)
    seen[0] = True
    todo = [0]
    while todo:
        i = todo.pop()
        for c in d.col[d.rowptr[i]:d.rowptr[i + 1]]:
            if not seen[c]:
                seen[c] = True
                todo.append(int(c))
    return seen


@pytest.mark.parametrize("family", ["special", "special_off"])
def test_special_plantings(family):
    d = vd_cases.ca(family)
    deg = np.diff(d.rowptr)
    hubc = _hub_component(d)
    p = np.zeros(d.n, dtype=bool)
    p[d.planted] = True
    rest = d.values[~p]
    assert ((rest >= 0) & (rest < 100) & ~is_neg_zero(rest)).all()
    small = [i for i in range(d.n) if not hubc[i] and deg[i] >= 1]  # two components of two nodes
    iso = [i for i in d.planted if deg[i] == 0]
    leaf = [i for i in d.planted if hubc[i]]
    assert len(small) == 4 and all(deg[i] == 1 for i in small) and set(small) <= set(d.planted)
    a, c = small[0], [i for i in small[1:] if i != d.col[d.rowptr[small[0]]]][0]
    assert_same_bits(d.values[[a, d.col[d.rowptr[a]], c, d.col[d.rowptr[c]]]], np.array([-0.0, np.inf, -np.inf, np.nan]))
    assert_same_bits(d.values[iso], np.array([-0.0, 5e-324, -5e-324, np.inf, np.nan]))
    if family == "special":
        (i,) = leaf
        assert deg[i] == 1 and d.col[d.rowptr[i]] == 0 and np.isposinf(d.values[i])
    else:
        assert not leaf
        both = vd_cases.ca("special")
        same = np.ones(d.n, dtype=bool)
        same[np.setdiff1d(both.planted, d.planted)] = False
        assert_same_bits(d.values[same], both.values[same])


# ------------------------------------------------------------------------------------
# the conditions on the reference's output
# ------------------------------------------------------------------------------------
def test_subn_reaches_negative_zero():
    d = vd_cases.ca("subn")
    assert d.stops == [1, 3, 8, 17]
    assert counts(d.last_avg[-1])[0] >= 1 and counts(d.flows[-1])[0] >= 1


def test_huge_overflows_both_ways():
    d = vd_cases.ca("huge")
    assert np.isposinf(d.flows).any() and np.isneginf(d.flows).any() and np.isnan(d.last_avg).any()
    # and row 0's 2101-term chains are among them while its neighbours still hold finite values
    assert not np.isfinite(d.last_avg[1][0]) and np.isfinite(d.last_avg[0]).all()


def test_special_conditions():
    d = vd_cases.ca("special")
    assert np.isnan(d.last_avg[-1]).any()
    iso = [i for i in d.planted if d.rowptr[i] == d.rowptr[i + 1]]
    # what the reference makes of an isolated node's input: -0.0 becomes +0.0, the others stay
    assert_same_bits(d.values[iso], np.array([-0.0, 5e-324, -5e-324, np.inf, np.nan]))
    for q in range(len(d.stops)):
        assert_same_bits(d.last_avg[q][iso], np.array([0.0, 5e-324, -5e-324, np.inf, np.nan]), d.stops[q])
    # the hub-leaf inf reaches row 0: finite after round 0, never again
    assert np.isfinite(d.last_avg[0][0]) and not np.isfinite(d.last_avg[1:, 0]).any()
    assert np.isposinf(d.last_avg[1][0]) and np.isnan(d.flows[1][d.rowptr[0]:d.rowptr[1]]).sum() == 1
    # ... and takes the component with it, which is why special_off exists (vd_cases)
    assert np.isfinite(d.last_avg[-1]).sum() < 1000 and np.isfinite(d.last_avg[0]).sum() >= 1000


def test_special_off_conditions():
    d = vd_cases.ca("special_off")
    assert np.isnan(d.last_avg[-1]).any() and np.isfinite(d.last_avg[-1]).sum() >= 1000
    iso = [i for i in d.planted if d.rowptr[i] == d.rowptr[i + 1]]
    assert is_neg_zero(d.values[iso[0]]) and not is_neg_zero(d.last_avg[-1][iso[0]]) and d.last_avg[-1][iso[0]] == 0.0
    assert np.isfinite(d.last_avg[:, _hub_component(d)]).all()


@pytest.mark.parametrize("family", RULE_FAMILIES)
def test_lossy_loses_on_an_odd_stored_flow(family):
    """A message is lost in the round after a stop on a slot whose stored flow, read at that stop,
    is -0.0 or non-finite: the receiver fires on that stored flow (CA:117-119)."""
    d, g = vd_cases.rule("lossy", family)
    odd = is_neg_zero(d.flows) | ~np.isfinite(d.flows)
    hits = [int((odd[q] & ~g.delivered[s] & (g.down == 0)).sum()) for q, s in enumerate(d.stops[:-1])]
    assert max(hits) >= 1, hits


@pytest.mark.parametrize("family", RULE_FAMILIES)
def test_pair_matches_a_planted_node_and_leaves_one_unfired(family):
    d, g = vd_cases.rule("pair", family)
    assert (g.mate[:, d.planted] >= 0).any()
    never = (g.mate < 0).all(axis=0)
    assert never.any() and (d.last_avg[-1][never].view(np.uint64) == 0).all()  # +0.0: PW:37, never assigned


@pytest.mark.parametrize("family", RULE_FAMILIES)
def test_churn_has_a_fresh_slot_and_a_dead_node_among_the_planted(family):
    d, g = vd_cases.rule("churn", family)
    p = np.zeros(g.n, dtype=bool)
    p[d.planted] = True
    src = np.repeat(np.arange(g.n), np.diff(g.rowptr))
    assert (g.fresh[1:] & (p[src] | p[g.col])).any()
    assert (g.alive[:, d.planted] == 0).any()
    if family == "special":  # the node beside node 0 that holds +inf dies before round 8; its slot is FRESH before round 24
        leaf = [i for i in d.planted if g.rowptr[i + 1] - g.rowptr[i] == 1 and g.col[g.rowptr[i]] == 0]
        assert leaf and g.alive[1][leaf[0]] == 0 and g.fresh[3][g.rowptr[leaf[0]]]


def test_tick_dynamic_addition_carries_a_planted_value():
    """CA:94-96 / PW:94-96: a message from an undeclared sender adds it; in the asymmetric case
    one such message comes from a planted node and carries a non-finite, zero or subnormal estimate."""
    for mode in ("ca", "pw"):
        d = vd_cases.tick("asym12", mode)
        decl = [set(d.decl_col[d.decl_rowptr[i]:d.decl_rowptr[i + 1]]) for i in range(d.n)]
        first = {}
        for t, i, kind, s in d.events:
            if kind == 0 and s not in decl[i]:
                first.setdefault((int(i), int(s)), int(t))
        assert sorted((t, i, s) for (i, s), t in first.items()) == sorted(tuple(int(x) for x in r) for r in d.dyn)
        assert len(d.dyn) == d.errors_logged >= 1
        es = d.dyn_payload[:, 1]
        ordinary = np.isfinite(es) & (np.abs(es) >= 2.0 ** -1022)
        assert (np.isin(d.dyn[:, 2], d.planted) & ~ordinary).any(), mode


def test_tick_inputs():
    for graph, mode in TICK_CASES:
        d = vd_cases.tick(graph, mode)
        assert (d.ticks, d.order) == (120, "rand:11") and d.snaps.shape == (120, d.n)
        assert_same_bits(np.array([float(s) for s in d.value_strs]), d.values, (graph, mode))
        assert [repr(float(x)) for x in d.values] == d.value_strs
        pv = d.values[d.planted]
        assert is_neg_zero(pv).any() and np.isposinf(pv).any() and np.isnan(pv).any() and (np.abs(pv) == 5e-324).sum() == 2
        assert np.isnan(d.snaps[-1]).any()


# ------------------------------------------------------------------------------------
# the oracles
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", CA_FAMILIES)
def test_python_oracle_ca_sync(family):
    d = vd_cases.ca(family)
    with np.errstate(over="ignore", invalid="ignore"):  # the overflow and the inf - inf are the point
        snaps = oracle.ca_sync(d.rowptr, d.col, d.values, d.stops[-1], rev=d.rev, snapshot_rounds=[s - 1 for s in d.stops])
    for q, s in enumerate(d.stops):
        assert_same_bits(snaps[s - 1][0], d.last_avg[q], (family, s, "estimates"))
        assert_same_bits(snaps[s - 1][1], d.flows[q], (family, s, "flows"))


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("family", CA_FAMILIES)
def test_c_oracle_ca_sync_and_resumed_rounds(family, threads):
    d = vd_cases.ca(family)
    a = f = None
    done = 0
    for q, s in enumerate(d.stops):
        a1, f1 = coracle.ca_sync(d.rowptr, d.col, d.rev, d.values, s, threads)
        assert_same_bits(a1, d.last_avg[q], (family, s, "estimates"))
        assert_same_bits(f1, d.flows[q], (family, s, "flows"))
        if a is None:
            a, f = a1.copy(), f1.copy()
        else:
            coracle.ca_rounds(d.rowptr, d.col, d.rev, d.values, s - done, a, f, threads)
            assert_same_bits(a, d.last_avg[q], (family, s, "estimates, resumed"))
            assert_same_bits(f, d.flows[q], (family, s, "flows, resumed"))
        done = s


@pytest.mark.parametrize("restatement", ["python", "coracle"])
@pytest.mark.parametrize("family", RULE_FAMILIES)
def test_lossy_restatements_equal_the_reference(family, restatement):
    d, g = vd_cases.rule("lossy", family)
    delivered = lambda r: g.delivered[r]  # noqa: E731
    for q, stop in enumerate(d.stops):
        if restatement == "python":
            a, f = lossy_python(g.rowptr, g.col, g.rev, d.values, stop, delivered)
        else:
            a, f, _ = oracle_lossy(g.rowptr, g.col, g.rev, d.values, stop, delivered)
        assert_same_bits(a, d.last_avg[q], (family, restatement, stop, "estimates"))
        assert_same_bits(f, d.flows[q], (family, restatement, stop, "flows"))


@pytest.mark.parametrize("restatement", ["python", "coracle"])
@pytest.mark.parametrize("family", RULE_FAMILIES)
def test_pair_restatements_equal_the_reference(family, restatement):
    d, g = vd_cases.rule("pair", family)
    rec = Recorded(g.mate, g.initiator)
    fn = pair_python if restatement == "python" else oracle_pair
    for q, stop in enumerate(d.stops):
        last, f, c = fn(g.rowptr, g.col, g.rev, d.values, stop, rec)[:3]
        assert_same_bits(last, d.last_avg[q], (family, restatement, stop, "last"))
        assert_same_bits(f, d.flows[q], (family, restatement, stop, "flows"))
        assert_same_bits(c, d.estimates[q], (family, restatement, stop, "cache"))


@pytest.mark.parametrize("family", RULE_FAMILIES)
def test_churn_restatement_equals_the_reference(family):
    d, g = vd_cases.rule("churn", family)
    res = churn_python(g.rowptr, g.col, g.rev, d.values, churn_script(g, d.stops[-1]))
    for q, stop in enumerate(d.stops):
        assert_same_bits(res.a_rounds[stop - 1], d.last_avg[q], (family, stop, "estimates"))
        assert_same_bits(res.f_rounds[stop - 1], d.flows[q], (family, stop, "flows"))


@pytest.mark.parametrize("which", ["python", "coracle"])
@pytest.mark.parametrize("graph,mode", TICK_CASES)
def test_replay_oracles_equal_the_reference(graph, mode, which):
    d = vd_cases.tick(graph, mode)
    tr = vd_cases.tick_trace(d)
    a = tr.arrays()
    assert trace_events_as_log(a) == [[int(x) for x in e] for e in d.events]
    assert np.array_equal(a["rowptr"], d.union_rowptr) and np.array_equal(a["col"], d.union_col)
    assert tr.last_avg_order() == [int(i) for i in d.key_order] and tr.dynamic_additions == d.errors_logged
    ticks = list(range(d.ticks))
    args = (a["rowptr"], d.values, a["tick_task_off"], a["tasks"], a["events"], a["out_ids"], tr.n_msgs, ticks)
    last, flows, est, snaps = oracle.replay_trace(*args) if which == "python" else coracle.replay(*args)
    for t in ticks:
        keys = d.key_order[:d.n_keys[t]]
        assert_same_bits(snaps[t][keys], d.snaps[t][keys], (graph, mode, which, "tick", t))
    assert_same_bits(last, d.snaps[-1], (graph, mode, which, "last"))
    assert_same_bits(flows, d.flows, (graph, mode, which, "flows"))
    assert_same_bits(est, d.estimates, (graph, mode, which, "estimates"))
