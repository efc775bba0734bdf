"""Every engine against the reference's own Peer code on the fp64 value domain, with no oracle
in between: tests/golden/vd_*.npz (vd_cases) hold what `Peer.on_receive / tick / avg_and_send`
left on signed zeros, subnormals, values that overflow and non-finite inputs, and each kernel path
must give those bits (parity_util.assert_same_bits: signs of zeros and infinities count, NaN
exactly where the reference has NaN). test_value_domain_golden.py holds the oracles to the same
files on the CPU, so a disagreement here is the kernel's alone.

Here: CollectAll in 12 configurations, CollectAllBatch, the scalar CollectAllLossy, PairwiseSync,
the scalar CollectAllChurn, Replay and the drop-in Engine. The K-column handles CollectAllLossyBatch
and CollectAllChurnBatch (k_light_cols, k_heavy_cols, k_max_err_cols) are held to the same files
in test_rev_columns_value_domain_gpu.py.

Everything runs on hub_mix (2400 nodes: rows of 2101 and 130 slots, light rows, 142 isolated rows)
for at most 40 rounds, or on 12 and 32 actors for 120 ticks."""
import functools

import numpy as np
import pytest

import fu
import vd_cases
from conftest import write_deployment_xml
from parity_util import assert_same_bits
from rule_cases import DOWN, UP, churn_states_after_events, lost_before
from vd_cases import CA_FAMILIES, RULE_FAMILIES, TICK_CASES, py_float_dict

pytestmark = pytest.mark.gpu

# name: (kernel, layout, hub_threshold, options). The lowered thresholds (64, 300) move the row of
# 130 slots to the heavy launches and the row of 2101 slots to the mega-hub chains.
CA_CONFIGS = {
    **{f"{k}-{lay}": (k, lay, None, {}) for k in ("recon", "stage", "pregather") for lay in ("given", "degree")},
    "recon-block_heavy": ("recon", "given", None, {"wave_heavy": 0}),
    "pregather-two_pass": ("pregather", "given", None, {"lag": 0}),
    "pregather-iso_tiles": ("pregather", "given", None, {"iso_rows": 0}),
    **{f"{k}-low_thresholds": (k, "given", 64, {"mega_hub": 300}) for k in ("recon", "stage", "pregather")},
}


@functools.lru_cache(maxsize=None)
def _graph():
    d = vd_cases.ca("subn")
    g = fu.Graph.from_csr(d.rowptr, d.col)
    assert np.array_equal(g.rev, d.rev)
    return g


@pytest.mark.parametrize("family", CA_FAMILIES)
@pytest.mark.parametrize("config", sorted(CA_CONFIGS))
def test_collectall_equals_the_reference(config, family):
    """fu.CollectAll stopped and read back after 1, 3, 8 and 17 rounds: estimates and flows are the
    reference's after as many generations (make_golden.ca_sync). `huge` is the order test (row 0's
    2101-term chains of CA:106 and CA:110 overflow at an element that depends on the order),
    `special` puts an inf and then a NaN into those chains, `special_off` keeps NaN, both infinities
    and -0.0 beside 2254 finite rows, and the isolated rows hold what CA:106-113 make of -0.0
    (+0.0), 5e-324, -5e-324, +inf and NaN. hub_mix gives kernel 8 a slice layout, so "stage" runs
    its own rounds here."""
    kernel, layout, hub_threshold, opts = CA_CONFIGS[config]
    d = vd_cases.ca(family)
    eng = fu.CollectAll(_graph(), d.values, kernel=kernel, layout=layout, hub_threshold=hub_threshold)
    try:
        for key, val in opts.items():
            eng.set_option(key, val)
        for q, stop in enumerate(d.stops):
            eng.run(stop - eng.rounds_done)
            assert_same_bits(eng.estimates(), d.last_avg[q], (config, family, stop, "estimates"))
            assert_same_bits(eng.flows(), d.flows[q], (config, family, stop, "flows"))
        assert eng.info()["kernel"] == kernel
    finally:
        eng.close()


def test_batch_columns_equal_their_own_reference_runs():
    """The five families as the K = 5 columns of one fu.CollectAllBatch run: each column is its
    own reference run, and the NaN and infinities of `huge`, `special` and `special_off` stay in
    their columns (`subn` and `wide` hold none at any stop)."""
    fams = [vd_cases.ca(f) for f in CA_FAMILIES]
    v = np.stack([d.values for d in fams], axis=1)
    with fu.CollectAllBatch(_graph(), v) as eng:
        for q, stop in enumerate(fams[0].stops):
            eng.run(stop - eng.rounds_done)
            a, f = eng.estimates(), eng.flows()
            for k, d in enumerate(fams):
                assert d.stops[q] == stop
                assert_same_bits(np.ascontiguousarray(a[:, k]), d.last_avg[q], (d.family, stop, "estimates"))
                assert_same_bits(np.ascontiguousarray(f[:, k]), d.flows[q], (d.family, stop, "flows"))
                if d.family in ("subn", "wide"):
                    assert np.isfinite(a[:, k]).all() and np.isfinite(f[:, k]).all(), (d.family, stop)
                elif stop == d.stops[-1]:
                    assert np.isnan(a[:, k]).any(), (d.family, stop)


@pytest.mark.parametrize("family", RULE_FAMILIES)
def test_lossy_equals_the_reference_under_recorded_loss(family):
    """fu.CollectAllLossy at the recorded (p, seed) and `down` mask: a receiver that misses a
    message fires on the pair it stored itself (CA:117-119), here also where that stored flow is
    -0.0, an infinity or NaN."""
    d, g = vd_cases.rule("lossy", family)
    with fu.CollectAllLossy(rowptr=g.rowptr, col=g.col, rev=g.rev, values=d.values) as eng:
        eng.set_loss(g.loss, g.seed)
        eng.set_link_mask(g.down)
        for q, stop in enumerate(d.stops):
            eng.run(stop - eng.rounds_done)
            assert_same_bits(eng.estimates(), d.last_avg[q], (family, stop, "estimates"))
            assert_same_bits(eng.flows(), d.flows[q], (family, stop, "flows"))
            assert eng.stats == (g.E * (stop - 1), lost_before(g, stop)), stop


@pytest.mark.parametrize("match", [0, 1])
@pytest.mark.parametrize("family", RULE_FAMILIES)
def test_pair_equals_the_reference_over_recorded_matching(family, match):
    """fu.PairwiseSync at the recorded seed: last averages, flows and the estimate cache after 5,
    20 and 40 rounds (PW:93-117 on each matched pair); a node that never fired holds +0.0."""
    d, g = vd_cases.rule("pair", family)
    with fu.PairwiseSync(rowptr=g.rowptr, col=g.col, rev=g.rev, values=d.values, seed=g.seed) as eng:
        eng.set_option("match", match)
        for q, stop in enumerate(d.stops):
            eng.run(stop - eng.rounds_done)
            assert_same_bits(eng.estimates(), d.last_avg[q], (family, match, stop, "last"))
            assert_same_bits(eng.flows(), d.flows[q], (family, match, stop, "flows"))
            assert_same_bits(eng.cache(), d.estimates[q], (family, match, stop, "cache"))
            assert eng.stats[0] == int(g.initiator[:stop].sum()), stop


@pytest.mark.parametrize("family", RULE_FAMILIES)
def test_churn_equals_the_reference_through_recorded_topologies(family):
    """fu.CollectAllChurn through the recorded set_topology events: a FRESH slot starts from the
    defaultdict zeros (CA:33-34), a dead node keeps its last average, an alive node without a live
    slot holds (v - 0) + 0.0 (CA:106-113), all of it on values where the sign of a zero shows; the
    slot states are the recorded live and fresh masks."""
    d, g = vd_cases.rule("churn", family)
    after_event = churn_states_after_events(g)
    with fu.CollectAllChurn(rowptr=g.rowptr, col=g.col, rev=g.rev, values=d.values) as eng:
        assert np.array_equal(eng.slot_state(), after_event[0])
        for q, stop in enumerate(d.stops):
            if q:
                eng.set_topology(g.alive[q], g.link_up[q])
                assert g.event_rounds[q] == eng.rounds_done
                assert np.array_equal(eng.slot_state(), after_event[q]), ("after the event before round", eng.rounds_done)
            eng.run(stop - eng.rounds_done)
            assert_same_bits(eng.estimates(), d.last_avg[q], (family, stop, "estimates"))
            assert_same_bits(eng.flows(), d.flows[q], (family, stop, "flows"))
            assert np.array_equal(eng.slot_state(), np.where(g.live[q], UP, DOWN)), stop


@pytest.mark.parametrize("persistent", [False, True, "noreg"])
@pytest.mark.parametrize("graph,mode", TICK_CASES)
def test_replay_equals_the_reference_tick_by_tick(graph, mode, persistent):
    """fu.Replay on the planted actors: global_values["last_avg"] after every one of the 120 ticks,
    then every flow and cached estimate, as the reference's Peers left them under the tick
    emulation (a receive negates the flow, CA:99: -(-0.0), -(inf), -(NaN))."""
    d = vd_cases.tick(graph, mode)
    tr = vd_cases.tick_trace(d)
    rep = fu.Replay(tr, d.values, persistent=bool(persistent), registers=persistent != "noreg")
    try:
        snaps = rep.run(d.ticks, snapshot_ticks=range(d.ticks))
        last, flows, est = rep.state()
    finally:
        rep.close()
    assert np.array_equal(tr.arrays()["col"], d.union_col)
    for t in range(d.ticks):
        keys = d.key_order[:d.n_keys[t]]
        assert_same_bits(snaps[t][keys], d.snaps[t][keys], (graph, mode, persistent, "tick", t))
    assert_same_bits(last, d.snaps[-1], (graph, mode, persistent, "last"))
    assert_same_bits(flows, d.flows, (graph, mode, persistent, "flows"))
    assert_same_bits(est, d.estimates, (graph, mode, persistent, "estimates"))


@pytest.mark.parametrize("mode", ["ca", "pw"])
def test_engine_watcher_prints_the_reference_floats(tmp_path, mode):
    """fu.Engine on the asym12 actors with planted values: the watcher's `value{...}` and
    `last_avg{...}` lines (CA:134-136) at t = 10 ... 110 are str() of a dict of the reference's
    floats, so nan, inf, -0.0 and 5e-324 print as Python prints them."""
    d = vd_cases.tick("asym12", mode)
    dep = tmp_path / "actors.xml"
    nbrs = [",".join(d.names[c] for c in d.decl_col[d.decl_rowptr[i]:d.decl_rowptr[i + 1]]) for i in range(d.n)]
    write_deployment_xml(dep, list(zip(d.names, d.value_strs, nbrs)))
    e = fu.Engine([], order=d.order, out=False)
    e.register_actor("peer", fu.CollectAllPeer if mode == "ca" else fu.PairwisePeer)
    e.load_deployment(str(dep))
    e.add_watcher(110.0, 10.0)
    e.run_until(10000)
    by_t = {}
    for ln in e.lines:
        if ":watcher:" in ln and ("last_avg{" in ln or "value{" in ln):
            by_t.setdefault(float(ln.split()[1].rstrip("]")), []).append(ln.split("] ", 2)[2])
    value_line = "value" + py_float_dict(d.names, d.values)
    assert "nan" in value_line and "inf" in value_line and "-0.0" in value_line and "5e-324" in value_line
    seen = ""
    for t in range(10, 111, 10):
        keys = d.key_order[:d.n_keys[t]]
        want = [value_line] + (["last_avg" + py_float_dict([d.names[k] for k in keys], d.snaps[t][keys])] if len(keys) else [])
        assert by_t[float(t)] == want, t
        seen += want[-1]
    assert "nan" in seen and "inf" in seen
