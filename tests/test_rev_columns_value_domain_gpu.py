"""The K-column lossy and churn handles (fu.CollectAllLossyBatch, fu.CollectAllChurnBatch;
csrc/fu_rev_round.h k_light_cols, k_heavy_cols, k_max_err_cols) against the reference's own Peer
code on the fp64 value domain: signed zeros, subnormals, chains that overflow, infinities and NaN
as the columns of one handle. Every column of a recording equals tests/golden/vd_*.npz at every
recorded stop by bit pattern (parity_util.assert_same_bits: NaN exactly where the reference has
it); a filler column equals the Python rule run on it alone. No tolerance anywhere, and no
reference comes from the engine. tests/test_rev_columns_value_domain.py holds the Python rules
and the inputs' conditions on the CPU; tests/test_rev_columns_gpu.py covers widths, tile and chunk
edges, statistics and the scaffold on uniform values.

What uniform inputs cannot see and these do: -F written as 0.0 - F (the sign of a zero flow), a
masked load written as a product with 0 (inf or NaN behind a slot that does not gather), a zero
slot that yields -0.0 (only next to an estimate of -0.0), a chunk carry that adds in another order
(`huge` overflows at another element), a column that reads its neighbour's row estimate.

1. no loss, everything alive: the five collect-all families as columns at K = 2, 3, 5, 16, and
   through the scalar handles;
2. the recorded loss masks and the recorded topologies: subn and special at K = 2, 3, 16, first
   and last columns; the error reduction on these values;
3. subn, huge and planted +inf, -0.0 and NaN at the chunk edges of heavy rows at K = 2, 3, 16."""
import numpy as np
import pytest

import fu
import vd_cases
from lossy_cases import hashed
from parity_util import assert_same_bits
from rev_columns_cases import LOSS_SEED, drive_churn, heavy_boundary_script
from rev_columns_vd_cases import (CA_LAYOUTS, ENGINES, HEAVY_LAYOUTS, HEAVY_LOSS, HEAVY_STOPS, RULE_LAYOUTS, error_case,
                                  fillers, graph, heavy_churn_steps, heavy_columns, heavy_lossy_stops, layout, stops,
                                  vd_columns, wanted)
from rule_cases import DOWN, UP, churn_states_after_events, lost_before
from vd_cases import CA_FAMILIES

pytestmark = pytest.mark.gpu


def _open(engine, kind, values):
    """A handle of `engine` on the graph of `kind`: the batch class for (n, K) values, the scalar
    one for (n,)."""
    g = graph(kind)
    wide = np.ndim(values) == 2
    if engine == "lossy":
        return (fu.CollectAllLossyBatch if wide else fu.CollectAllLossy)(rowptr=g.rowptr, col=g.col, rev=g.rev, values=values)
    return (fu.CollectAllChurnBatch if wide else fu.CollectAllChurn)(rowptr=g.rowptr, col=g.col, rev=g.rev, values=values)


def _check_columns(eng, engine, kind, fams, q, what):
    """Every column after stop q: the recording, or the Python rule for a filler."""
    a, f = eng.estimates(), eng.flows()
    for c in range(a.shape[1]):
        want_a, want_f = wanted(engine, kind, fams, c, q)
        assert_same_bits(np.ascontiguousarray(a[:, c]), want_a, what + (c, fams.get(c, "filler"), "estimates"))
        assert_same_bits(np.ascontiguousarray(f[:, c]), want_f, what + (c, fams.get(c, "filler"), "flows"))
        if fams.get(c, "filler") in ("subn", "wide", "filler"):
            assert np.isfinite(a[:, c]).all() and np.isfinite(f[:, c]).all(), what + (c,)


# ------------------------------------------------------------------------------------
# 1. no loss, everything alive: the collect-all recordings
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CA_LAYOUTS))
@pytest.mark.parametrize("engine", ENGINES)
def test_lossless_columns_equal_the_collect_all_recordings(engine, name):
    """CollectAllLossyBatch at loss 0 and CollectAllChurnBatch without a topology call, stopped
    after 1, 3, 8 and 17 rounds. hub_mix's row of 2101 slots is 1024 + 1024 + 53 slots at K = 2,
    five chunks of 409 and one of 56 at K = 5, sixteen of 128 and one of 53 at K = 16, where the
    row of 130 slots is 128 + 2; `huge` is the order test of the chunk carry."""
    V, fams = layout("ca", CA_LAYOUTS[name])
    g = graph("ca")
    with _open(engine, "ca", V) as eng:
        for q, stop in enumerate(stops("ca")):
            eng.run(stop - eng.rounds_done)
            _check_columns(eng, engine, "ca", fams, q, (engine, name, stop))
            if engine == "lossy":
                assert eng.stats == (g.E * (stop - 1), 0), stop
            else:
                assert (eng.slot_state() == UP).all() and eng.stats == (g.n, g.E), stop


@pytest.mark.parametrize("family", CA_FAMILIES)
@pytest.mark.parametrize("engine", ENGINES)
def test_scalar_handles_equal_the_collect_all_recordings(engine, family):
    """The same through CollectAllLossy(loss=0) and CollectAllChurn (k_light, k_heavy): when a
    K-column case above fails, this tells the rule from the column kernels."""
    d = vd_cases.ca(family)
    with _open(engine, "ca", d.values) as eng:
        for q, stop in enumerate(d.stops):
            eng.run(stop - eng.rounds_done)
            assert_same_bits(eng.estimates(), d.last_avg[q], (engine, family, stop, "estimates"))
            assert_same_bits(eng.flows(), d.flows[q], (engine, family, stop, "flows"))
            if engine == "lossy":
                assert eng.stats == (d.E * (stop - 1), 0), stop
            else:
                assert (eng.slot_state() == UP).all() and eng.stats == (d.n, d.E), stop


# ------------------------------------------------------------------------------------
# 2. the recorded loss and the recorded topologies
# ------------------------------------------------------------------------------------
def _lossy_handle(V):
    g = graph("lossy")
    eng = fu.CollectAllLossyBatch(rowptr=g.rowptr, col=g.col, rev=g.rev, values=V, loss=g.loss, seed=g.seed)
    eng.set_link_mask(g.down)
    return eng


@pytest.mark.parametrize("name", sorted(RULE_LAYOUTS))
def test_lossy_columns_equal_the_recordings_under_recorded_loss(name):
    """subn and special beside filler columns at the recorded (p, seed) and `down` mask: a lost
    slot fires on the pair its row stored (kOwn), in both heavy rows, where that flow is -0.0, an
    infinity or NaN. The fillers follow lossy_python on the recorded masks at every stop."""
    V, fams = vd_columns("lossy", *RULE_LAYOUTS[name])
    g = graph("lossy")
    with _lossy_handle(V) as eng:
        for q, stop in enumerate(g.stops):
            eng.run(stop - eng.rounds_done)
            _check_columns(eng, "lossy", "lossy", fams, q, (name, stop))
            assert eng.stats == (g.E * (stop - 1), lost_before(g, stop)), stop


def _churn_through_the_recording(eng, after_stop, err_every=0):
    """The recorded events and stops on a churn handle: slot_state() after every event and every
    stop; after_stop(q, stop). Returns the error traces of the runs, stacked."""
    g = graph("churn")
    after_event = churn_states_after_events(g)
    traces = []
    assert np.array_equal(eng.slot_state(), after_event[0])
    for q, stop in enumerate(g.stops):
        if q:
            eng.set_topology(g.alive[q], g.link_up[q])
            assert g.event_rounds[q] == eng.rounds_done
            assert np.array_equal(eng.slot_state(), after_event[q]), ("after the event before round", eng.rounds_done)
        traces.append(eng.run(stop - eng.rounds_done, err_every=err_every))
        assert np.array_equal(eng.slot_state(), np.where(g.live[q], UP, DOWN)), stop
        after_stop(q, stop)
    return np.concatenate(traces) if err_every else None


@pytest.mark.parametrize("name", sorted(RULE_LAYOUTS))
def test_churn_columns_equal_the_recordings_through_recorded_topologies(name):
    """subn and special beside filler columns through the recorded set_topology events: FRESH
    slots (kZero) next to estimates of -0.0, DOWN slots (kSkip) in front of inf and NaN, dead
    rows that keep all K estimates. The fillers follow churn_python on the same script."""
    V, fams = vd_columns("churn", *RULE_LAYOUTS[name])
    with _open("churn", "churn", V) as eng:
        _churn_through_the_recording(eng, lambda q, stop: _check_columns(eng, "churn", "churn", fams, q, (name, stop)))


@pytest.mark.parametrize("engine", ENGINES)
def test_error_trace_on_the_value_domain(engine):
    """k_max_err_cols at (special, filler, subn), err_every = 1, targets = the reference's last
    estimates (rev_columns_vd_cases.error_case): the subn and filler traces are numpy's
    max |a - target| over the Python rule's estimates of every round, subnormal differences
    included, under churn over the alive nodes; the special column's entry is NaN from the round
    the rule first holds a NaN, in no earlier round, and raises no other column."""
    V, target, want, _ = error_case(engine)
    fams = layout(engine, ("special", None, "subn"))[1]
    if engine == "lossy":
        with _lossy_handle(V) as eng:
            eng.set_targets(target)
            trace = eng.run(len(want), err_every=1)
            _check_columns(eng, engine, engine, fams, len(stops(engine)) - 1, ("err", engine))
            last = eng.max_err()
    else:
        with _open("churn", "churn", V) as eng:
            eng.set_targets(target)
            trace = _churn_through_the_recording(
                eng, lambda q, stop: _check_columns(eng, engine, engine, fams, q, ("err", engine, stop)), err_every=1)
            last = eng.max_err()
    assert trace.shape == want.shape
    for c in range(3):
        assert_same_bits(np.ascontiguousarray(trace[:, c]), np.ascontiguousarray(want[:, c]), (engine, "trace", c))
    assert np.array_equal(np.isnan(trace[:, 0]), np.isnan(want[:, 0])) and np.isfinite(trace[:, 1:]).all()
    assert_same_bits(last, want[-1], (engine, "max_err"))


# ------------------------------------------------------------------------------------
# 3. special values at the chunk edges of each K
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HEAVY_LAYOUTS))
def test_churn_special_values_at_the_chunk_edges(name):
    """subn, huge and the planted column (+inf and -0.0 on the two sides of the first chunk edge,
    NaN on the last slot of every row of more than one chunk) through heavy_boundary_script(K),
    which takes exactly those slots DOWN and brings half of them back FRESH; every column against
    churn_python. The filler columns also equal a handle that holds them alone."""
    g, V, spec = heavy_columns(name)
    script = heavy_boundary_script(len(spec))[0]
    steps = heavy_churn_steps(name)
    fill = fillers(spec)
    seen = []
    with fu.CollectAllChurnBatch(g, V) as eng:
        drive_churn(eng, script, steps, (name,), after=lambda q: seen.append((eng.estimates()[:, fill], eng.flows()[:, fill])))
    if fill:
        def same(q):
            assert_same_bits(alone.estimates(), seen[q][0], (name, "fillers alone, estimates", q))
            assert_same_bits(alone.flows(), seen[q][1], (name, "fillers alone, flows", q))

        with fu.CollectAllChurnBatch(g, np.ascontiguousarray(V[:, fill])) as alone:
            drive_churn(alone, script, [s._replace(a=s.a[:, fill], f=s.f[:, fill]) for s in steps], (name, "alone"), after=same)


@pytest.mark.parametrize("name", sorted(HEAVY_LAYOUTS))
def test_lossy_special_values_at_the_chunk_edges(name):
    """The same columns at p = 0.5 after 1, 2, 5 and 10 rounds against lossy_python: half of the
    slots of every chunk are kOwn, the planted ones in some rounds."""
    g, V, spec = heavy_columns(name)
    want = heavy_lossy_stops(name)
    fill = fillers(spec)
    lost = 0
    alone = fu.CollectAllLossyBatch(g, np.ascontiguousarray(V[:, fill]), loss=HEAVY_LOSS, seed=LOSS_SEED) if fill else None
    try:
        with fu.CollectAllLossyBatch(g, V, loss=HEAVY_LOSS, seed=LOSS_SEED) as eng:
            done = 0
            for stop in HEAVY_STOPS:
                eng.run(stop - done)
                lost += sum(int((~hashed(HEAVY_LOSS, LOSS_SEED, g.E)(r)).sum()) for r in range(max(done, 1), stop))
                done = stop
                a, f = eng.estimates(), eng.flows()
                assert_same_bits(a, want[stop][0], (name, "estimates", stop))
                assert_same_bits(f, want[stop][1], (name, "flows", stop))
                assert eng.stats == (g.E * (stop - 1), lost)
                if alone is not None:
                    alone.run(stop - alone.rounds_done)
                    assert_same_bits(alone.estimates(), a[:, fill], (name, "fillers alone, estimates", stop))
                    assert_same_bits(alone.flows(), f[:, fill], (name, "fillers alone, flows", stop))
                    assert alone.stats == eng.stats
    finally:
        if alone is not None:
            alone.close()
