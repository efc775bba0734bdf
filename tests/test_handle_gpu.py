"""The handle scaffold the batched, lossy, pairwise and churn engines share, on the GPU: the run
loop with its error-trace slots, the timed loop, reset, the state errors of a live handle and the
teardown, each engine against its own restatement (coracle.ca_sync / ca_rounds per column,
lossy_cases.oracle_lossy, pair_cases.oracle_pair, churn_cases.churn_python), by bit pattern.

Two golden graphs: ca_sync_er300_m450 (light rows only) and ca_sync_star_257, whose hub is above
every engine's heavy threshold (64, 128, 64 and 128 slots), so both launch classes of every
engine run. The batch has K = 3 columns: an error width that is neither 1 nor a divisor of 256.
The churn handle runs under a fixed topology with a fifth of the nodes dead and a tenth of the
links down (star_257's hub alive), applied when it is made; its error trace is the maximum over
the alive nodes."""
import functools
import math

import numpy as np
import pytest

import coracle
import fu
from churn_cases import churn_python, random_masks
from conftest import ca_sync_fixtures, load_npz
from fu import _lib as L
from lossy_cases import hashed, oracle_lossy
from pair_cases import oracle_pair
from parity_util import FAMILIES, assert_same_bits

pytestmark = pytest.mark.gpu

ENGINES = ("batch", "lossy", "pair", "churn")
GRAPHS = ("er300_m450", "star_257")
SEED, LOSS, K = 11, 0.25, 3
R_FIT, R_GROW, R_TIMED = 4, 12, 3  # run(4, err_every=4); run(12, err_every=1); run_timed(3)
R = R_FIT + R_GROW + R_TIMED
ARG, STATE = -1, -4


@functools.lru_cache(maxsize=None)
def _graph(name):
    d = load_npz(dict(ca_sync_fixtures())[name]["file"])
    g = fu.Graph.from_csr(d["rowptr"], d["col"])
    return g, np.ascontiguousarray(d["values"], dtype=np.float64)


def _values(eng, name):
    g, v = _graph(name)
    if eng != "batch":
        return v
    return np.stack([v, FAMILIES["sym"](g.n, seed=3), FAMILIES["wide"](g.n, seed=3)], axis=1)


def _targets(eng, name):
    """Nothing special about them: the trace is max |a_r - t| whatever t is."""
    g, _ = _graph(name)
    t = np.stack([FAMILIES["sym"](g.n, seed=20 + c) for c in range(K)], axis=1)
    return t if eng == "batch" else np.ascontiguousarray(t[:, 0])


@functools.lru_cache(maxsize=None)
def _topology(name):
    """The churn handle's (alive, link_up): the hub of the star stays alive."""
    g, _ = _graph(name)
    return random_masks(g, 0.2, 0.1, SEED, keep=(int(np.argmax(g.degrees)),) if name == "star_257" else ())


@functools.lru_cache(maxsize=None)
def _ref(eng, name):
    """(a_rounds, state): the estimates after each of rounds 0 .. R-1, and what the handle holds
    after R rounds, from the oracle alone."""
    g, _ = _graph(name)
    v = _values(eng, name)
    if eng == "batch":
        cols, flows = [], []
        for c in range(K):
            vc = np.ascontiguousarray(v[:, c])
            a, f = coracle.ca_sync(*g.arrays(), vc, 1)
            per = [a.copy()]
            for _ in range(R - 1):
                coracle.ca_rounds(*g.arrays(), vc, 1, a, f)
                per.append(a.copy())
            cols.append(np.stack(per))
            flows.append(f.copy())
        a_rounds = np.stack(cols, axis=2)
        return a_rounds, {"estimates": a_rounds[-1], "flows": np.stack(flows, axis=1)}
    if eng == "lossy":
        a, f, sn = oracle_lossy(*g.arrays(), v, R, hashed(LOSS, SEED, g.E), snaps=tuple(range(R)))
        return np.stack([sn[r] for r in range(R)]), {"estimates": a, "flows": f}
    if eng == "churn":
        ref = churn_python(*g.arrays(), v, [("topology",) + _topology(name)] + [("run", 1)] * R)
        return np.stack(ref.a_rounds), {"estimates": ref.a, "flows": ref.f}
    last, f, c, sn = oracle_pair(*g.arrays(), v, R, SEED, snaps=tuple(range(R)))
    return np.stack([sn[r] for r in range(R)]), {"estimates": last, "flows": f, "cache": c}


def _make(eng, name):
    g, _ = _graph(name)
    v = _values(eng, name)
    if eng == "batch":
        return fu.CollectAllBatch(g, v)
    if eng == "lossy":
        return fu.CollectAllLossy(g, v, loss=LOSS, seed=SEED)
    if eng == "churn":
        h = fu.CollectAllChurn(g, v)
        h.set_topology(*_topology(name))
        return h
    return fu.PairwiseSync(g, v, seed=SEED)


def _state(eng, h):
    s = {"estimates": h.estimates(), "flows": h.flows()}
    if eng == "pair":
        s["cache"] = h.cache()
    return s


def _want_trace(eng, name, rounds):
    a_rounds, t = _ref(eng, name)[0], _targets(eng, name)
    on = _topology(name)[0] != 0 if eng == "churn" else slice(None)  # a dead node's frozen estimate does not count
    return np.stack([np.max(np.abs(a_rounds[r - 1] - t)[on], axis=0) for r in rounds])


def _same_state(got, want, what):
    assert got.keys() == want.keys()
    for key in want:
        assert_same_bits(got[key], want[key], what + (key,))


@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("eng", ENGINES)
def test_shared_run_loop(eng, name):
    what = (eng, name)
    h = _make(eng, name)
    h.set_targets(_targets(eng, name))
    tr = h.run(R_FIT, err_every=R_FIT)  # one check: fits the slots allocated at create
    assert_same_bits(tr, _want_trace(eng, name, [R_FIT]), what + ("first trace",))
    tr = h.run(R_GROW, err_every=1)  # the slots grow; the round counter goes on
    assert_same_bits(tr, _want_trace(eng, name, range(R_FIT + 1, R_FIT + R_GROW + 1)), what + ("second trace",))
    assert h.rounds_done == R_FIT + R_GROW
    ms = h.run_timed(R_TIMED)
    assert math.isfinite(ms) and ms >= 0.0, ms
    assert h.rounds_done == R
    _same_state(_state(eng, h), _ref(eng, name)[1], what + ("after run_timed",))
    assert_same_bits(np.atleast_1d(h.max_err()), _want_trace(eng, name, [R])[0].reshape(-1), what + ("max_err",))
    h.reset()
    assert h.rounds_done == 0
    h.run(R)
    fresh = _make(eng, name)
    fresh.run(R)
    _same_state(_state(eng, h), _state(eng, fresh), what + ("reset and rerun against a fresh handle",))
    _same_state(_state(eng, fresh), _ref(eng, name)[1], what + ("fresh handle",))
    fresh.close()
    h.close()


@pytest.mark.parametrize("eng", ENGINES)
def test_live_handle_state_errors(eng):
    name = "er300_m450"
    h = _make(eng, name)
    t = _targets(eng, name)
    out = np.full(K, -1.0)
    out_p = out.ctypes.data_as(L.P(L.f64))  # K doubles for the batch, one for the others

    def call(fn, *args):
        return getattr(L.lib, f"fu_{eng}_{fn}")(h._h, *args), L.last_error()

    assert call("run", 2, 1, None) == (STATE, f"fu_{eng}_run: err_every > 0 needs fu_{eng}_set_targets")
    assert call("max_err", out_p) == (STATE, f"fu_{eng}_max_err: call fu_{eng}_set_targets first")
    h.set_targets(t)
    if eng == "pair":  # allowed before any round: every last average is still 0.0
        assert call("max_err", out_p)[0] == 0
        assert_same_bits(out[:1], np.array([np.max(np.abs(0.0 - t))]), "pair max_err at round 0")
    else:
        assert call("max_err", out_p) == (STATE, f"fu_{eng}_max_err: no round has run")
    assert call("run", -1, 0, None) == (ARG, f"fu_{eng}_run: bad arguments")
    assert call("run_timed", 1, None) == (ARG, f"fu_{eng}_run_timed: bad arguments")
    assert h.rounds_done == 0  # none of them ran a round
    tr = h.run(2, err_every=2)
    assert_same_bits(tr, _want_trace(eng, name, [2]), (eng, "the handle still runs"))
    h.close()


@pytest.mark.parametrize("first,second,third", [("batch", "lossy", "pair"), ("lossy", "pair", "batch"),
                                                ("pair", "batch", "lossy"), ("churn", "pair", "lossy"),
                                                ("lossy", "churn", "batch"), ("batch", "pair", "churn")])
def test_handles_close_in_the_opposite_order_of_creation(first, second, third):
    """Two engines on one graph, each closed after a run, the later one first; the earlier one
    is unharmed by it, and a handle of the third engine made afterwards matches the oracle."""
    name = "star_257"
    a = _make(first, name)
    b = _make(second, name)
    a.run(R)
    b.run(R)
    _same_state(_state(second, b), _ref(second, name)[1], (second, "second handle"))
    b.close()
    _same_state(_state(first, a), _ref(first, name)[1], (first, "first handle, the second closed"))
    a.close()
    a.close()  # closing twice is nothing
    with _make(third, name) as c:
        c.run(R)
        _same_state(_state(third, c), _ref(third, name)[1], (third, "third handle"))
