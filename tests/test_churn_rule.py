"""The restatement of the churn rule (churn_cases.churn_python) against the pinned C oracle,
without the engine: no topology call is coracle.ca_sync; a topology set before round 0 is
coracle.ca_sync on the live subgraph; a pure removal continues as coracle.ca_rounds on the live
subgraph; and after a kill and after a revival with new inputs the alive nodes converge to
fu.churn_targets, which is what the lossy engine's link mask cannot give."""
import numpy as np
import pytest

import coracle
import fu
import oracle
from churn_cases import (DOWN, FRESH, UP, check_static, churn_python, compact, cut, hub60, live_np, random_masks, row_slots,
                         tile_limit_graph)
from conftest import ca_sync_fixtures, load_npz
from parity_util import assert_same_bits


@pytest.mark.parametrize("name,meta", ca_sync_fixtures())
def test_no_topology_call_is_ca_sync(name, meta):
    """Rounds 0-19, estimates and flows, and the recorded snapshots up to round 19."""
    d = load_npz(meta["file"])
    rp, col, v = d["rowptr"], d["col"], d["values"]
    rev = oracle.build_rev(rp, col)
    got = churn_python(rp, col, rev, v, [("run", 20)])
    assert (got.state == UP).all() and got.steps[0].alive_nodes == len(v) and got.steps[0].live_slots == len(col)
    a = f = None
    for r in range(20):
        if a is None:
            a, f = coracle.ca_sync(rp, col, rev, v, 1)
        else:
            coracle.ca_rounds(rp, col, rev, v, 1, a, f)
        assert_same_bits(got.a_rounds[r], a, (name, "estimates", r))
        assert_same_bits(got.f_rounds[r], f, (name, "flows", r))
    for k, r in enumerate(int(r) for r in d["rounds"]):
        if r < 20:
            assert_same_bits(got.a_rounds[r], np.ascontiguousarray(d["last_avg"][k], dtype=np.float64), (name, "fixture", r))
            assert_same_bits(got.f_rounds[r], np.ascontiguousarray(d["flows"][k], dtype=np.float64), (name, "fixture", r))


def _static_masks(gname, case):
    g = {"hub60": hub60, "tile_limit": tile_limit_graph}[gname]()
    hub = int(np.argmax(g.degrees))
    if case == "random":  # 20 % of the nodes dead, 10 % of the links down
        alive, up = random_masks(g, 0.2, 0.1, 3, keep=(hub,))
        assert 0.1 < 1 - alive.mean() < 0.3 and 0.05 < 1 - up.mean() < 0.15
    else:
        alive, up = random_masks(g, 0.2, 0.1, 4)
        alive[hub] = 0
    return g, alive, up


@pytest.mark.parametrize("case", ["random", "hub_dead"])
@pytest.mark.parametrize("gname", ["hub60", "tile_limit"])
def test_static_topology_is_ca_sync_on_the_live_subgraph(gname, case):
    g, alive, up = _static_masks(gname, case)
    v = fu.uniform_values(g.n, seed=5)
    rounds = 20 if gname == "hub60" else 6
    got = churn_python(*g.arrays(), v, [("topology", alive, up), ("run", rounds)])
    live = live_np(*g.arrays(), alive, up)
    assert got.steps[0].alive_nodes == int(alive.sum()) and got.steps[0].live_slots == int(live.sum())
    assert np.array_equal(got.steps[0].state, np.where(live, FRESH, DOWN))
    check_static(g, alive, up, v, got.a, got.f, got.state, rounds, (gname, case))


def test_pure_removal_continues_as_ca_rounds_on_the_live_subgraph():
    """A kill and a cut after round 6 and nothing revived: no FRESH slot, so rounds 7-19 are
    the steady-state rounds of the oracle on the live subgraph, continued from the restatement's
    own (a, f) gathered onto it."""
    g = hub60()
    v = fu.uniform_values(g.n, seed=5)
    alive, up = random_masks(g, 0.2, 0.1, 3)
    up = cut(g, up, row_slots(g, 0)[[0, 20, 48]])
    live = live_np(*g.arrays(), alive, up)
    rp, col, rev, kmap = compact(*g.arrays(), live)
    got = churn_python(*g.arrays(), v, [("run", 7), ("topology", alive, up), ("run", 13)])
    assert not (got.steps[1].state == FRESH).any() and (got.steps[1].state == DOWN).sum() == (~live).sum()
    assert_same_bits(got.steps[1].f[~live], np.zeros(int((~live).sum())), "dropped flows")
    on = alive != 0
    a, f = got.steps[0].a.copy(), np.ascontiguousarray(got.steps[0].f[kmap])
    frozen = a[~on].copy()
    for r in range(7, 20):
        coracle.ca_rounds(rp, col, rev, v, 1, a, f)
        assert_same_bits(got.a_rounds[r][on], a[on], ("estimates", r))
        assert_same_bits(got.f_rounds[r][kmap], f, ("flows", r))
        assert_same_bits(got.a_rounds[r][~on], frozen, ("dead nodes keep their estimate", r))
        assert_same_bits(got.f_rounds[r][~live], np.zeros(int((~live).sum())), ("down flows", r))


CONVERGENCE_ROUNDS = 400


def test_alive_nodes_converge_to_the_means_of_the_alive_inputs():
    """hub60: a kill (10 nodes, the hub among them, and 9 links), then everything revived with new
    inputs, R rounds after each. R = 400 is the first multiple of 50 at which the restatement is
    within 1e-9 of fu.churn_targets on every alive node after both events: observed 1.03e-10
    after the kill and 2.8e-14 after the revival at R = 400; 2.5e-9 after the kill at R = 350
    (without the hub the live graph is sparse and mixes slowly)."""
    g = hub60()
    v1, v2 = fu.uniform_values(g.n, seed=5), fu.uniform_values(g.n, seed=6)
    alive, up = random_masks(g, 0.2, 0.1, 3)
    alive[0] = 0
    R = CONVERGENCE_ROUNDS
    got = churn_python(*g.arrays(), v1, [("run", 30), ("topology", alive, up), ("run", R), ("topology", None, None),
                                         ("values", v2), ("run", R)])
    on = alive != 0
    t1 = fu.churn_targets(g, v1, alive, up)
    err1 = float(np.max(np.abs(got.steps[2].a - t1)[on]))
    t2 = fu.churn_targets(g, v2)
    err2 = float(np.max(np.abs(got.a - t2)))
    print(f"R = {R}: after the kill {err1:.3e}, after the revival {err2:.3e}")
    assert err1 < 1e-9 and err2 < 1e-9
    # the dead nodes' last estimates, which a link mask would keep averaging in, are far off
    assert float(np.max(np.abs(got.steps[2].a - t1)[~on])) > 1.0
