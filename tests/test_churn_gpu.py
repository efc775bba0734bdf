"""fu.CollectAllChurn (csrc/fu_churn.hip) against restatements that do not run it: the recorded
fixtures and coracle.ca_sync with everything alive, coracle.ca_sync on the live subgraph under a
static topology, and the rule on Python floats (churn_cases.churn_python) wherever nodes and
links leave and join between rounds. Every comparison is by bit pattern, on estimates and flows,
and exact on the slot states and the counts.

The kernel's row classes change at degree 128 (light tiles of at most 256 rows and 2048 slots /
one block per row, staged in chunks of 2048 slots): lossy_cases.tile_limit_graph() closes its
tiles in every way and has one row of degree 129, star(2100)'s hub row spans two chunks, and
churn_cases.chunk_edge_graph() has six heavy rows of one slot under a chunk, a chunk, a chunk and
one slot, two chunks, two chunks and one slot, linked to each other, at the first, a middle and the
last ids. Sections 8-11 run on it, on a topology call before every round, on graphs of one node,
no link, one link and more nodes than slots, and on mask bytes other than 0 and 1; the conditions
on their inputs are tests/test_churn_case_inputs.py's, on any host."""
import functools

import numpy as np
import pytest

import coracle
import fu
from churn_cases import (DOWN, FRESH, HEAVY_CHUNK, TILE_ROWS, TILE_SLOTS, UP, byte_masks, check_static, chunk_edge_case,
                         chunk_edge_graph, chunk_edge_topology, churn_python, cut, flapping_case, heavy_rows, hub60, live_np,
                         random_masks, row_slots, scripted_run, star, tile_census, tile_limit_graph, tile_segment)
from conftest import ca_sync_fixtures, load_npz
from fu import _lib as L
from parity_util import FAMILIES, assert_same_bits, count_neg_zero

pytestmark = pytest.mark.gpu

GRAPHS = {"hub60": hub60, "tile_limit": tile_limit_graph}


def _check(eng, a_ref, f_ref, what):
    assert_same_bits(eng.estimates(), a_ref, what + ("estimates",))
    assert_same_bits(eng.flows(), f_ref, what + ("flows",))


def _apply(eng, step):
    if step[0] == "run":
        eng.run(step[1])
    elif step[0] == "topology":
        eng.set_topology(step[1], step[2])
    elif step[0] == "values":
        eng.set_values(step[1])
    else:
        eng.reset()


def _follow(eng, script, ref, what):
    """Every step of the script on the engine; after each, estimates, flows, slot states and
    the counts are the restatement's."""
    for q, (step, want) in enumerate(zip(script, ref.steps)):
        _apply(eng, step)
        _check(eng, want.a, want.f, what + (q, step[0]))
        assert np.array_equal(eng.slot_state(), want.state), what + (q, step[0], "slot states")
        assert eng.stats == (want.alive_nodes, want.live_slots), what + (q, step[0])


# ------------------------------------------------------------------------------------
# 1. everything alive, no topology call: the engine is CollectAll
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,meta", ca_sync_fixtures())
def test_all_alive_equals_the_recorded_fixtures(name, meta):
    """run(5); run(15) on one handle, against the recording of round 4 and coracle.ca_sync after
    5 and 20 rounds; a second handle stepped round by round through rounds 0-19."""
    d = load_npz(meta["file"])
    rp, col, v = d["rowptr"], d["col"], d["values"]
    rev = fu.Graph.from_csr(rp, col).rev
    k4 = [int(r) for r in d["rounds"]].index(4)
    with fu.CollectAllChurn(rowptr=rp, col=col, values=v) as eng, fu.CollectAllChurn(rowptr=rp, col=col, rev=rev, values=v) as one:
        assert eng.stats == (len(v), len(col)) and (eng.slot_state() == FRESH).all()
        _check(eng, np.zeros(len(v)), np.zeros(len(col)), (name, "before round 0"))
        eng.run(5)
        _check(eng, np.ascontiguousarray(d["last_avg"][k4], dtype=np.float64), np.ascontiguousarray(d["flows"][k4], dtype=np.float64),
               (name, "recorded round 4"))
        _check(eng, *coracle.ca_sync(rp, col, rev, v, 5), (name, 5))
        eng.run(15)
        assert eng.rounds_done == 20 and (eng.slot_state() == UP).all()
        _check(eng, *coracle.ca_sync(rp, col, rev, v, 20), (name, 20))
        a, f = coracle.ca_sync(rp, col, rev, v, 1)
        for r in range(20):
            one.run(1)
            _check(one, a, f, (name, "round", r))
            coracle.ca_rounds(rp, col, rev, v, 1, a, f)


def test_all_alive_equals_collectall_on_the_tile_limit_graph():
    g = tile_limit_graph()
    v = fu.uniform_values(g.n, seed=3)
    with fu.CollectAllChurn(g, v) as eng, fu.CollectAll(g, v) as ca:
        for r in (5, 15):
            eng.run(r)
            ca.run(r)
            _check(eng, ca.estimates(), ca.flows(), ("after", eng.rounds_done))
        _check(eng, *coracle.ca_sync(*g.arrays(), v, 20), ("oracle", 20))


# ------------------------------------------------------------------------------------
# 2. a topology set before round 0: CollectAll on the live subgraph
# ------------------------------------------------------------------------------------
def _tile_masks():
    """tile_limit_graph with a fifth of the nodes dead and a tenth of the links down, and on top:
    dead rows inside the 256-row tile without a slot, the 2048-slot tile with every slot DOWN, a
    tile with exactly one live slot, the heavy row with its first, an inner and its last slot
    DOWN. Each is asserted here, on the inputs."""
    g = tile_limit_graph()
    rp, col, rev = g.arrays()
    tiles = tile_census(rp)
    h = tile_segment("heavy")[0]
    alive, up = random_masks(g, 0.2, 0.1, 21, keep=(h,))
    iso0 = tile_segment("isolated")[0]
    alive[iso0:iso0 + TILE_ROWS] = 1
    alive[[iso0 + 3, iso0 + 100, iso0 + TILE_ROWS - 1]] = 0
    r8 = tile_segment("rr8")[0]
    up = cut(g, up, np.arange(rp[r8], rp[r8 + TILE_ROWS]))
    r3 = tile_segment("rr3")[0]
    s0, s1 = int(rp[r3]), int(rp[r3 + TILE_ROWS])
    k1 = next(k for k in range(s0, s1) if not r3 <= col[k] < r3 + TILE_ROWS)  # its reverse lies in another tile
    up = cut(g, up, [k for k in range(s0, s1) if k != k1])
    src = np.repeat(np.arange(g.n), np.diff(rp))
    alive[[src[k1], col[k1]]] = 1
    up[[k1, rev[k1]]] = 1
    hs = row_slots(g, h)
    up = cut(g, up, hs[[0, 64, 128]])
    live = live_np(rp, col, rev, alive, up)
    assert (iso0, iso0 + TILE_ROWS, 0, "rows") in tiles and not alive[iso0 + 3] and alive[iso0 + 4]
    assert (r8, r8 + TILE_ROWS, TILE_SLOTS, "rows") in tiles and not live[rp[r8]:rp[r8 + TILE_ROWS]].any()
    assert alive[r8:r8 + TILE_ROWS].any()  # rows that fire on a = v with the divisor 1
    assert (r3, r3 + TILE_ROWS, s1 - s0, "rows") in tiles and int(live[s0:s1].sum()) == 1 and live[k1]
    assert len(hs) == 129 and alive[h] and not live[hs[[0, 64, 128]]].any() and 64 < int(live[hs].sum()) < 126
    return g, alive, up


def _heavy_dead_masks():
    """The heavy row dead while all of its neighbours live."""
    g = tile_limit_graph()
    h = tile_segment("heavy")[0]
    alive, up = random_masks(g, 0.2, 0.1, 22)
    hs = row_slots(g, h)
    alive[g.col[hs]] = 1
    alive[h] = 0
    assert alive[g.col[hs]].all() and not live_np(*g.arrays(), alive, up)[hs].any()
    assert all(live_np(*g.arrays(), alive, up)[row_slots(g, int(j))].any() for j in g.col[hs][:8])
    return g, alive, up


@pytest.mark.parametrize("masks", [_tile_masks, _heavy_dead_masks], ids=["tiles", "heavy_dead"])
def test_static_topology_equals_ca_sync_on_the_live_subgraph(masks):
    g, alive, up = masks()
    v = fu.uniform_values(g.n, seed=5)
    live = live_np(*g.arrays(), alive, up)
    with fu.CollectAllChurn(g, v) as eng:
        eng.set_topology(alive, up)
        assert eng.stats == (int(alive.sum()), int(live.sum()))
        assert np.array_equal(eng.slot_state(), np.where(live, FRESH, DOWN))
        done = 0
        for r in (1, 2, 7, 20):
            eng.run(r - done)
            done = r
            check_static(g, alive, up, v, eng.estimates(), eng.flows(), eng.slot_state(), r, (masks.__name__, r))


# ------------------------------------------------------------------------------------
# 3. nodes and links leave and join between rounds
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scripted(gname, family):
    g = GRAPHS[gname]()
    if family == "uniform":
        v1, v2 = fu.uniform_values(g.n, seed=3), fu.uniform_values(g.n, seed=4)
    elif family == "special":
        v1, v2 = fu.uniform_values(g.n, seed=3), fu.uniform_values(g.n, seed=4)
        v1[[7, 19, 33]] = [-0.0, np.inf, -np.inf]
        v2[[5, 41]] = [-0.0, np.nan]
    else:
        v1, v2 = FAMILIES[family](g.n, 4), FAMILIES[family](g.n, 5)
    script = scripted_run(g, 7, v2)
    return g, v1, script, churn_python(*g.arrays(), v1, script)


@pytest.mark.parametrize("gname", ["hub60", "tile_limit"])
def test_scripted_inputs_mix_the_three_states(gname):
    """Conditions on the scripted case, from the restatement alone: before the round that follows
    the revival, a light tile (and the heavy row, where the graph has one) holds UP, DOWN and
    FRESH slots at once; the double topology call leaves slots FRESH whose flow, non-zero
    before, is dropped."""
    g, _, script, ref = _scripted(gname, "uniform")
    assert [s[0] for s in script] == ["run", "topology", "run", "topology", "run", "values", "run", "topology", "topology", "run",
                                      "reset", "run"]
    st = ref.steps[3].state
    mixed = [t for t in tile_census(g.rowptr) if set(st[g.rowptr[t[0]]:g.rowptr[t[1]]].tolist()) == {UP, DOWN, FRESH}]
    assert mixed
    assert (heavy_rows(g) != []) == (gname == "tile_limit")
    for h in heavy_rows(g):
        assert set(st[row_slots(g, h)].tolist()) == {UP, DOWN, FRESH}
    hub = int(np.argmax(g.degrees))
    assert set(st[row_slots(g, hub)].tolist()) == {UP, DOWN, FRESH}
    before, between, after = ref.steps[6], ref.steps[7], ref.steps[8]
    flipped = (before.state == UP) & (between.state == DOWN) & (after.state == FRESH)
    assert flipped.any() and (before.f[flipped] != 0.0).any()
    assert_same_bits(after.f[flipped], np.zeros(int(flipped.sum())), "dropped flows")
    assert (ref.steps[10].state != UP).all() and not ref.steps[10].a.any()  # the reset


@pytest.mark.parametrize("gname", ["hub60", "tile_limit"])
def test_scripted_run_equals_the_python_restatement(gname):
    g, v1, script, ref = _scripted(gname, "uniform")
    with fu.CollectAllChurn(g, v1) as eng:
        _follow(eng, script, ref, (gname,))
        assert eng.rounds_done == 3


def test_a_run_is_splittable_under_churn():
    """run(17) equals run(5); run(12), also with FRESH and DOWN slots at the start."""
    g, v1, script, ref = _scripted("tile_limit", "uniform")
    with fu.CollectAllChurn(g, v1) as one, fu.CollectAllChurn(g, v1) as two:
        for eng in (one, two):
            for step in script[:4]:
                _apply(eng, step)
        one.run(17)
        two.run(5)
        two.run(12)
        _check(two, one.estimates(), one.flows(), ("split",))
        assert np.array_equal(one.slot_state(), two.slot_state())


# ------------------------------------------------------------------------------------
# 4. a heavy row of two chunks
# ------------------------------------------------------------------------------------
def test_deaths_across_the_chunk_boundary_of_a_heavy_row():
    """star(2100): the leaves on slots chunk-2 .. chunk+1 of the hub's row die with 300 random
    leaves, later all revive; 6 rounds around each event. The S and T carried from chunk to
    chunk, the live count summed over both chunks and the divisor all show here."""
    g = star(2100)
    hs = row_slots(g, 0)
    assert len(hs) == 2100 > HEAVY_CHUNK
    rng = np.random.default_rng(8)
    dead = np.concatenate([g.col[hs[HEAVY_CHUNK - 2:HEAVY_CHUNK + 2]], 1 + rng.choice(2100, size=300, replace=False)])
    alive = np.ones(g.n, dtype=np.uint8)
    alive[dead] = 0
    live = live_np(*g.arrays(), alive, None)
    assert alive[0] and not live[hs[HEAVY_CHUNK - 2:HEAVY_CHUNK + 2]].any()
    assert live[hs[:HEAVY_CHUNK]].any() and live[hs[HEAVY_CHUNK:]].any() and 296 <= int((~live[hs]).sum()) <= 304
    v = fu.uniform_values(g.n, seed=3)
    script = [("run", 6), ("topology", alive, None), ("run", 1), ("run", 5), ("topology", None, None), ("run", 1), ("run", 5)]
    ref = churn_python(*g.arrays(), v, script)
    with fu.CollectAllChurn(g, v) as eng:
        _follow(eng, script, ref, ("star",))


# ------------------------------------------------------------------------------------
# 5. the value domain
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["subn", "wide", "huge", "special"])
def test_value_domain_under_the_script(family):
    """Subnormals around zero (the -0.0 flows that a skipped slot's +0.0 must not disturb), 36
    decades, overflowing chains, and a column with -0.0, +-inf and a NaN."""
    g, v1, script, ref = _scripted("hub60", family)
    flows = np.concatenate(ref.f_rounds)  # of every round run
    if family == "subn":
        assert count_neg_zero(flows) > 0 and count_neg_zero(np.concatenate([s.f for s in ref.steps])) > 0
        assert count_neg_zero(np.concatenate(ref.a_rounds)) > 0
    if family == "huge":
        assert np.isnan(flows).any() and np.isinf(flows).any()
    if family == "special":
        assert np.isnan(flows).any() and np.isfinite(flows).any()
    with fu.CollectAllChurn(g, v1) as eng:
        _follow(eng, script, ref, (family,))


# ------------------------------------------------------------------------------------
# 6. the error reduction over the alive nodes
# ------------------------------------------------------------------------------------
def test_error_trace_is_the_maximum_over_the_alive_nodes():
    g = hub60()
    v = fu.uniform_values(g.n, seed=3)
    alive, up = random_masks(g, 0.2, 0.1, 3, keep=(0,))
    R = 8
    script = [("run", 6), ("topology", alive, up), ("run", R)]
    ref = churn_python(*g.arrays(), v, script)
    on = alive != 0
    p = int(np.flatnonzero(~on)[0])
    t = fu.churn_targets(g, v, alive, up)
    t[p] = ref.steps[0].a[p] + 2.0 ** 20  # the dead node's frozen estimate, 2^20 off its target
    want = np.array([np.max(np.abs(ref.a_rounds[6 + r] - t)[on]) for r in range(R)])
    assert float(np.max(want)) < 2.0 ** 10 and abs(ref.a[p] - t[p]) > 2.0 ** 19
    with fu.CollectAllChurn(g, v) as eng:
        eng.set_targets(t)
        with pytest.raises(fu.FuError) as ei:  # no round has run
            eng.max_err()
        assert ei.value.code == -4
        eng.run(6)
        eng.set_topology(alive, up)
        trace = eng.run(R, err_every=1)
        assert_same_bits(trace, want, "every round")
        assert_same_bits(np.array([eng.max_err()]), want[-1:], "max_err")
        _check(eng, ref.a, ref.f, ("after the trace",))
        eng.set_topology(np.zeros(g.n, dtype=np.uint8), None)
        assert eng.stats == (0, 0)
        assert_same_bits(eng.run(2, err_every=1), np.zeros(2), "every node dead")
        assert_same_bits(np.array([eng.max_err()]), np.zeros(1), "every node dead, max_err")
        assert_same_bits(eng.estimates(), ref.a, "dead nodes keep their estimates")


# ------------------------------------------------------------------------------------
# 7. the timed entry point, interleaved handles, the command line
# ------------------------------------------------------------------------------------
def test_run_timed_and_interleaved_handles():
    g = tile_limit_graph()
    v1, v2 = fu.uniform_values(g.n, seed=3), fu.uniform_values(g.n, seed=4)
    alive, up = random_masks(g, 0.2, 0.1, 21)
    ref = churn_python(*g.arrays(), v1, [("run", 3), ("topology", alive, up), ("run", 10)])
    a2, f2 = coracle.ca_sync(*g.arrays(), v2, 10)
    with fu.CollectAllChurn(g, v1) as c1, fu.CollectAllChurn(g, v2) as c2, fu.CollectAll(g, v2) as ca:
        c1.run(3)
        assert c2.run_timed(4) > 0.0
        ca.run(5)
        c1.set_topology(alive, up)
        assert c1.run_timed(10) > 0.0
        c2.run(6)
        ca.run(5)
        assert c1.rounds_done == 13 and c2.rounds_done == 10
        _check(c1, ref.a, ref.f, ("timed, under churn",))
        assert np.array_equal(c1.slot_state(), ref.state)
        _check(c2, a2, f2, ("second churn handle",))
        _check(ca, a2, f2, ("CollectAll",))


def test_cli_bench_graph_with_churn(capsys):
    """`python -m fu bench-graph SPEC --churn F --churn-seed S` (in process): the usual line plus
    alive=<count>, node i dead iff U_i < F on the fu_values_uniform stream at S."""
    from fu.__main__ import main

    assert main(["bench-graph", "er:n=2000,m=8000", "--rounds", "7", "--churn", "0.1", "--churn-seed", "4"]) == 0
    line = capsys.readouterr().out.strip()
    g = fu.Graph.from_spec("er:n=2000,m=8000", seed=1)
    alive = int((fu.uniform_values(g.n, seed=4, lo=0.0, hi=1.0) >= 0.1).sum())
    assert 1700 < alive < 1900
    assert line.startswith(f"graph n={g.n} E={g.E} ") and " rounds=7 " in line and line.endswith(f" alive={alive}")
    assert np.isfinite(float(line.split(" max_err=")[1].split()[0]))


# ------------------------------------------------------------------------------------
# 8. heavy rows at the chunk edges
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_chunk_edge_static_topology_equals_ca_sync_on_the_live_subgraph(which):
    """Rows of 2047, 2048, 2049, 4096 and 4097 slots under a topology set before round 0: "A" has
    slots 0, 2047, 2048 and d-1 of the long rows DOWN, the 2048 row alive without a live slot and
    the 2047 row dead; "B" one live slot in the 2049 row, the one of its second chunk, and the
    second chunk of the 4096 row DOWN; "C" that slot as the 2049 row's only DOWN one and the middle
    chunk of the 4097 row DOWN."""
    g = chunk_edge_graph()
    alive, up = chunk_edge_topology(which)
    v = fu.uniform_values(g.n, seed=5)
    live = live_np(*g.arrays(), alive, up)
    with fu.CollectAllChurn(g, v) as eng:
        eng.set_topology(alive, up)
        assert eng.stats == (int(alive.sum()), int(live.sum()))
        assert np.array_equal(eng.slot_state(), np.where(live, FRESH, DOWN))
        for r in (1, 2, 5):
            eng.run(r - eng.rounds_done)
            check_static(g, alive, up, v, eng.estimates(), eng.flows(), eng.slot_state(), r, ("chunk edges", which, r))
        assert eng.stats == (int(alive.sum()), int(live.sum()))


@pytest.mark.parametrize("family", ["uniform", "subn", "special"])
def test_chunk_edge_scripted_run_equals_the_python_restatement(family):
    """run(3); topology "A"; run(1); run(2); half of the dead and of the cut links back; run(1);
    run(2); reset; run(2), everything compared after every step: UP, DOWN and FRESH slots in one
    chunk of every long row, slots that turn FRESH on both sides of a chunk boundary and in the
    one-slot last chunks, heavy rows at both ends of a slot. "subn" brings -0.0 and "special" NaN
    into the long rows' flows (tests/test_churn_case_inputs.py)."""
    g, v, script, ref = chunk_edge_case(family)
    with fu.CollectAllChurn(g, v) as eng:
        _follow(eng, script, ref, ("chunk edges", family))
        assert eng.rounds_done == 2


# ------------------------------------------------------------------------------------
# 9. a topology call before every round
# ------------------------------------------------------------------------------------
def test_flapping_topology_every_round():
    """Ten times set_topology(fresh random masks); run(1) on tile_limit_graph(): slots that go
    UP -> DOWN -> FRESH -> UP -> DOWN, topology calls on both parities of the double buffer (the
    flow a call drops is the one the next round reads)."""
    g, v, script, ref = flapping_case()
    with fu.CollectAllChurn(g, v) as eng:
        _follow(eng, script, ref, ("flapping",))
        assert eng.rounds_done == len(script) // 2


# ------------------------------------------------------------------------------------
# 10. one node, no link, one link, more nodes than slots
# ------------------------------------------------------------------------------------
NO_I32 = np.zeros(0, dtype=np.int32)
NO_U8 = np.zeros(0, dtype=np.uint8)


def _u8(*x):
    return np.array(x, dtype=np.uint8)


def _follow_csr(rp, col, v, script, what):
    """_follow on a handle made from the raw CSR; returns the restatement's Result."""
    rev = fu.Graph.from_csr(rp, col).rev if len(col) else NO_I32
    ref = churn_python(rp, col, rev, v, script)
    with fu.CollectAllChurn(rowptr=rp, col=col, values=v) as eng:
        assert eng.stats == (len(v), len(col)) and eng.slot_state().shape == (len(col),) and eng.flows().shape == (len(col),)
        _follow(eng, script, ref, what)
    return ref


def test_one_node_without_a_link():
    """n = 1, E = 0: set_topology with and without an alive array and with an empty link_up, the
    node dead and alive again, reset, every readback."""
    script = [("run", 2), ("topology", _u8(0), None), ("values", np.array([7.0])), ("run", 1), ("topology", None, NO_U8),
              ("run", 1), ("topology", _u8(1), NO_U8), ("reset",), ("topology", None, None), ("run", 1), ("topology", _u8(0), NO_U8),
              ("reset",), ("run", 2)]
    ref = _follow_csr(np.zeros(2, dtype=np.int64), NO_I32, np.array([3.5]), script, ("n = 1",))
    assert [float(s.a[0]) for s in ref.steps] == [3.5, 3.5, 3.5, 3.5, 3.5, 7.0, 7.0, 0.0, 0.0, 7.0, 7.0, 0.0, 0.0]
    assert [s.alive_nodes for s in ref.steps][:5] == [1, 0, 0, 0, 1]


def test_five_isolated_nodes_two_of_them_dead():
    v = np.array([1.0, -2.5, -0.0, 1e300, 5e-324])
    rp = np.zeros(6, dtype=np.int64)
    alive = _u8(1, 0, 1, 0, 1)
    script = [("topology", alive, None), ("run", 2), ("topology", _u8(0, 0, 1, 0, 1), NO_U8), ("values", v + 1.0), ("run", 1),
              ("reset",), ("run", 1)]
    ref = _follow_csr(rp, NO_I32, v, script, ("isolated",))
    assert (ref.steps[0].alive_nodes, ref.steps[0].live_slots) == (3, 0)
    assert_same_bits(ref.steps[1].a, np.array([1.0, 0.0, 0.0, 0.0, 5e-324]), "the dead keep 0.0")  # (-0.0 - 0.0) + 0.0 = +0.0
    assert_same_bits(ref.steps[4].a, np.array([1.0, 0.0, 1.0, 0.0, 1.0]), "node 0 keeps its estimate")
    with fu.CollectAllChurn(rowptr=rp, col=NO_I32, values=v) as eng:
        eng.set_topology(alive)
        assert eng.stats == (3, 0)
        eng.run(3)
        assert_same_bits(eng.estimates(), ref.steps[1].a, "isolated, the first topology")


def test_two_nodes_and_one_link():
    """Kill one end: the survivor fires v / 1. Revive it: the slot is FRESH, then UP. Cut the link
    with both ends alive."""
    rp, col = np.array([0, 1, 2], dtype=np.int64), np.array([1, 0], dtype=np.int32)
    v = np.array([1.0, 4.0])
    script = [("run", 2), ("topology", _u8(1, 0), None), ("run", 1), ("topology", _u8(1, 1), _u8(1, 1)), ("run", 1), ("run", 1),
              ("topology", None, _u8(0, 0)), ("run", 2), ("topology", None, None), ("run", 1), ("reset",), ("run", 1)]
    ref = _follow_csr(rp, col, v, script, ("one link",))
    assert ref.steps[1].state.tolist() == [DOWN, DOWN] and ref.steps[2].a[0] == 1.0 and ref.steps[2].a[1] == ref.steps[0].a[1]
    assert ref.steps[3].state.tolist() == [FRESH, FRESH] and ref.steps[4].state.tolist() == [UP, UP]
    assert ref.steps[6].state.tolist() == [DOWN, DOWN] and ref.steps[6].alive_nodes == 2 and ref.steps[7].a.tolist() == [1.0, 4.0]
    assert ref.steps[8].state.tolist() == [FRESH, FRESH]


def test_more_nodes_than_slots():
    """n = 1000 with the single link 998 - 999: the topology pass is sized by n, and the alive
    nodes at ids >= E = 2 are counted by threads, and from 256 on by blocks, that hold no slot."""
    n = 1000
    g = fu.Graph.from_edges(n, np.array([998]), np.array([999]))
    assert g.E == 2 < n
    v = fu.uniform_values(n, seed=6)
    a1, _ = random_masks(g, 0.3, 0.0, 61)
    a2 = np.ones(n, dtype=np.uint8)
    a2[256:] = random_masks(g, 0.3, 0.0, 62)[0][256:]
    a3 = np.ones(n, dtype=np.uint8)
    a3[:2] = 0
    a4, _ = random_masks(g, 0.3, 0.0, 63, keep=(998, 999))
    assert 600 < a1.sum() < 800 and a2[:256].all() and 0 < (a2 == 0).sum() and a4[998:].all()
    script = [("topology", a1, None), ("run", 2), ("topology", a2, None), ("run", 1), ("topology", a3, _u8(1, 1)), ("run", 1),
              ("topology", a4, None), ("run", 2), ("reset",), ("run", 1), ("topology", a4, _u8(0, 0)), ("run", 1)]
    ref = churn_python(*g.arrays(), v, script)
    assert [ref.steps[q].alive_nodes for q in (0, 2, 4, 6)] == [int(a.sum()) for a in (a1, a2, a3, a4)]
    assert ref.steps[4].alive_nodes == n - 2 and ref.steps[6].live_slots == 2 and ref.steps[10].live_slots == 0
    with fu.CollectAllChurn(g, v) as eng:
        _follow(eng, script, ref, ("n > E",))


# ------------------------------------------------------------------------------------
# 11. mask bytes other than 0 and 1, through the C entry point
# ------------------------------------------------------------------------------------
def test_any_nonzero_mask_byte_is_on():
    """fu_churn_set_topology called directly with alive bytes from {0, 1, 2, 128, 255} and link_up
    bytes 7 on a slot and 255 on its reverse (fu.CollectAllChurn.set_topology would normalise
    them): the counts, the states and 5 rounds are the restatement's under the same masks as
    booleans."""
    g = hub60()
    v = fu.uniform_values(g.n, seed=3)
    alive, up = byte_masks(g, 71)
    script = [("run", 2), ("topology", alive != 0, up != 0), ("run", 5)]
    ref = churn_python(*g.arrays(), v, script)
    assert 0 < ref.steps[1].alive_nodes < g.n and 0 < ref.steps[1].live_slots < int((up != 0).sum())
    with fu.CollectAllChurn(g, v) as eng:
        eng.run(2)
        assert L.lib.fu_churn_set_topology(eng._h, L.ptr(alive), L.ptr(up)) == 0, L.last_error()
        assert eng.stats == (ref.steps[1].alive_nodes, ref.steps[1].live_slots)
        assert np.array_equal(eng.slot_state(), ref.steps[1].state)
        _check(eng, ref.steps[1].a, ref.steps[1].f, ("bytes", "after the call"))
        for r in range(5):
            eng.run(1)
            _check(eng, ref.a_rounds[2 + r], ref.f_rounds[2 + r], ("bytes", "round", r))
        assert np.array_equal(eng.slot_state(), ref.state)


# ------------------------------------------------------------------------------------
# 12. the rule itself: the reference's Peers through the recorded topologies (tests/golden/)
# ------------------------------------------------------------------------------------
def test_reference_peers_through_recorded_topologies():
    """hub_mix (rows of 2101 and 130 slots, light tiles, isolated rows): rounds 0-7 all alive,
    topologies before rounds 8, 16 and 24, run from stop to stop. Estimates and flows are what the
    reference's own on_receive / tick / avg_and_send left (make_golden.ca_churn_sync, neighbours
    kept in row order); the slot states are the entries that driver created and dropped.
    The values are in [0, 100), so no estimate is -0.0: a FRESH slot that gathered -f_old[rev k]
    (-0.0, the dropped flow) would leave every bit here as it is; the subnormal family of
    test_chunk_edge_scripted_run_equals_the_python_restatement is what sees that."""
    import rule_cases

    d = rule_cases.load("churn")
    after_event = rule_cases.churn_states_after_events(d)
    with fu.CollectAllChurn(rowptr=d.rowptr, col=d.col, rev=d.rev, values=d.values) as eng:
        assert np.array_equal(eng.slot_state(), after_event[0])
        for q, stop in enumerate(d.stops):
            if q:
                eng.set_topology(d.alive[q], d.link_up[q])
                assert d.event_rounds[q] == eng.rounds_done
                assert np.array_equal(eng.slot_state(), after_event[q]), ("after the event before round", eng.rounds_done)
            counts = (int((d.alive[q] != 0).sum()), int(d.live[q].sum()))
            assert eng.stats == counts, stop
            eng.run(stop - eng.rounds_done)
            _check(eng, d.last_avg[q], d.flows[q], ("reference peers", "after", stop))
            assert np.array_equal(eng.slot_state(), np.where(d.live[q], UP, DOWN)), stop
            assert eng.stats == counts, stop
