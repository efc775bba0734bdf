"""Conditions on the inputs of the churn engine's GPU cases (tests/test_churn_gpu.py), from host
code and the Python restatement (churn_cases.churn_python) alone: that a graph, a topology or a
script really holds the rows, chunks, slot states and values for which a case was built. No engine
runs here, so nothing needs a GPU."""
import numpy as np
import pytest

from churn_cases import (CHUNK_EDGE_CHAIN, CHUNK_EDGE_DEGREES, CHUNK_EDGE_REVIVAL, DOWN, FLAP_ROUNDS, FRESH, HEAVY_CHUNK,
                         TILE_HEAVY_DEG, UP, chunk_edge_case, chunk_edge_graph, chunk_edge_rows, chunk_edge_topology, flapping_case,
                         heavy_rows, live_np, row_slots, tile_census, tile_segment)
from parity_util import count_neg_zero

C = HEAVY_CHUNK


def _chunks(d):
    return [(c0, min(c0 + C, d)) for c0 in range(0, d, C)]


def _live(which):
    g = chunk_edge_graph()
    alive, up = chunk_edge_topology(which)
    return g, alive, live_np(*g.arrays(), alive, up)


# ------------------------------------------------------------------------------------
# the chunk-edge graph
# ------------------------------------------------------------------------------------
def test_chunk_edge_graph_rows_ids_and_tiles():
    g = chunk_edge_graph()
    row = chunk_edge_rows()
    assert list(CHUNK_EDGE_DEGREES) == [129, 2047, 2048, 2049, 4096, 4097] and C == 2048 and TILE_HEAVY_DEG == 128
    assert sorted(row) == list(CHUNK_EDGE_DEGREES)
    heavy = heavy_rows(g)
    assert heavy[:3] == [0, 1, 2] and heavy[4:] == [g.n - 2, g.n - 1] and 3000 < heavy[3] < g.n - 3000
    assert [len(_chunks(d)) for d in (2047, 2048, 2049, 4096, 4097)] == [1, 1, 2, 2, 3]
    assert _chunks(2049)[-1] == (2048, 2049) and _chunks(4097)[-1] == (4096, 4097)  # a last chunk of one slot
    assert _chunks(2048)[-1] == (0, C) and _chunks(4096)[-1] == (C, 2 * C)  # a last chunk that is full
    assert 14_000 < g.E // 2 < 19_000 and g.E <= 40_000
    # pairwise linked, the other slots are leaves of the row's own
    for h in heavy:
        nb = g.col[row_slots(g, h)]
        assert sorted(set(heavy) - {h}) == [int(j) for j in nb if g.degrees[j] > TILE_HEAVY_DEG]
        light = nb[g.degrees[nb] <= TILE_HEAVY_DEG]
        assert len(light) == g.degrees[h] - 5 and (g.degrees[light] <= 2).all()
    light = np.flatnonzero(g.degrees <= TILE_HEAVY_DEG)
    assert int((g.degrees[light] == 2).sum()) == 2 * len(range(0, len(light) - 1, CHUNK_EDGE_CHAIN))
    # the tile plan around the heavy rows: the first tile starts after three of them, one tile is
    # closed by the middle one, the last tile ends where the last two begin
    tiles = tile_census(g.rowptr)
    assert tiles[0][0] == 3 and tiles[-1][1] == g.n - 2 and tiles[-1][3] == "heavy"
    assert [t for t in tiles if t[1] == heavy[3]][0][3] == "heavy" and any(t[0] == heavy[3] + 1 for t in tiles)
    assert sum(j - i for i, j, _, _ in tiles) == g.n - 6
    src = np.repeat(np.arange(g.n), np.diff(g.rowptr))
    both_light = (g.degrees[src] <= 2) & (g.degrees[g.col] <= 2)
    assert all(both_light[g.rowptr[i]:g.rowptr[j]].any() for i, j, _, _ in tiles)


def test_chunk_edge_topology_a():
    """Topology "A". A chunk that holds nothing but slots cut by position (the one-slot last
    chunks of the 2049 and 4097 rows: slot d-1) is DOWN as a whole; every other chunk keeps a live
    slot. The 4096 row's all-DOWN chunk therefore sits in topology "B"."""
    g, alive, live = _live("A")
    row = chunk_edge_rows()
    leaves = np.flatnonzero(g.degrees <= 2)
    assert 0.07 < 1.0 - alive[leaves].mean() < 0.13
    for d in (2049, 4096, 4097):
        hs = row_slots(g, row[d])
        named = [0, C - 1, C, d - 1]
        assert alive[row[d]] and not live[hs[named]].any()
        for c0, c1 in _chunks(d):
            others = [q for q in range(c0, c1) if q not in named]
            assert (others == []) != bool(live[hs[others]].any()), (d, c0)
        assert [c for c in _chunks(d) if not live[hs[c[0]:c[1]]].any()] == ([] if d == 4096 else [_chunks(d)[-1]])
    hs = row_slots(g, row[2048])
    assert alive[row[2048]] and alive[g.col[hs]].any() and not live[hs].any()  # fires a = v / 1
    hs = row_slots(g, row[2047])
    assert not alive[row[2047]] and alive[g.col[hs]].all() and not live[hs].any()
    hh = np.concatenate([[k for k in row_slots(g, h) if g.degrees[g.col[k]] > TILE_HEAVY_DEG] for h in heavy_rows(g)])
    assert len(hh) == 30 and live[hh].any() and not live[hh].all()
    assert live[[k for k in row_slots(g, row[4096]) if g.col[k] == row[4097]]].all()  # both ends in kc_heavy
    assert 64 < int(live[row_slots(g, row[129])].sum()) < 129


def test_chunk_edge_topologies_b_and_c():
    g, alive, live = _live("B")
    row = chunk_edge_rows()
    hs = row_slots(g, row[2049])
    assert alive[row[2049]] and np.flatnonzero(live[hs]).tolist() == [C]  # the divisor is 2
    hs = row_slots(g, row[4096])
    assert alive[row[4096]] and not live[hs[C:2 * C]].any() and live[hs[:C]].sum() > C // 2
    g, alive, live = _live("C")
    hs = row_slots(g, row[2049])
    assert alive[row[2049]] and np.flatnonzero(~live[hs]).tolist() == [C]
    hs = row_slots(g, row[4097])
    assert alive[row[4097]] and not live[hs[C:2 * C]].any() and live[hs[:C]].sum() > C // 2 and live[hs[2 * C]]


def test_chunk_edge_script_mixes_the_states_in_one_chunk():
    """From the restatement: before the round that follows the revival every row above one chunk
    holds UP, DOWN and FRESH slots in one chunk, DOWN slots become FRESH on both sides of a chunk
    boundary (the one-slot last chunks of the 2049 and 4097 rows among them), in that round the S
    chain is not zero where the first chunk ends, and after the rounds that follow the row's flows
    differ on the two sides: a carry that restarts per chunk gives another estimate."""
    g, _, script, ref = chunk_edge_case("uniform")
    assert [s[0] for s in script] == ["run", "topology", "run", "run", "topology", "run", "run", "reset", "run"]
    assert script[CHUNK_EDGE_REVIVAL][0] == "topology" and script[CHUNK_EDGE_REVIVAL - 3][0] == "topology"
    row = chunk_edge_rows()
    before, st = ref.steps[CHUNK_EDGE_REVIVAL - 1], ref.steps[CHUNK_EDGE_REVIVAL]
    for d in (2049, 4096, 4097):
        hs = row_slots(g, row[d])
        mixed = [c for c in _chunks(d) if set(st.state[hs[c[0]:c[1]]].tolist()) == {UP, DOWN, FRESH}]
        assert (0, C) in mixed and (d == 2049 or len(mixed) == 2), (d, mixed)
        ks = [k for k in hs[:C] if st.state[k] == UP]
        S = 0.0
        for k in ks:
            S = S + -st.f[g.rev[k]]
        assert S != 0.0
        assert st.state[hs[d - 1]] == FRESH and before.state[hs[d - 1]] == DOWN
        after = ref.steps[CHUNK_EDGE_REVIVAL + 2]
        flows = [after.f[hs[c0:c1]][st.state[hs[c0:c1]] != DOWN] for c0, c1 in _chunks(d)]
        assert all(len(f) for f in flows) and not any(np.isin(f, flows[0]).all() for f in flows[1:]), d
    assert ((before.state == DOWN) & (st.state == FRESH)).sum() > 100
    was, now = script[1][1] != 0, script[CHUNK_EDGE_REVIVAL][1] != 0
    after = ref.steps[CHUNK_EDGE_REVIVAL + 1]
    assert (~was & now).sum() > 100 and (~now).sum() > 100
    assert (after.a[~was & now] != st.a[~was & now]).all()  # the revived fire again
    assert np.array_equal(after.a[~now], ref.steps[0].a[~now])  # the dead keep the estimate of round 2
    assert (ref.steps[7].state != UP).all() and not ref.steps[7].a.any()  # the reset


@pytest.mark.parametrize("family", ["subn", "special"])
def test_chunk_edge_value_families_reach_a_heavy_row(family):
    g, v, _, ref = chunk_edge_case(family)
    per_row = {d: np.concatenate([f[row_slots(g, h)] for f in ref.f_rounds]) for d, h in chunk_edge_rows().items()}
    if family == "subn":
        assert any(count_neg_zero(f) > 0 for d, f in per_row.items() if d > C)
        assert count_neg_zero(np.concatenate(ref.a_rounds)) > 0
    else:
        assert count_neg_zero(v) == 1 and np.isinf(v).sum() == 2 and np.isnan(v).sum() == 1
        assert any(np.isnan(f).any() for d, f in per_row.items() if d > C)
        assert np.isfinite(np.concatenate(ref.f_rounds)).any() and np.isfinite(ref.a).any()


# ------------------------------------------------------------------------------------
# the flapping run
# ------------------------------------------------------------------------------------
def test_flapping_run_flaps():
    g, _, script, ref = flapping_case()
    assert [s[0] for s in script] == ["topology", "run"] * FLAP_ROUNDS
    h = tile_segment("heavy")[0]
    assert all(s[1][h] for s in script[::2])
    at_call = np.stack([s.state for s in ref.steps[::2]])  # the states that round r runs on
    after = np.stack([s.state for s in ref.steps[1::2]])
    assert not (after == FRESH).any()
    want = [UP, DOWN, FRESH, UP, DOWN]
    hit = np.zeros(g.E, dtype=bool)
    for r in range(FLAP_ROUNDS - len(want) + 1):
        hit |= np.all(at_call[r:r + len(want)] == np.array(want)[:, None], axis=0)
    assert hit.any() and hit[row_slots(g, h)].any()  # in a light tile and on the heavy row
    # the round counter at a topology call is its index: both parities of the double buffer
    assert {r & 1 for r in range(FLAP_ROUNDS)} == {0, 1}
    fresh = at_call == FRESH
    twice = [k for k in np.flatnonzero(fresh.sum(axis=0) >= 2) if np.diff(np.flatnonzero(fresh[:, k])).max() > 1]
    assert twice
    # a DOWN slot of round r that is FRESH in r+1, on an even and on an odd r
    assert {r & 1 for r in range(FLAP_ROUNDS - 1) if ((at_call[r] == DOWN) & (at_call[r + 1] == FRESH)).any()} == {0, 1}
