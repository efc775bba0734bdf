"""Conditions on the inputs of the batched, lossy and pairwise engines' GPU cases, from host code
and the Python restatements alone: that a graph really holds the rows, tiles and pairs for
which a case was built. No engine runs here, so nothing needs a GPU; the cases themselves are in
test_lossy_gpu.py, test_pair_gpu.py and test_batch_gpu.py."""
import collections

import numpy as np
import pytest

import fu
from lossy_cases import SEED as LOSS_SEED
from lossy_cases import TILE_ROWS, TILE_SLOTS, tile_census, tile_limit_graph, tile_segment
from pair_cases import (CLASS_DEGREES, CLASS_ROUNDS, LAST_SLOT_ROUNDS, LAST_SLOT_SEED, SEED, class_graph, dense66,
                        pair_count, pairs_of_round)
from parity_util import (BATCH_BOUNDARY_DEGREES, BATCH_LIGHT_DEGREES, _batch_boundary_graph, _class_edge_graph,
                         batch_chunk_degrees)


# ------------------------------------------------------------------------------------
# lossy: the light tiles
# ------------------------------------------------------------------------------------
def test_tile_census_on_hand_made_rows():
    """The restated plan on rowptrs small enough to read: each way a tile closes, heavy rows
    in no tile, and the order of the tests where two limits are met at once."""
    def rowptr(degrees):
        return np.concatenate([[0], np.cumsum(degrees)])

    assert tile_census(rowptr([2, 0, 3])) == [(0, 3, 5, "end")]
    assert tile_census(rowptr([1] * 256)) == [(0, 256, 256, "end")]
    assert tile_census(rowptr([1] * 257)) == [(0, 256, 256, "rows"), (256, 257, 1, "end")]
    assert tile_census(rowptr([128] * 17)) == [(0, 16, 2048, "slots"), (16, 17, 128, "end")]
    assert tile_census(rowptr([129, 5, 129, 129, 7, 7])) == [(1, 2, 5, "heavy"), (4, 6, 14, "end")]
    assert tile_census(rowptr([8] * 256 + [1])) == [(0, 256, 2048, "rows"), (256, 257, 1, "end")]
    assert tile_census(rowptr([8] * 255 + [9, 1])) == [(0, 255, 2040, "slots"), (255, 257, 10, "end")]
    assert tile_census(rowptr([129])) == []


def test_tile_limit_graph_closes_tiles_in_every_way():
    g = tile_limit_graph()
    tiles = tile_census(g.rowptr)
    heavy = tile_segment("heavy")[0]
    rows = sum(j - i for i, j, _, _ in tiles)
    assert rows == g.n - 1 and all(not i <= heavy < j for i, j, _, _ in tiles)  # every row but the heavy one, once
    assert all(g.rowptr[j] - g.rowptr[i] == ne and j - i <= TILE_ROWS and ne <= TILE_SLOTS for i, j, ne, _ in tiles)
    full = [(i, j, ne) for i, j, ne, _ in tiles if j - i == TILE_ROWS]
    assert any(ne == 0 for _, _, ne in full)
    assert any(0 < ne < TILE_SLOTS for _, _, ne in full)
    assert any(ne == TILE_SLOTS for _, _, ne in full)
    why = collections.Counter(w for _, _, _, w in tiles)
    assert why["rows"] >= 3 and why["slots"] >= 1 and why["heavy"] >= 1 and why["end"] == 1
    assert (tile_segment("rr8")[0], tile_segment("rr8")[0] + TILE_ROWS, TILE_SLOTS, "rows") in tiles  # the masked tile
    assert tiles[-1][1] == g.n and g.degrees[-1] == 0  # the end tile's last rows are isolated


def test_loss_reaches_every_tile_kind():
    """fu_lossy_delivered at p = 0.25 within rounds 1-8: every tile with a slot has a lost and a
    delivered slot, and the 256th row of every full tile with a slot has a lost one (so thread
    255 runs a chain that differs from the lossless one)."""
    g = tile_limit_graph()
    D = np.stack([fu.lossy_delivered(LOSS_SEED, r, 0, g.E, 0.25) for r in range(1, 9)]).astype(bool)
    full = 0
    for i, j, ne, _ in tile_census(g.rowptr):
        if ne == 0:
            continue
        part = D[:, g.rowptr[i]:g.rowptr[j]]
        assert part.any() and not part.all(), (i, j)
        if j - i == TILE_ROWS:
            full += 1
            last = D[:, g.rowptr[j - 1]:g.rowptr[j]]
            assert last.size and not last.all(), (i, j)
    assert full >= 5


def test_class_edge_graph_has_no_tile_at_the_row_limit():
    """What the cases on tile_limit_graph() add: on the class graph of test_lossy_gpu.py the slot
    limit closes every tile but two, and no tile holds 256 rows or no slot."""
    tiles = tile_census(_class_edge_graph(7).rowptr)
    why = collections.Counter(w for _, _, _, w in tiles)
    assert why["rows"] == 0 and why["heavy"] == 1 and why["end"] == 1 and why["slots"] == len(tiles) - 2
    assert max(j - i for i, j, _, _ in tiles) < TILE_ROWS
    assert min(ne for _, _, ne, _ in tiles) > 0


# ------------------------------------------------------------------------------------
# pairwise: many heavy pairs, and the chunks of a long listener row
# ------------------------------------------------------------------------------------
def test_dense66_lists_more_than_1024_heavy_pairs_every_round():
    g = dense66()
    assert g.n == 6144 and g.E == 6144 * 66 and (g.degrees == 66).all()
    for r in range(6):
        pairs = pairs_of_round(*g.arrays(), SEED, r)
        assert len(pairs) > 1024, (r, len(pairs))  # more pairs than blocks: the list loop's second pass
        mate, initiator = fu.pair_matching(g, SEED, r)  # the host's own matching counts the same
        assert int(initiator.sum()) == len(pairs) and int((mate >= 0).sum()) == 2 * len(pairs)
    assert pair_count(*g.arrays(), SEED, 6) > 6 * 1024


def _slots_of(g, c, seed, rounds):
    """(slots on which node c fired as initiator, as listener) within `rounds` rounds."""
    ini, lis = [], []
    for r in range(rounds):
        for i, s, j, t in pairs_of_round(*g.arrays(), seed, r):
            if i == c:
                ini.append(s)
            if j == c:
                lis.append(t)
    return ini, lis


def test_class_graph_long_rows_answer_from_every_chunk():
    """The listener's sum runs over chunks of 1024 slots with -F1 in slot t's place. Within
    CLASS_ROUNDS rounds at SEED the centre of degree 2500 listens on a slot of its second chunk
    and on one of its third, and initiates on a slot past the first chunk."""
    g = class_graph()
    ini, lis = _slots_of(g, CLASS_DEGREES.index(2500), SEED, CLASS_ROUNDS)
    assert any(1024 <= t < 2048 for t in lis) and any(t >= 2048 for t in lis)
    assert any(s >= 1024 for s in ini)


def test_class_graph_last_slot_of_1025_needs_its_own_seed():
    """The centre of degree 1025 has one slot in its second chunk, slot 1024. At SEED it never
    listens on it within CLASS_ROUNDS rounds; at LAST_SLOT_SEED it does within LAST_SLOT_ROUNDS,
    in the run's last round but one; that is the seed of test_pair_gpu.py's extra case."""
    g = class_graph()
    c = CLASS_DEGREES.index(1025)
    assert 1024 not in _slots_of(g, c, SEED, CLASS_ROUNDS)[1]
    hit = [r for r in range(LAST_SLOT_ROUNDS)
           if any(j == c and t == 1024 for _, _, j, t in pairs_of_round(*g.arrays(), LAST_SLOT_SEED, r))]
    assert LAST_SLOT_ROUNDS - 2 in hit


# ------------------------------------------------------------------------------------
# batched: every K against its chunk edges
# ------------------------------------------------------------------------------------
def test_batch_boundary_graph_has_exactly_the_listed_centres():
    g = _batch_boundary_graph()
    k = len(BATCH_BOUNDARY_DEGREES)
    assert [int(d) for d in g.degrees[:k]] == BATCH_BOUNDARY_DEGREES
    assert len(set(BATCH_BOUNDARY_DEGREES)) == k and BATCH_BOUNDARY_DEGREES[-1] == 4097
    assert set(BATCH_LIGHT_DEGREES) <= set(BATCH_BOUNDARY_DEGREES)
    assert int(g.col[:g.rowptr[k]].min()) >= k  # a centre's neighbours are leaves
    assert g.n == k + 6000


@pytest.mark.parametrize("K", range(1, 17))
def test_batch_boundary_graph_has_the_chunk_edges_of_every_width(K):
    ce = 2048 // K
    want = batch_chunk_degrees(K)
    assert want == [ce - 1, ce, ce + 1, 2 * ce - 1, 2 * ce, 2 * ce + 1]
    deg = set(int(d) for d in _batch_boundary_graph().degrees[:len(BATCH_BOUNDARY_DEGREES)])
    for d in want:
        assert d in deg and d > 64, (K, d)  # a heavy row: one block, chunks of ce edges
    assert (ce + 1) * K > 2048 >= ce * K  # ce + 1 edges are the first that do not fit one chunk
