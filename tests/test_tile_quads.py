"""Kernel 8's light tiles take their flows by global 4-aligned quads (16-byte accesses, four
consecutive edges per lane). A quad at a tile boundary holds edges of two
tiles, and the neighbouring tile may rewrite its own in place at the same time, so what
matters here is where the tiles start and end relative to the quads: every start residue
e0 % 4, tiles of exactly 1024 edges that start off a quad boundary (257 quads for 256
lanes), tiles of one node, last tiles of 1, 2 and 3 edges, and the arrays' tails
(E % 4 != 0). The device reports no tile bounds, so the cut rule is restated below and the
geometry asserted on the CPU; everything else is bitwise against the C oracle through the
C ABI with kernel 8 forced."""
import functools

import numpy as np
import pytest

import coracle
import fu
from parity_util import _er_with_outlier_pairs, assert_same_bits

pytestmark = pytest.mark.gpu

TE, TN = 1024, 128  # kernel 8's tile: edges x rows (csrc/fu_tuning.h)


def light_tiles(rowptr, hub_threshold=128):
    """FP::build_stage_light restated: rows of more than min(hub_threshold, TE) edges are
    heavy rows (tiles of their own, another kernel); the other rows are cut greedily into
    tiles of at most TN rows and TE edges. Returns [(row0, row1, e0, e1)]."""
    rp = [int(x) for x in rowptr]
    n, lim, out, i = len(rp) - 1, min(hub_threshold, TE), [], 0
    while i < n:
        if rp[i + 1] - rp[i] > lim:
            i += 1
            continue
        b = i
        while i < n and i - b < TN:
            if rp[i + 1] - rp[i] > lim or rp[i + 1] - rp[b] > TE:
                break
            i += 1
        out.append((b, i, rp[b], rp[i]))
    return out


def whole_quads(tiles):
    """First edges of the quads that lie wholly inside one light tile."""
    q = [np.arange((e0 + 3) // 4 * 4, e1 // 4 * 4, 4) for _, _, e0, e1 in tiles if e1 - e0 >= 4]
    return np.concatenate(q) if q else np.zeros(0, dtype=np.int64)


def _stage(g, v, hub_threshold=None):
    eng = fu.CollectAll(g, v, kernel="stage", hub_threshold=hub_threshold)
    assert eng.info()["kernel"] == "stage", eng.info()
    return eng


# ------------------------------------------------------------------------------------
# ER(5000, 20000)
# ------------------------------------------------------------------------------------
ER_SEED = 1


@functools.lru_cache(maxsize=None)
def _er_case():
    g = fu.Graph.erdos_renyi(5000, 20000, seed=ER_SEED)
    v = fu.uniform_values(g.n, seed=ER_SEED)
    rounds = {r: coracle.ca_sync(g.rowptr, g.col, g.rev, v, r) for r in range(1, 27)}
    return g, v, rounds


def test_er_every_start_residue_and_the_array_tails():
    """Rounds 1 and 2 compute the old flows (fm) and store both words; from round 3 on the
    flows are read and their high words stored only where they changed."""
    g, v, ref = _er_case()
    tiles = light_tiles(g.rowptr)
    assert {e0 % 4 for _, _, e0, _ in tiles} == {0, 1, 2, 3}, "pick another seed"
    assert g.E % 4 != 0, "pick another seed"
    assert len(tiles) > 8  # more than one block per XCD slot
    eng = _stage(g, v)
    done = 0
    for r in (1, 2, 3, 4, 5, 6, 25):
        eng.run(r - done)
        done = r
        assert_same_bits(eng.estimates(), ref[r][0], ("a", r))
        assert_same_bits(eng.flows(), ref[r][1], ("f", r))
    eng.close()


def test_er_error_reduction_every_round():
    """err_every = 1: the tile kernel's CHECK instantiation, against the oracle's trace."""
    g, v, ref = _er_case()
    tgt, _ = fu.component_means(g.rowptr, g.col, v)
    eng = _stage(g, v)
    eng.set_targets(tgt)
    tr = eng.run(26, err_every=1)
    # entry k: after round k (round 0 is the first), i.e. after k + 1 rounds
    want = np.array([np.max(np.abs(ref[k + 1][0] - tgt)) for k in range(26)])
    assert_same_bits(np.asarray(tr, dtype=np.float64), want)
    assert_same_bits(eng.estimates(), ref[26][0])
    assert_same_bits(eng.flows(), ref[26][1])
    eng.close()


# ------------------------------------------------------------------------------------
# hand-built tiles
# ------------------------------------------------------------------------------------
HUB = 64  # hub_threshold of the hand-built graphs: a row of 65 edges is a heavy row
LEAVES = 200


def _rows_graph(front, back):
    """Rows of prescribed degrees: `front` rows first, then LEAVES leaf rows, then `back`
    rows; every edge joins a prescribed row and a leaf (dealt round-robin, so the leaves'
    degrees differ by at most one)."""
    degs = list(front) + list(back)
    ids = list(range(len(front))) + list(range(len(front) + LEAVES, len(front) + LEAVES + len(back)))
    assert max(degs) <= LEAVES
    src, dst, nxt = [], [], 0
    for i, d in zip(ids, degs):
        src.append(np.full(d, i))
        dst.append(len(front) + (nxt + np.arange(d)) % LEAVES)
        nxt += d
    n = len(front) + LEAVES + len(back)
    g = fu.Graph.from_edges(n, np.concatenate(src), np.concatenate(dst))
    deg = np.diff(g.rowptr)
    assert [int(deg[i]) for i in ids] == degs
    assert int(deg[len(front):len(front) + LEAVES].max()) <= HUB  # the leaves are light rows
    return g


# front rows (tiles as light_tiles cuts them; a heavy row ends a tile too):
#   [3] + 15 x [64]      963 edges at e0 = 0
#   16 x [64]           1024 edges at e0 = 963  (residue 3: 257 quads)
#   [5]                 one node, 5 edges at e0 = 1987 (residue 3), then a heavy row of 65
#   15 x [64] + [63]    1023 edges at e0 = 2057 (residue 1)
#   16 x [64]           1024 edges at e0 = 3080 (residue 0: 256 quads)
#   15 x [64] + [61]    1021 edges at e0 = 4104 (residue 0)
#   15 x [64] + [61]    1021 edges at e0 = 5125 (residue 1)
#   [64] + [2]          e0 = 6146 (residue 2); the leaves follow in the same tile
FRONT = ([3] + [64] * 15 + [64] * 16 + [5, 65] + [64] * 15 + [63] + [64] * 16 + ([64] * 15 + [61]) * 2
         + [64, 2])


@pytest.mark.parametrize("last", [1, 2, 3])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_hand_built_tiles(last, shift):
    """`shift` rows of one edge after the first row move every tile boundary by `shift`
    edges; the back rows are a heavy row and one row of `last` edges, so the last tile has
    one node and 1, 2 or 3 edges."""
    g = _rows_graph(FRONT[:1] + [1] * shift + FRONT[1:] if shift else FRONT, [65, last])
    tiles = light_tiles(g.rowptr, HUB)
    by_e0 = {e0: (r1 - r0, e1 - e0) for r0, r1, e0, e1 in tiles}
    if shift == 0:
        assert by_e0[0] == (16, 963) and by_e0[963] == (16, 1024) and by_e0[1987] == (1, 5)
        assert by_e0[2057] == (16, 1023) and by_e0[3080] == (16, 1024)
        assert by_e0[4104] == (16, 1021) and by_e0[5125] == (16, 1021) and 6146 in by_e0
    # a tile of TE edges that starts off a quad boundary: 257 quads (the bound: TE / 4 + 1)
    assert any(e1 - e0 == TE and e0 % 4 for _, _, e0, e1 in tiles)
    assert max((e1 + 3) // 4 - e0 // 4 for _, _, e0, e1 in tiles) == TE // 4 + 1
    assert any(r1 - r0 == 1 for r0, r1, _, _ in tiles)                 # a tile of one node
    assert tiles[-1][3] == g.E and tiles[-1][3] - tiles[-1][2] == last  # the last tile
    assert tiles[-1][1] - tiles[-1][0] == 1
    # neighbouring light tiles meet at every residue
    ends = {e1 for _, _, _, e1 in tiles}
    assert {e0 % 4 for _, _, e0, _ in tiles if e0 in ends} == {0, 1, 2, 3}
    v = fu.uniform_values(g.n, seed=7 + last)
    eng = _stage(g, v, hub_threshold=HUB)
    for r in range(1, 13):  # a stale or clobbered boundary word shows in a later round
        eng.run(1)
        a_ref, f_ref = coracle.ca_sync(g.rowptr, g.col, g.rev, v, r)
        assert_same_bits(eng.estimates(), a_ref, ("a", r))
        assert_same_bits(eng.flows(), f_ref, ("f", r))
    eng.close()


# ------------------------------------------------------------------------------------
# packed tables and the conditional high-word store
# ------------------------------------------------------------------------------------
def _hi(f):
    return np.ascontiguousarray(f).view(np.uint64) >> np.uint64(32)


def test_packed_widths_and_both_high_word_store_forms():
    """The input of test_stage_forced_layouts_bitwise, with a packing plan every round
    (pack_every 1). The table of this graph is still unpacked after 100 rounds (the codes need
    the estimates within 2^32 keys of each other), so the first part runs, in steps of 5
    rounds and for 60 rounds at least, until the widths 32, 16 and 8 have all been in use (with
    escapes: the far-off pairs never enter the window); then 40 more rounds with the table
    converged. Round r rewrites f_{r-2} in place: a whole quad's high words go out as one
    16-byte store when all four changed, word by word when fewer did, and by the oracle's
    flows both happen during the run (on this graph no high word changes after round ~230:
    the last rounds store low words only)."""
    g, v = _er_with_outlier_pairs(60_000, 240_000, 32, seed=11)
    q = whole_quads(light_tiles(g.rowptr, 16))
    assert len(q) > 1000
    eng = _stage(g, v, hub_threshold=16)
    eng.set_option("pack_every", 1)
    seen, r1 = set(), 0
    while r1 < 60 or (not {8, 16, 32} <= seen and r1 < 600):
        eng.run(5)
        r1 += 5
        seen.update(eng.pack_widths())
    assert {8, 16, 32} <= seen, (seen, r1)
    got = {r1: (eng.estimates(), eng.flows())}
    eng.run(40)
    got[r1 + 40] = (eng.estimates(), eng.flows())
    assert eng.pack_widths()[2] == 8
    eng.close()
    # the oracle, round by round: f after r rounds against f after r - 2
    a, f = coracle.ca_sync(g.rowptr, g.col, g.rev, v, 2, nthreads=16)
    prev2, prev1 = coracle.ca_sync(g.rowptr, g.col, g.rev, v, 1, nthreads=16)[1], f.copy()
    all4 = some = 0  # whole quads whose four high words changed / of which one to three did
    for r in range(3, r1 + 41):
        coracle.ca_rounds(g.rowptr, g.col, g.rev, v, 1, a, f, nthreads=16)
        ch = (_hi(f) != _hi(prev2)).astype(np.int32)
        cnt = ch[q] + ch[q + 1] + ch[q + 2] + ch[q + 3]
        all4 += int(np.count_nonzero(cnt == 4))
        some += int(np.count_nonzero((cnt > 0) & (cnt < 4)))
        prev2, prev1 = prev1, f.copy()
        if r in got:
            assert_same_bits(got[r][0], a, ("a", r))
            assert_same_bits(got[r][1], f, ("f", r))
    print("rounds", r1, "+ 40; quads with all four / one to three high words changed:", all4, some)
    assert all4 > 0 and some > 0, (all4, some)
