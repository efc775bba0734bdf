"""Named cuts of small graphs for the partitioned collect-all path (fu.dist), shared by the CPU
checks of their conditions (test_dist_case_inputs.py), the CPU model of the partitioned rounds
(test_dist_gloo.py) and the GPU parity cases (test_dist_cuts_gpu.py). Each case is
(graph, values, bounds, world, options): the bounds are explicit wherever the case names its
cut, so it keeps its shape whatever fu.dist.split_ranges does later (three cases are about the
default cut and take it from there); values are fu.uniform_values at VALUE_SEED; options are the
fu_set_option keys the case runs with. Numpy and the host graph code only: nothing here
touches a GPU.

The per-rank counts these cuts drive to their edges (fu_plan.cpp, fu_ca_launch.h's launchers,
fu_dist.hip): the number of boundary light tiles 0 or all of them, no light tile at all, an
empty send list, a zero-count middle peer, many more ghost slots than rows, no edge.
"""
import collections
import functools

import numpy as np

import fu
from fu.dist import partition, split_ranges

VALUE_SEED = 5
Case = collections.namedtuple("Case", "g v bounds world options")

CASES = ("star_hub_alone", "star_hub_alone_mega", "star_hub_first_w8", "islands_w4", "slivers_w8",
         "er_w8_ghost_heavy", "rmat_w8_hub_ranks")

ISLAND_BLOCKS = (1500, 1000, 300, 700)          # islands_w4: rows per rank
SLIVER_WIDTHS = (1, 2, 63, 64, 65, 257)         # slivers_w8: rows of the six leading ranks
RMAT_HUB, RMAT_MEGA = 32, 256                   # rmat_w8_hub_ranks: hub_threshold, mega_hub


def star(n, hub):
    """Star of n nodes through from_csr: `hub` (0 or n - 1) is joined to every other node."""
    assert hub in (0, n - 1)
    leaves = np.arange(1, n) if hub == 0 else np.arange(n - 1)
    deg = np.ones(n, dtype=np.int64)
    deg[hub] = n - 1
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    col = np.empty(2 * (n - 1), dtype=np.int32)
    col[rowptr[leaves]] = hub
    col[rowptr[hub]:rowptr[hub + 1]] = leaves
    return fu.Graph.from_csr(rowptr, col)


def _undirected(g, shift=0):
    src = np.repeat(np.arange(g.n, dtype=np.int64), g.degrees)
    keep = src < g.col
    return src[keep] + shift, g.col[keep].astype(np.int64) + shift


def _islands():
    na, nb, nz, nd = ISLAND_BLOCKS
    sa, da = _undirected(fu.Graph.erdos_renyi(na, 6000, seed=31))
    sb, db = _undirected(fu.Graph.erdos_renyi(nb, 4000, seed=32), shift=na)
    # the last block: 700 more nodes of the first component, three links each, all of them into
    # the first block (none inside the block, none to the second component)
    rng = np.random.default_rng(33)
    sd = np.repeat(np.arange(nd, dtype=np.int64) + na + nb + nz, 3)
    dd = rng.integers(0, na, size=3 * nd)
    n = na + nb + nz + nd
    return fu.Graph.from_edges(n, np.concatenate([sa, sb, sd]), np.concatenate([da, db, dd]))


@functools.lru_cache(maxsize=None)
def case(name):
    """star_hub_alone / star_hub_alone_mega: star of 257 nodes, the hub last; world 3, bounds
        [0, 128, 256, 257]. Rank 2 is the hub alone (1 row, 256 edges, 256 ghosts, no light
        tile): a heavy row with the default options, a mega hub with mega_hub = 64. Ranks 0 and
        1: every row's only neighbour is a ghost (every light tile a boundary tile, no interior
        tile), and they exchange nothing with each other.
    star_hub_first_w8: star of 1500 nodes, the hub first; world 8, the bounds of split_ranges
        now that it leaves no rank empty ([0, 1, 2, 94, 376, 657, 938, 1219, 1500]; it gave
        [0, 1, 1, 94, ...] before): the hub alone on rank 0, one leaf alone on rank 1.
    islands_w4: 3500 nodes, world 4, bounds on the block edges: ER(1500, 6000); a second ER
        component ER(1000, 4000) with no edge to the rest; 300 nodes of degree 0; 700 more
        nodes of the first component, each linked to three nodes of the first block only.
        Rank 1 has edges, no ghost and sends nothing; rank 2 has no edge; ranks 0 and 3 talk
        only to each other, across the two silent ranks.
    slivers_w8: RGG(20000, average degree 8), world 8: ranks of 1, 2, 63, 64, 65 and 257 rows
        (either side of the tile heights 64, 128 and 256), the rest split in two. The rows of
        the 1- and 2-row ranks have ghost neighbours only.
    er_w8_ghost_heavy: ER(8000, 32000), world 8, the default bounds: every rank
        hears from all 7 peers and has more than twice as many ghost slots as rows.
    rmat_w8_hub_ranks: R-MAT(11, 16) relabelled by descending degree (fu_graph_relabel order 1),
        the relabelled graph cut at the default bounds, world 8, hub_threshold 32
        and mega_hub 256: the first ranks hold rows above 32 edges only, the last ones rows of
        at most 32 edges only.
    Every size is the one first tried: no case had to grow to meet its conditions."""
    options = {}
    if name in ("star_hub_alone", "star_hub_alone_mega"):
        g, world, bounds = star(257, 256), 3, [0, 128, 256, 257]
        if name.endswith("mega"):
            options = {"mega_hub": 64}
    elif name == "star_hub_first_w8":
        g, world = star(1500, 0), 8
        bounds = split_ranges(g.rowptr, world)
    elif name == "islands_w4":
        g, world = _islands(), 4
        bounds = np.concatenate([[0], np.cumsum(ISLAND_BLOCKS)])
    elif name == "slivers_w8":
        g, world = fu.Graph.random_geometric(20000, avg_deg=8, seed=9), 8
        lead = int(np.sum(SLIVER_WIDTHS))
        bounds = np.concatenate([[0], np.cumsum(SLIVER_WIDTHS), [lead + (g.n - lead) // 2, g.n]])
    elif name == "er_w8_ghost_heavy":
        g, world = fu.Graph.erdos_renyi(8000, 32000, seed=7), 8
        bounds = split_ranges(g.rowptr, world)
    elif name == "rmat_w8_hub_ranks":
        g, _ = fu.Graph.rmat(11, 16, seed=6).relabel("degree")
        world = 8
        bounds = split_ranges(g.rowptr, world)
        options = {"hub_threshold": RMAT_HUB, "mega_hub": RMAT_MEGA}
    else:
        raise KeyError(name)
    bounds = np.asarray(bounds, dtype=np.int64)
    bounds.setflags(write=False)
    v = fu.uniform_values(g.n, seed=VALUE_SEED)
    v.setflags(write=False)
    return Case(g, v, bounds, world, options)


@functools.lru_cache(maxsize=None)
def plans(name):
    c = case(name)
    return tuple(partition(c.g.rowptr, c.g.col, c.g.rev, c.world, r, bounds=c.bounds) for r in range(c.world))


def peer_counts(plan):
    """(sent to, received from) every rank: two int arrays of nranks entries."""
    return np.diff(plan.send_a_off), np.diff(plan.recv_a_off)


def rows_all_ghost(plan):
    """bool per local row: the row has a neighbour and every neighbour is a ghost."""
    src = np.repeat(np.arange(plan.n_local), np.diff(plan.rowptr))
    own = np.zeros(plan.n_local, dtype=np.int64)
    np.add.at(own, src[plan.col < plan.n_local], 1)
    return (np.diff(plan.rowptr) > 0) & (own == 0)


def check_plan_symmetry(rowptr, plans):
    """What rank p sends to q is what q expects from p, in q's slot order (estimates and
    flows); the counts agree; every local index is in range."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    for p in plans:
        for q in plans:
            if p.rank == q.rank:
                continue
            nf = p.send_f_off[q.rank + 1] - p.send_f_off[q.rank]
            assert nf == q.recv_f_off[p.rank + 1] - q.recv_f_off[p.rank], (p.rank, q.rank)
            sent_gidx = p.send_f_idx[p.send_f_off[q.rank]:p.send_f_off[q.rank + 1]] + rowptr[p.lo]
            exp = q.ghost_f_gidx[q.recv_f_off[p.rank]:q.recv_f_off[p.rank + 1]]
            assert np.array_equal(sent_gidx, exp), (p.rank, q.rank)
            na = p.send_a_off[q.rank + 1] - p.send_a_off[q.rank]
            assert na == q.recv_a_off[p.rank + 1] - q.recv_a_off[p.rank], (p.rank, q.rank)
            sent_a = p.send_a_idx[p.send_a_off[q.rank]:p.send_a_off[q.rank + 1]] + p.lo
            exp_a = q.ghost_a_gid[q.recv_a_off[p.rank]:q.recv_a_off[p.rank + 1]]
            assert np.array_equal(sent_a, exp_a), (p.rank, q.rank)
        assert p.send_a_off[p.rank + 1] == p.send_a_off[p.rank] and p.recv_a_off[p.rank + 1] == p.recv_a_off[p.rank]
        assert p.send_a_off[0] == 0 and p.send_a_off[-1] == len(p.send_a_idx)
        assert p.recv_a_off[0] == 0 and p.recv_a_off[-1] == p.n_ghost_a == len(p.ghost_a_gid)
        assert p.recv_f_off[-1] == p.n_ghost_f and len(p.rowptr) == p.n_local + 1 and p.rowptr[0] == 0
        assert len(p.col) == len(p.rev) == p.e_local
        if p.e_local:
            assert 0 <= p.col.min() and p.col.max() < p.n_local + p.n_ghost_a
            assert 0 <= p.rev.min() and p.rev.max() < p.e_local + p.n_ghost_f
        if len(p.send_a_idx):
            assert 0 <= p.send_a_idx.min() and p.send_a_idx.max() < p.n_local
