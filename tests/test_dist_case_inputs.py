"""fu.dist.split_ranges / partition on cuts that are not balanced slabs, and the conditions of
the named cut cases (dist_cases.py) that test_dist_gloo.py and test_dist_cuts_gpu.py run, from
the plans alone: n_local, e_local, n_ghost_a, the per-peer send and receive counts, the row
degrees and "every neighbour of the row is a ghost". A case can then never quietly stop
reaching the count it was built for. Nothing here needs a GPU."""
import ctypes

import numpy as np
import pytest

import fu
from conftest import ca_sync_fixtures, load_npz
from dist_cases import (CASES, ISLAND_BLOCKS, RMAT_HUB, RMAT_MEGA, SLIVER_WIDTHS, case, check_plan_symmetry,
                        peer_counts, plans, rows_all_ghost, star)
from fu.dist import partition, split_ranges


# ------------------------------------------------------------------------------------
# 1. split_ranges and partition
# ------------------------------------------------------------------------------------
def old_split_ranges(rowptr, nranks, balance="edges"):
    """The formula before empty ranks were refused (restated): nothing keeps two bounds apart."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = len(rowptr) - 1
    if balance == "nodes":
        return np.array([(n * p) // nranks for p in range(nranks + 1)], dtype=np.int64)
    work = rowptr + np.arange(n + 1, dtype=np.int64)
    targets = [(work[-1] * p) // nranks for p in range(nranks + 1)]
    b = np.searchsorted(work, targets, side="left").astype(np.int64)
    b[0], b[-1] = 0, n
    return np.maximum.accumulate(b)


def _path(n):
    return fu.Graph.from_edges(n, np.arange(n - 1), np.arange(1, n))


def _hub_graphs():
    d = load_npz(dict(ca_sync_fixtures())["rmat9_ef8"]["file"])
    out = {f"star{n}_hub_{where}": star(n, 0 if where == "first" else n - 1).arrays()
           for n in (257, 1500) for where in ("first", "last")}
    out["path40"] = _path(40).arrays()
    rp, col = np.asarray(d["rowptr"], dtype=np.int64), np.asarray(d["col"], dtype=np.int32)
    out["rmat9_ef8"] = fu.Graph.from_csr(rp, col).arrays()
    return out


HUB_GRAPHS = _hub_graphs()


def test_old_formula_left_ranks_empty():
    """The defect: the rows of the issue's table, from the restated old formula."""
    rp = HUB_GRAPHS["star257_hub_first"][0]
    assert old_split_ranges(rp, 8).tolist() == [0, 1, 1, 17, 65, 113, 161, 209, 257]
    assert old_split_ranges(HUB_GRAPHS["star1500_hub_first"][0], 8).tolist() == [0, 1, 1, 94, 376, 657, 938, 1219, 1500]
    assert old_split_ranges(HUB_GRAPHS["star257_hub_last"][0], 4).tolist() == [0, 96, 192, 257, 257]
    assert old_split_ranges(HUB_GRAPHS["star1500_hub_last"][0], 8).tolist() == [0, 281, 562, 843, 1125, 1406, 1500, 1500, 1500]


@pytest.mark.parametrize("balance", ["edges", "nodes"])
@pytest.mark.parametrize("world", range(2, 9))
@pytest.mark.parametrize("name", sorted(HUB_GRAPHS))
def test_split_ranges_leaves_no_rank_empty(name, world, balance):
    rp, col, rev = HUB_GRAPHS[name]
    n = len(rp) - 1
    b = split_ranges(rp, world, balance=balance)
    assert b.dtype == np.int64 and b.shape == (world + 1,)
    assert b[0] == 0 and b[-1] == n and (np.diff(b) >= 1).all(), b
    old = old_split_ranges(rp, world, balance)
    if (np.diff(old) >= 1).all():
        assert np.array_equal(b, old)
    else:  # a bound moves only as far as the nearest row that keeps one row per rank
        assert (np.abs(b - old) <= world).all(), (b, old)
    if balance == "edges":
        ps = [partition(rp, col, rev, world, r) for r in range(world)]
        assert [(p.lo, p.hi) for p in ps] == list(zip(b[:-1].tolist(), b[1:].tolist()))
        check_plan_symmetry(rp, ps)


def test_split_ranges_hub_bounds():
    assert split_ranges(HUB_GRAPHS["star257_hub_first"][0], 8).tolist() == [0, 1, 2, 17, 65, 113, 161, 209, 257]
    assert split_ranges(HUB_GRAPHS["star257_hub_last"][0], 4).tolist() == [0, 96, 192, 256, 257]
    assert split_ranges(HUB_GRAPHS["star1500_hub_last"][0], 8).tolist() == [0, 281, 562, 843, 1125, 1406, 1498, 1499, 1500]
    assert split_ranges(_path(8).rowptr, 8).tolist() == list(range(9))


@pytest.mark.parametrize("kind", ["er", "rgg", "rmat"])
def test_split_ranges_unchanged_on_the_suite_graphs(kind):
    """The graphs the GPU partition tests and the README numbers cut with the default bounds:
    the old formula is strictly increasing there (the condition that makes the comparison say
    something), and split_ranges returns exactly its bounds."""
    g = {"er": lambda: fu.Graph.erdos_renyi(60_000, 240_000, seed=21),
         "rgg": lambda: fu.Graph.random_geometric(200_000, avg_deg=8, seed=21),
         "rmat": lambda: fu.Graph.rmat(14, 16, seed=3)}[kind]()
    for world in (2, 3, 8):
        for balance in ("edges", "nodes"):
            old = old_split_ranges(g.rowptr, world, balance)
            assert old[0] == 0 and old[-1] == g.n and (np.diff(old) >= 1).all(), (world, balance, old)
            assert np.array_equal(split_ranges(g.rowptr, world, balance=balance), old), (world, balance)


@pytest.mark.parametrize("balance", ["edges", "nodes"])
def test_split_ranges_refuses_fewer_nodes_than_ranks(balance):
    rp = _path(5).rowptr
    with pytest.raises(ValueError, match=r"\b5 nodes\b.*\b6 ranks\b"):
        split_ranges(rp, 6, balance=balance)
    with pytest.raises(ValueError, match=r"\b5 nodes\b.*\b8 ranks\b"):
        partition(*_path(5).arrays(), 8, 0)
    assert split_ranges(rp, 5, balance=balance).tolist() == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("bounds,rank", [([0, 20, 10, 40], 1),      # not monotone
                                         ([0, 10, 10, 40], 1),      # rank 1 empty
                                         ([0, 0, 10, 40], 0),       # rank 0 empty
                                         ([0, 10, 40, 40], 2),      # last rank empty
                                         ([1, 10, 20, 40], 0),      # does not start at 0
                                         ([0, 10, 20, 39], 2),      # does not end at n
                                         ([0, 10, 20, 41], 2)])
def test_partition_refuses_bad_bounds(bounds, rank, monkeypatch):
    """ValueError naming the rank, whichever rank asks for its plan; nothing reaches libfu."""
    from fu import _lib

    def no_call(name, *args):
        raise AssertionError(f"{name} called")

    monkeypatch.setattr(_lib, "call", no_call)
    rp, col, rev = HUB_GRAPHS["path40"]
    for r in range(3):
        with pytest.raises(ValueError, match=rf"\brank {rank}\b"):
            partition(rp, col, rev, 3, r, bounds=bounds)
    with pytest.raises(ValueError, match="entries"):
        partition(rp, col, rev, 3, 0, bounds=[0, 20, 40])


def test_create_local_refuses_an_empty_rank_before_any_device_call():
    """fu_dist_create_local with n_local = 0: FU_ERR_ARG (-1) from the argument check, on a host
    with or without a GPU (without one, a device call would answer FU_ERR_HIP, -2)."""
    off = np.zeros(3, dtype=np.int64)
    rp = np.zeros(1, dtype=np.int64)
    v = np.zeros(1)
    out = fu._lib.vp()
    with pytest.raises(fu.FuError) as ei:
        fu._lib.call("fu_dist_create_local", 0, 0, fu._lib.ptr(rp), None, fu._lib.ptr(v), 0, 2, 1,
                     fu._lib.ptr(off), None, fu._lib.ptr(off), 0, ctypes.byref(out))
    assert ei.value.code == -1, ei.value
    assert not out.value


# ------------------------------------------------------------------------------------
# 2. the named cut cases
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_case_bounds_and_plans(name):
    c, ps = case(name), plans(name)
    assert len(ps) == c.world and c.bounds[0] == 0 and c.bounds[-1] == c.g.n and (np.diff(c.bounds) >= 1).all()
    assert c.g.n <= 20000 and len(c.v) == c.g.n
    assert np.array_equal(c.v, fu.uniform_values(c.g.n, seed=5))
    check_plan_symmetry(c.g.rowptr, ps)
    for p in ps:
        assert (p.lo, p.hi) == (c.bounds[p.rank], c.bounds[p.rank + 1])
        assert p.e_local == c.g.rowptr[p.hi] - c.g.rowptr[p.lo]


@pytest.mark.parametrize("name", ["star_hub_alone", "star_hub_alone_mega"])
def test_star_hub_alone(name):
    c, ps = case(name), plans(name)
    assert c.bounds.tolist() == [0, 128, 256, 257] and c.world == 3
    assert c.options == ({"mega_hub": 64} if name.endswith("mega") else {})
    hub = ps[2]
    assert (hub.n_local, hub.e_local, hub.n_ghost_a) == (1, 256, 256)
    assert np.diff(hub.rowptr).tolist() == [256]  # > hub_threshold 128: no light tile; > mega_hub 64
    assert (hub.col >= hub.n_local).all()
    for p in ps[:2]:
        assert (p.n_local, p.e_local, p.n_ghost_a) == (128, 128, 1)
        assert (np.diff(p.rowptr) == 1).all() and rows_all_ghost(p).all()  # boundary tiles only
        sent, recv = peer_counts(p)
        assert sent.tolist() == [0, 0, 128] and recv.tolist() == [0, 0, 1]
    assert peer_counts(hub)[0].tolist() == [1, 1, 0] and peer_counts(hub)[1].tolist() == [128, 128, 0]


def test_star_hub_first_w8():
    c, ps = case("star_hub_first_w8"), plans("star_hub_first_w8")
    assert c.world == 8 and np.array_equal(c.bounds, split_ranges(c.g.rowptr, 8))
    assert c.bounds.tolist() == [0, 1, 2, 94, 376, 657, 938, 1219, 1500]
    assert (ps[0].n_local, ps[0].e_local, ps[0].n_ghost_a) == (1, 1499, 1499)
    assert any(p.n_local < 64 for p in ps[1:])
    for p in ps[1:]:  # leaves only: ghost neighbours only, one peer
        assert rows_all_ghost(p).all() and p.n_ghost_a == 1
        assert peer_counts(p)[0].tolist() == [p.n_local] + [0] * 7


def test_islands_w4():
    c, ps = case("islands_w4"), plans("islands_w4")
    assert np.diff(c.bounds).tolist() == list(ISLAND_BLOCKS) and c.world == 4
    assert ps[1].e_local > 0 and ps[1].n_ghost_a == 0 and len(ps[1].send_a_idx) == 0
    assert ps[2].e_local == 0 and ps[2].n_ghost_a == 0 and len(ps[2].send_a_idx) == 0
    assert ps[2].n_local == 300 and (np.diff(ps[2].rowptr) == 0).all()
    s0, r0 = peer_counts(ps[0])
    s3, r3 = peer_counts(ps[3])
    assert s0[1] == s0[2] == 0 and r0[1] == r0[2] == 0 and s0[3] > 0 and r0[3] == 700
    assert s3[1] == s3[2] == 0 and r3[1] == r3[2] == 0 and s3[0] == 700 and r3[0] == s0[3]
    # the zero-count middle peers leave the later peer's offset where it was
    assert ps[0].recv_a_off.tolist() == [0, 0, 0, 0, 700] and ps[3].recv_a_off.tolist() == [0, r3[0], r3[0], r3[0], r3[0]]
    assert rows_all_ghost(ps[3]).all()  # the last block is wired to the first block only
    assert not rows_all_ghost(ps[0]).any() and ps[0].n_ghost_a < ps[0].n_local
    # two components with edges, and 300 of one node each
    _, comp = fu.component_means(c.g.rowptr, c.g.col, c.v)
    assert len(np.unique(comp[2500:2800])) == 300 and not set(comp[1500:2500]) & set(comp[:1500])
    assert set(comp[2800:]) <= set(comp[:1500])


def test_slivers_w8():
    """The widths and the all-ghost rows as the case states them. Ranks two or more apart do
    share edges where one of them is a sliver: the generator numbers the nodes by cell, column
    after column, about 226 nodes to a column (sqrt(8 n / pi): it grows with n), so the
    neighbours of any run of fewer rows than a column lie a whole column further on as well.
    No size of this graph keeps a 1-row rank to its two adjacent ranks; the widths are what the
    case is for, so they stay, and what is pinned here is what does hold: the two wide ranks
    behind the slivers hear only from their adjacent ranks (zero-count leading peers), and
    most slivers have a non-adjacent peer and a silent peer between two talking ones."""
    c, ps = case("slivers_w8"), plans("slivers_w8")
    assert c.world == 8 and np.diff(c.bounds)[:6].tolist() == list(SLIVER_WIDTHS)
    assert abs(int(ps[6].n_local) - int(ps[7].n_local)) <= 1
    for p in ps[:2]:
        assert p.e_local > 0 and rows_all_ghost(p).all() and p.n_ghost_a == len(np.unique(p.ghost_a_gid))
    for p in ps:
        assert p.e_local > 0 and p.n_ghost_a > 0
    assert np.nonzero(peer_counts(ps[7])[1])[0].tolist() == [6]
    assert np.nonzero(peer_counts(ps[6])[1])[0].tolist() == [5, 7]
    far = gaps = 0
    for p in ps[:5]:
        talk = np.nonzero(peer_counts(p)[1])[0]
        far += any(abs(int(q) - p.rank) >= 2 for q in talk)
        gaps += any(peer_counts(p)[1][q] == 0 for q in range(talk.min(), talk.max()) if q != p.rank)
    assert far >= 3 and gaps >= 3 and peer_counts(ps[0])[1].tolist() == [0, 2, 3, 0, 0, 2, 0, 0]
    # interior tiles exist only on the wide ranks: rows without a ghost in runs longer than two tiles
    assert int((~_has_ghost(ps[6])).sum()) > 9000


def _has_ghost(p):
    src = np.repeat(np.arange(p.n_local), np.diff(p.rowptr))
    out = np.zeros(p.n_local, dtype=bool)
    out[src[p.col >= p.n_local]] = True
    return out


def test_er_w8_ghost_heavy():
    c, ps = case("er_w8_ghost_heavy"), plans("er_w8_ghost_heavy")
    assert c.world == 8 and np.array_equal(c.bounds, split_ranges(c.g.rowptr, 8))
    for p in ps:
        sent, recv = peer_counts(p)
        others = [q for q in range(8) if q != p.rank]
        assert (sent[others] > 0).all() and (recv[others] > 0).all()
        assert p.n_ghost_a > 2 * p.n_local


def test_rmat_w8_hub_ranks():
    c, ps = case("rmat_w8_hub_ranks"), plans("rmat_w8_hub_ranks")
    assert c.world == 8 and np.array_equal(c.bounds, split_ranges(c.g.rowptr, 8))
    assert c.options == {"hub_threshold": RMAT_HUB, "mega_hub": RMAT_MEGA}
    deg = c.g.degrees
    assert (np.diff(deg) <= 0).all()  # the degree-descending relabelling
    hub_only = [p.rank for p in ps if (np.diff(p.rowptr) > RMAT_HUB).all()]
    light_only = [p.rank for p in ps if (np.diff(p.rowptr) <= RMAT_HUB).all()]
    assert hub_only and light_only and hub_only[0] == 0 and light_only[-1] == 7
    assert (np.diff(ps[0].rowptr) > RMAT_MEGA).any()  # mega hubs on the first rank
    assert any((np.diff(p.rowptr) > RMAT_HUB).any() and (np.diff(p.rowptr) <= RMAT_HUB).any() for p in ps)
    assert all(p.e_local > 0 and p.n_ghost_a > 0 for p in ps)
