"""Rows whose neighbours are not in ascending id order, for every engine. The parity contract
rests on the row order: S = 0.0 + F.., T = 0.0 + E.. are summed left to right in the caller's
row order (CA:106, CA:110), and fu_graph_from_csr keeps that order. Every generator and
fu_graph_from_edges return ascending rows, so on the graphs the suite already trusts a path
that sums in ascending id order (slice order, bucket order, chunk order) cannot be told from
one that sums in row order. `reorder_rows` takes such a graph and permutes each row; the CPU
conditions on these inputs are in test_order_case_inputs.py, the GPU runs in
test_row_order_gpu.py (uniform values) and test_row_order_values_gpu.py (the value families of
parity_util.FAMILIES, FAMILY_TRIPLES below). Numpy and the host graph code only: nothing here
touches a GPU.

The case graphs are the ones the other modules build, reordered; their sizes and degrees are
unchanged (rowptr is the same array)."""
import functools

import numpy as np

import coracle
import fu
from churn_cases import chunk_edge_graph
from lossy_cases import tile_limit_graph
from pair_cases import class_graph as pair_class_graph
from pair_cases import dense66
from parity_util import (FAMILIES, FINITE_EXTRAS, NONFINITE_EXTRAS, PACK_STOPS, _batch_boundary_graph,
                         _class_edge_graph)

HOWS = ("random", "descending", "rotated", "zigzag")


def sorted_cols(rowptr, col):
    """col with every row in ascending neighbour id."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    src = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    return np.asarray(col)[np.lexsort((np.asarray(col), src))]


def reorder_cols(rowptr, col, how, seed=0):
    """col with every row permuted by `how` (the rows as sets, and rowptr, unchanged):
    "random": a seeded permutation per row; "descending"; "rotated": ascending, rotated by
    deg // 2 (np.roll), so the smallest id stands mid-row and every chunk boundary falls inside
    a monotone run; "zigzag": smallest, largest, second smallest, second largest, ..., the
    largest column jump between consecutive slots."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n, E = len(rowptr) - 1, int(rowptr[-1])
    deg = np.diff(rowptr)
    src = np.repeat(np.arange(n, dtype=np.int64), deg)
    asc = sorted_cols(rowptr, col)
    p = np.arange(E, dtype=np.int64) - rowptr[src]  # position in the row
    d = deg[src]
    if how == "random":
        key = np.random.default_rng(seed).random(E)
        return np.ascontiguousarray(asc[np.lexsort((key, src))], dtype=np.int32)
    if how == "descending":
        rank = d - 1 - p
    elif how == "rotated":
        rank = (p - d // 2) % np.maximum(d, 1)
    elif how == "zigzag":
        rank = np.where(p % 2 == 0, p // 2, d - 1 - p // 2)
    else:
        raise KeyError(how)
    return np.ascontiguousarray(asc[rowptr[src] + rank], dtype=np.int32)


def reorder_rows(g, how, seed=0):
    """fu.Graph.from_csr(rowptr, col'): the same graph and the same rowptr, each row permuted."""
    return fu.Graph.from_csr(g.rowptr, reorder_cols(g.rowptr, g.col, how, seed))


def slot_map(g_from, g_to):
    """m with g_to's slot m[k] the same directed edge (i -> j) as g_from's slot k (two orders of
    one graph; rows hold a neighbour once)."""
    n = g_from.n
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(g_from.rowptr))
    assert np.array_equal(g_from.rowptr, g_to.rowptr)
    o_from = np.lexsort((g_from.col, src))
    o_to = np.lexsort((g_to.col, src))
    assert np.array_equal(g_from.col[o_from], g_to.col[o_to])
    m = np.empty(g_from.E, dtype=np.int64)
    m[o_from] = o_to
    return m


def is_ascending(rowptr, col):
    """bool per row: strictly ascending neighbour ids (rows of 0 and 1 slots are)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(rowptr) - 1
    if len(col) < 2:
        return np.ones(n, dtype=bool)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    bad = (src[1:] == src[:-1]) & (col[1:] <= col[:-1])
    out = np.ones(n, dtype=bool)
    out[src[1:][bad]] = False
    return out


# ------------------------------------------------------------------------------------
# the case graphs, ascending as their builders return them
# ------------------------------------------------------------------------------------
MEGA_HUB = 300           # the lowered mega_hub of the R-MAT cases
RMAT_SMALL = (9, 8, 4)   # scale, edge factor, seed: the size of the recording rmat9_ef8
RMAT_LARGE = (12, 16, 4)  # the graph of test_first_rounds_flows_each_round


@functools.lru_cache(maxsize=None)
def c16_graph():
    """The graph of test_c16_narrow_and_wide_tiles_bitwise, restated: RGG(60000, 8), ER(20000,
    80000) behind it and three long-range links. The blocks that hold an end of such a link are
    the wide ones (c16_blocks; the ER part spans 20000 ids, so its blocks are narrow too, with
    offsets over most of the window)."""
    a = fu.Graph.random_geometric(60_000, avg_deg=8, seed=8)
    b = fu.Graph.erdos_renyi(20_000, 80_000, seed=8)
    src = [np.repeat(np.arange(a.n), np.diff(a.rowptr)), np.repeat(np.arange(b.n), np.diff(b.rowptr)) + a.n]
    dst = [np.asarray(a.col, dtype=np.int64), np.asarray(b.col, dtype=np.int64) + a.n]
    far = np.array(C16_FAR, dtype=np.int64)
    return fu.Graph.from_edges(a.n + b.n, np.concatenate(src + [far[:, 0], far[:, 1]]),
                               np.concatenate(dst + [far[:, 1], far[:, 0]]))


C16_FAR = ((5, 45_000), (100, 79_000), (30_000, 70_123))
C16_BLOCK = 1024  # fu_plan.h kR0E


def c16_blocks(rowptr, col):
    """(narrow, base): per 1024-slot block whether every column lies within [-32768, 32767] of
    the block's first row (FP::build_blocks), and that row: the blocks whose slots kernel 4
    reads as 2-byte offsets."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    E = int(rowptr[-1])
    nblk = -(-E // C16_BLOCK)
    first = np.arange(nblk, dtype=np.int64) * C16_BLOCK
    base = np.searchsorted(rowptr, first, side="right") - 1  # the last row with rowptr[i] <= k
    off = col - np.repeat(base, C16_BLOCK)[:E] + 32768
    ok = (off >= 0) & (off <= 65535)
    narrow = np.logical_and.reduceat(ok, first)
    return narrow, base


def _dist_graph(name):
    from dist_cases import case

    return case(name).g


# name -> builder of the ascending graph
GRAPHS = {
    "class_edge": lambda: _class_edge_graph(7),
    "rmat_small": lambda: fu.Graph.rmat(RMAT_SMALL[0], RMAT_SMALL[1], seed=RMAT_SMALL[2]),
    "rmat_large": lambda: fu.Graph.rmat(RMAT_LARGE[0], RMAT_LARGE[1], seed=RMAT_LARGE[2]),
    "c16": c16_graph,
    "batch_boundary": _batch_boundary_graph,
    "tile_limit": tile_limit_graph,
    "chunk_edge": chunk_edge_graph,
    "pair_class": pair_class_graph,
    "dense66": dense66,
    "cut_slivers": lambda: _dist_graph("slivers_w8"),
    "cut_rmat": lambda: _dist_graph("rmat_w8_hub_ranks"),
    "pack_er": lambda: fu.Graph.erdos_renyi(20_000, 80_000, seed=1),  # parity_util._width_graph
}

# The seeds the sensitivity test of test_order_case_inputs.py fixed: the per-row permutation
# of how = "random" (the other orders take no seed) and fu.uniform_values' seed per case.
# Seed 3 was tried first everywhere; it left the centre of degree 4 of batch_boundary, one row of
# 338 slots of rmat_large and the first row of rr3 of tile_limit with the ascending order's bits
# and the first row of 3 slots of pack_er with the ascending order's bits at every stop, so these
# four cases moved to the next seed at which every named row differs.
REORDER_SEED = 1
VALUE_SEED = {**{name: 3 for name in GRAPHS}, "batch_boundary": 4, "rmat_large": 5, "tile_limit": 6, "pack_er": 4}

# The seeds of the value families, keyed (case, family), fixed the same way: seed 3 first, then
# 4, 5, ... up to 12, the first at which the family's conditions of test_order_case_inputs.py
# hold for every order of GPU_HOWS. Seed 3 holds but for:
#   wide  batch_boundary 5: at 3 the centres of degree 13 (random) and 17 (rotated), at 4 those of
#         degree 4, 8, 12 and 13 (rotated) keep the ascending order's estimate at every stop;
#         pair_class 4: at 3 the centre of degree 7 keeps its estimate under "descending".
#   subn  c16 4 and pack_er 4: at 3 no named row reaches -0.0.
#   huge  rmat_small 5: at 3 and 4 its one named row (221 slots) ends in the ascending order's
#         bits and class; c16 4: at 3 no named row differs under "rotated"; dense66 11: the first
#         seed at which one of its two named rows changes class (zigzag); cut_slivers 7: likewise
#         (3 to 6: no first row of a rank changes class).
#   sym   pack_er 6: at 3 the plan's rule wavers between 16 and 8 bits from round 292 to 328, at 4
#         and 5 it stays at 16 bits to round 328 (the mean is near zero, where the keys are sparse),
#         so the last stop of parity_util.PACK_STOPS would not find the 8-bit table.
# HUGE_BITWISE_ONLY: no seed from 3 to 12 makes a named row of these cases change class (their
# named rows have 8 to 22 slots and stay finite or meet the same infinity in either order);
# they run `huge` under the bitwise condition and the whole-graph class condition only.
VALUE_SEED.update({(name, family): 3 for name in GRAPHS for family in FAMILIES})
VALUE_SEED.update({("batch_boundary", "wide"): 5, ("pair_class", "wide"): 4, ("c16", "subn"): 4, ("pack_er", "subn"): 4,
                   ("rmat_small", "huge"): 5, ("c16", "huge"): 4, ("dense66", "huge"): 11, ("cut_slivers", "huge"): 7,
                   ("pack_er", "sym"): 6})
HUGE_BITWISE_ONLY = ("c16", "pack_er")

# The rounds in total at which the GPU tests read estimates and flows back.
STOPS = {
    "class_edge": (1, 3, 8, 17),
    "rmat_small": (1, 2, 3, 5, 12),
    "rmat_large": (1, 2, 3, 5, 12),
    "c16": (2, 25),
    "batch_boundary": (1, 2, 3, 8),
    "tile_limit": (1, 2, 3, 6),
    "chunk_edge": (1, 2, 3, 6),
    "pair_class": (2, 8),
    "dense66": (2, 8),
    "cut_slivers": (1, 2, 3, 4, 7, 20),
    "cut_rmat": (1, 2, 3, 4, 7, 20),
    "pack_er": (2, 9),  # and, on the GPU, wherever the packed table reaches 8 bits
}

# (case, how) pairs that the GPU tests run: the sensitivity test covers exactly these
GPU_HOWS = {
    "class_edge": ("random", "zigzag"),
    "rmat_small": ("random", "descending"),
    "rmat_large": ("random", "zigzag"),
    "c16": ("rotated", "zigzag"),
    "batch_boundary": ("random", "rotated"),
    "tile_limit": ("random", "zigzag"),
    "chunk_edge": ("random", "rotated"),
    "pair_class": ("random", "descending"),
    "dense66": ("random", "zigzag"),
    "cut_slivers": ("random", "zigzag"),
    "cut_rmat": ("random", "descending"),
    "pack_er": ("random",),
}

# The value families of parity_util.FAMILIES that the GPU tests run on reordered rows, per case,
# beside the uniform values above: the one table that test_order_case_inputs.py (the CPU
# conditions) and test_row_order_values_gpu.py (the runs) both parametrize from.
ORDER_FAMILIES = ("wide", "huge", "subn")
PACK_FAMILIES = ("neg", "sym", "binade")  # the families whose table packs down to 8 bits
GPU_FAMILIES = {name: ORDER_FAMILIES + (PACK_FAMILIES if name == "pack_er" else ()) for name in GRAPHS}
FAMILY_TRIPLES = [(name, how, family) for name in GRAPHS for how in GPU_HOWS[name] for family in GPU_FAMILIES[name]]

# `huge` stops early: once NaN has spread over a component every order agrees (NaN against NaN
# is no difference), so a late stop detects nothing; one later stop stays, the case's last.
STOPS_BY_FAMILY = {"huge": {name: tuple(sorted({1, 2, 3, STOPS[name][-1]})) for name in GRAPHS}}


@functools.lru_cache(maxsize=None)
def base_graph(name):
    """The case graph with ascending rows: as built, but for cut_rmat, whose builder relabels an
    R-MAT by degree and so leaves its rows in the old ids' order; there the rows are sorted."""
    g = GRAPHS[name]()
    if name == "cut_rmat":
        assert not is_ascending(g.rowptr, g.col).all()
        g = fu.Graph.from_csr(g.rowptr, sorted_cols(g.rowptr, g.col))
    return g


@functools.lru_cache(maxsize=None)
def graph(name, how):
    """The case graph `name` with its rows reordered by `how`."""
    return reorder_rows(base_graph(name), how, REORDER_SEED)


@functools.lru_cache(maxsize=None)
def values(name, family="uniform"):
    """The case's values: fu.uniform_values, or a family of parity_util.FAMILIES, at the seed
    VALUE_SEED fixes for (case, family)."""
    n = base_graph(name).n
    if family == "uniform":
        v = fu.uniform_values(n, seed=VALUE_SEED[name])
    else:
        v = FAMILIES[family](n, seed=VALUE_SEED[name, family])
    v.setflags(write=False)
    return v


def stops(name, family="uniform"):
    """The rounds in total at which the GPU tests of (case, family) read back."""
    return STOPS_BY_FAMILY.get(family, STOPS)[name]


@functools.lru_cache(maxsize=None)
def reference(name, how, stops_=None, family="uniform"):
    """{stop: (a, f)} of coracle.ca_sync on the reordered graph, computed once per case and
    family and shared (read-only) by the tests. how = None: the ascending graph."""
    g = base_graph(name) if how is None else graph(name, how)
    v = values(name, family)
    out, done, a, f = {}, 0, None, None
    for stop in stops_ or stops(name, family):
        if a is None:
            a, f = coracle.ca_sync(*g.arrays(), v, stop, nthreads=8)
        else:
            coracle.ca_rounds(*g.arrays(), v, stop - done, a, f, nthreads=8)
        done = stop
        out[stop] = (a.copy(), f.copy())
        for x in out[stop]:
            x.setflags(write=False)
    return out


def named_rows(name):
    """{row: why}: the rows the sensitivity test names. The star centres of the class graphs
    (every row class's first and last degree); every row above 128 slots (the heavy rows of the
    main, lossy and churn engines) on the chunk, tile, R-MAT and cut graphs; the first rows of
    the regular segments of the tile graph; the ends of the long-range links of the c16 graph;
    the first row of every rank of the slivers cut; two rows of the circulant graph."""
    g = base_graph(name)
    deg = g.degrees
    rows = {}
    if name in ("chunk_edge", "tile_limit", "rmat_small", "rmat_large", "cut_rmat"):
        for i in np.flatnonzero(deg > 128):
            rows[int(i)] = f"heavy row of degree {int(deg[i])}"
    if name == "tile_limit":
        from lossy_cases import tile_segment

        for seg in ("rr3", "rr8"):
            rows[tile_segment(seg)[0]] = f"first row of {seg}"
    if name == "c16":
        for link in C16_FAR:
            for i in link:
                rows[i] = f"end of the long-range link {link}"
    if name == "cut_slivers":
        for lo in cut_bounds(name, 8)[:-1]:
            rows[int(lo)] = f"first row of the rank at {int(lo)}"
    if name == "dense66":
        rows = {0: "row 0", g.n // 2: "row n / 2"}
    if name == "pack_er":
        rows = {int(np.argmax(deg)): "the longest row", int(np.flatnonzero(deg >= 3)[0]): "the first row of 3 or more slots"}
    if name == "class_edge":
        from parity_util import CLASS_EDGE_DEGREES as degs
    elif name == "batch_boundary":
        from parity_util import BATCH_BOUNDARY_DEGREES as degs
    elif name == "pair_class":
        from pair_cases import CLASS_DEGREES as degs
    else:
        degs = ()
    for c, d in enumerate(degs):
        assert int(deg[c]) == d
        rows[c] = f"centre of degree {d}"
    return rows


def _differs(x, y):
    """assert_same_bits' rule, element by element: NaN against NaN is no difference."""
    xn, yn = np.isnan(x), np.isnan(y)
    bits = lambda z: np.ascontiguousarray(z).view(np.uint64)  # noqa: E731
    return (xn != yn) | (~(xn | yn) & (bits(x) != bits(y)))


def differing_rows(name, how, family="uniform"):
    """(estimate differs, some flow differs): bool per row, true where the C oracle on the
    reordered graph and on the ascending one differ, slot for slot, at one of the stops of
    (case, family) at least (the GPU tests compare at every stop). A difference is judged as
    parity_util.assert_same_bits judges it."""
    g, base = graph(name, how), base_graph(name)
    got, asc = reference(name, how, None, family), reference(name, None, None, family)
    m = slot_map(g, base)
    src = np.repeat(np.arange(g.n), base.degrees)
    da, df = np.zeros(g.n, dtype=bool), np.zeros(g.n, dtype=bool)
    for stop in stops(name, family):
        da |= _differs(got[stop][0], asc[stop][0])
        df[src[_differs(got[stop][1], asc[stop][1][m])]] = True
    return da, df


def value_class(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN, per element."""
    x = np.asarray(x)
    return np.where(np.isnan(x), 3, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 0)))


def class_changing_rows(name, how, family="huge"):
    """bool per row: the row's estimate, or one of its flows, is of another class (finite, +inf,
    -inf, NaN) on the reordered graph than on the ascending one at one of the stops."""
    g, base = graph(name, how), base_graph(name)
    got, asc = reference(name, how, None, family), reference(name, None, None, family)
    m = slot_map(g, base)
    src = np.repeat(np.arange(g.n), base.degrees)
    out = np.zeros(g.n, dtype=bool)
    for stop in stops(name, family):
        out |= value_class(got[stop][0]) != value_class(asc[stop][0])
        out[src[value_class(got[stop][1]) != value_class(asc[stop][1][m])]] = True
    return out


def neg_zero_rows(name, how, family="subn"):
    """bool per row: the reordered oracle holds -0.0 in the row's estimate or in one of its
    flows at one of the stops."""
    g = graph(name, how)
    got = reference(name, how, None, family)
    src = np.repeat(np.arange(g.n), g.degrees)
    nz = lambda x: np.ascontiguousarray(x).view(np.uint64) == np.uint64(1 << 63)  # noqa: E731
    out = np.zeros(g.n, dtype=bool)
    for stop in stops(name, family):
        out |= nz(got[stop][0])
        out[src[nz(got[stop][1])]] = True
    return out


EXEMPT_DEGREES = (0, 1, 2)  # one order only (0, 1), or a sum of two terms, which commutes (2)


# ------------------------------------------------------------------------------------
# the partition cases: uneven cuts of two dist_cases graphs at worlds 2, 3 and 8
# ------------------------------------------------------------------------------------
def cut_bounds(name, world):
    """Uneven bounds. cut_slivers (RGG 20000): leading ranks of 65, or 2 and 257, rows; at world
    8 the case's own slivers. cut_rmat (R-MAT 11 by descending degree, hub_threshold 32,
    mega_hub 256): the hubs alone on the leading ranks; at world 8 the case's own bounds."""
    from dist_cases import case

    c = case({"cut_slivers": "slivers_w8", "cut_rmat": "rmat_w8_hub_ranks"}[name])
    n = c.g.n
    if world == 8:
        return np.array(c.bounds)
    if name == "cut_slivers":
        return np.array({2: [0, 65, n], 3: [0, 2, 259, n]}[world], dtype=np.int64)
    return np.array({2: [0, 40, n], 3: [0, 8, 300, n]}[world], dtype=np.int64)


def cut_options(name):
    from dist_cases import RMAT_HUB, RMAT_MEGA

    return {"hub_threshold": RMAT_HUB, "mega_hub": RMAT_MEGA} if name == "cut_rmat" else {}


# ------------------------------------------------------------------------------------
# pack_er with the packing families: small components beside it, behind the escape code
# ------------------------------------------------------------------------------------
def with_components(g, v, extras):
    """g with its rows as they are and v, plus one small component per entry of `extras` (a
    pair, or three nodes closed to a triangle, as test_value_domain._giant_with_extras adds
    them) carrying that entry's values; the new rows follow g's."""
    rp, col, val, k = [np.asarray(g.rowptr, dtype=np.int64)], [np.asarray(g.col, dtype=np.int32)], [np.asarray(v)], g.n
    end = int(g.rowptr[-1])
    for comp in extras:
        m = len(comp)
        assert m in (2, 3)
        rows = [[k + 1], [k]] if m == 2 else [[k + 2, k + 1], [k, k + 2], [k + 1, k]]
        for row in rows:
            col.append(np.array(row, dtype=np.int32))
            end += len(row)
            rp.append(np.array([end], dtype=np.int64))
        val.append(np.array(comp, dtype=np.float64))
        k += m
    return fu.Graph.from_csr(np.concatenate(rp), np.concatenate(col)), np.concatenate(val)


@functools.lru_cache(maxsize=None)
def pack_graph(family, extras="nonfinite"):
    """(g, v): pack_er with shuffled rows and the family's values, and beside it the components
    of parity_util.NONFINITE_EXTRAS (or FINITE_EXTRAS): +-inf, NaN, -0.0, +-5e-324 and
    1.7e308, which never enter the packed window."""
    g, v = with_components(graph("pack_er", "random"), values("pack_er", family),
                           {"nonfinite": NONFINITE_EXTRAS, "finite": FINITE_EXTRAS, "signed_zero": SIGNED_ZERO_EXTRAS}[extras])
    v.setflags(write=False)
    return g, v


# A pair and a triangle of subnormals whose estimates keep returning to -0.0 (with period 2 and
# 3) while a flow and the node's own estimate sum to -0.0: there (F + a) - E is -0.0 for E = +0.0
# and +0.0 for E = -0.0, so the sign of a gathered zero shows in the flows for as long as the
# rounds go on (test_signed_zero_extras_show_the_sign_of_a_gathered_zero). Elsewhere T = 0.0 + E..
# absorbs it, which is why the components of test_value_domain.py do not show it.
SIGNED_ZERO_EXTRAS = [(-5e-324, -5e-324), (5e-324, -5e-324, -1.5e-323)]


def pack_stops(family, extras="nonfinite"):
    """The case's stops, then parity_util.PACK_STOPS: the table at 32, 16 and 8 bits; with
    the signed-zero components one and two rounds more, for their periods."""
    last = PACK_STOPS[family][-1]
    return STOPS["pack_er"] + PACK_STOPS[family] + ((last + 1, last + 2) if extras == "signed_zero" else ())


PACK_SETTLED = 8  # rounds before a stop over which the plan's rule gives the stop's width already


@functools.lru_cache(maxsize=None)
def pack_reference(family, extras="nonfinite"):
    """{rounds: (a, f)} of the oracle on pack_graph at pack_stops and PACK_SETTLED rounds
    before each packing stop, computed once and shared read-only."""
    g, v = pack_graph(family, extras)
    at = sorted(set(pack_stops(family, extras)) | {r - PACK_SETTLED for r in PACK_STOPS[family]})
    out, done, a, f = {}, 0, None, None
    for r in at:
        if a is None:
            a, f = coracle.ca_sync(*g.arrays(), v, r, nthreads=8)
        else:
            coracle.ca_rounds(*g.arrays(), v, r - done, a, f, nthreads=8)
        done = r
        out[r] = (a.copy(), f.copy())
        for x in out[r]:
            x.setflags(write=False)
    return out


STRADDLE_STEPS = (8, 16, 24, 32)


@functools.lru_cache(maxsize=None)
def straddle_values():
    """Mixed-sign subnormals on pack_er at the seed of
    test_value_domain.test_packing_window_straddles_signed_zero: the first plan packs to 8 bits
    with both zeros inside the window."""
    v = FAMILIES["subn"](base_graph("pack_er").n, seed=1)
    v.setflags(write=False)
    return v
