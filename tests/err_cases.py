"""The inputs of tests/test_err_paths.py (graphs, values, the oracle's rounds, probes and D per
case), shared with the CPU checks of their conditions in tests/test_parity_util.py. Numpy,
the host graph generators and the C oracle only: nothing here touches a GPU."""
import functools

import numpy as np

import coracle
import fu
from parity_util import (CLASS_EDGE_DEGREES, _class_edge_graph, _isolated_then_heavy_graph,
                         _isolated_then_heavy_rows, _width_graph, planted_D)


def oracle_rounds(g_arrays, v, rounds, nthreads=8):
    """(rounds, n): the C oracle's estimates a_r after each of rounds 0 .. rounds-1."""
    a, f = coracle.ca_sync(*g_arrays, v, 1, nthreads=nthreads)
    out = np.empty((rounds, len(a)))
    out[0] = a
    for r in range(1, rounds):
        coracle.ca_rounds(*g_arrays, v, 1, a, f, nthreads=nthreads)
        out[r] = a
    return out


def _unique(seq):
    return list(dict.fromkeys(int(x) for x in seq))


# ---- the inputs of tests/test_err_paths.py, shared with the CPU checks of their conditions
ERR_R = 6


@functools.lru_cache(maxsize=None)
def err_class_case():
    """Section 1: (g, v, a_rounds, probes) on the class-edge graph. Probes (caller ids): the 28
    star centres, node n-1, the first background node, 12 seeded background nodes and the
    last 5 rows of the degree order (descending, ties by id). This graph has no background node of
    degree 0 (centre 0 is its only empty row), so these stand in for them: with centre 0 they
    are the rows that the degree layout moves to the very end, as the two largest centres
    move to the front."""
    g = _class_edge_graph(7)
    v = fu.uniform_values(g.n, seed=3)
    k = len(CLASS_EDGE_DEGREES)
    rng = np.random.default_rng(17)
    zero_deg = np.argsort(-g.degrees, kind="stable")[-5:]  # the degree layout's last rows (ties by id)
    probes = _unique(list(range(k)) + [g.n - 1, k] + list(k + rng.choice(g.n - k, 12, replace=False)) + list(zero_deg))
    return g, v, oracle_rounds(g.arrays(), v, ERR_R), probes


ISO_TAILS = ("heavy_hub", "hub_iso_heavy", "iso_end")


@functools.lru_cache(maxsize=None)
def err_isolated_case(tail):
    """Section 2: (g, v, a_rounds, probes): the first, a middle and the last row of the
    isolated run, the heavy row, the mega hub and node 0."""
    g = _isolated_then_heavy_graph(tail)
    v = fu.uniform_values(g.n, seed=8)
    _, _, iso0, n_iso, heavy, hub = _isolated_then_heavy_rows(tail)
    probes = [iso0, iso0 + n_iso // 2, iso0 + n_iso - 1, heavy, hub, 0]
    return g, v, oracle_rounds(g.arrays(), v, ERR_R), probes


ERR_RMAT_HUB, ERR_RMAT_MEGA = 32, 300


@functools.lru_cache(maxsize=None)
def err_rmat_case():
    """Section 3: (g, v, a_rounds, probes) on R-MAT scale 12 with hub_threshold 32 and
    mega_hub 300: the three highest-degree rows (mega hubs), three heavy rows (degree in
    (32, 300]), the last row and 8 seeded light rows."""
    g = fu.Graph.rmat(12, 16, seed=4)
    v = fu.uniform_values(g.n, seed=4)
    deg = g.degrees
    top = np.argsort(-deg, kind="stable")[:3]
    heavy = np.nonzero((deg > ERR_RMAT_HUB) & (deg <= ERR_RMAT_MEGA))[0]
    heavy = heavy[[0, len(heavy) // 2, len(heavy) - 1]]
    light = np.nonzero(deg <= ERR_RMAT_HUB)[0]
    light = np.random.default_rng(18).choice(light, 8, replace=False)
    probes = _unique(list(top) + list(heavy) + [g.n - 1] + list(light))
    return g, v, oracle_rounds(g.arrays(), v, ERR_R), probes


ERR_DIST_R = 5
ERR_DIST_CASES = [("er", 2), ("er", 3), ("rmat", 2), ("rgg", 2), ("rgg", 3)]
ERR_DIST_HUB, ERR_DIST_MEGA = 32, 256
# (tile edges, tile nodes) of every light-tile launch: kernel 4's four geometries (fu_plan.h
# kGeoEdges / kGeoNodes; kernel 9's tiles are kernel 4's) and kernel 8's (fu_tuning.h kStageTE / TN)
LIGHT_TILE_GEOMETRIES = [(2048, 256), (1024, 128), (1024, 256), (512, 64)]
MAX_TILE_NODES = 256


def light_tiles(rowptr, te, tn, hub_threshold, mega_hub):
    """[(first row, end row)] of the light tiles, as FP::build_tiles_geom and
    FP::build_stage_light cut them: consecutive rows of degree <= min(hub_threshold, te,
    mega_hub), at most tn rows and te edges per tile; longer rows get tiles of their own."""
    deg = np.diff(rowptr)
    n, lim = len(deg), min(hub_threshold, te, mega_hub)
    out, i = [], 0
    while i < n:
        if deg[i] > lim:
            i += 1
            continue
        b = i
        while i < n and i - b < tn and deg[i] <= lim and rowptr[i + 1] - rowptr[b] <= te:
            i += 1
        out.append((b, i))
    return out


def rows_with_ghosts(plan):
    """bool per local row: the row has a ghost column."""
    src = np.repeat(np.arange(plan.n_local), np.diff(plan.rowptr))
    out = np.zeros(plan.n_local, dtype=bool)
    out[src[plan.col >= plan.n_local]] = True
    return out


def dist_thresholds(kind):
    """(hub_threshold, mega_hub) the partition cases run with: set on R-MAT, the defaults else."""
    return (ERR_DIST_HUB, ERR_DIST_MEGA) if kind == "rmat" else (128, 8192)


@functools.lru_cache(maxsize=None)
def err_dist_case(kind, world):
    """Section 4: (g, v, a_rounds, plans, probes, D, kinds). kinds[rank] maps a kind of row to
    the local row that rank plants: "first", "last", "ghost" (a light row with a ghost column:
    a boundary tile), "longest" (its highest-degree row), then
      * on ER and R-MAT, "no_ghost": a light row with no ghost column. These graphs have no
        locality, so every light tile of every rank reads a ghost and the row still sits in a
        boundary tile;
      * on R-MAT, "mega_ghost": a mega hub with ghost columns (not the longest row);
      * on the random geometric graph (rows sorted by x, so a rank is a slab and only the rows
        near its ends have ghosts), "interior": the middle of the longest run of light rows
        without ghost columns. The run is longer than 2 x 256 rows, so whatever the tile
        geometry (<= 256 rows per tile) the row's tile lies inside the run: an interior tile,
        computed by the second light launch of a partitioned round.
    probes[k][rank] is the row planted in run k (every rank plants one row of its own in every
    run, rotated so that the ranks' rows differ in kind), D[rank] its own power of two."""
    from fu.dist import partition

    if kind == "er":
        g = fu.Graph.erdos_renyi(6000, 24000, seed=21)
        v = fu.uniform_values(g.n, seed=21)
    elif kind == "rmat":
        g = fu.Graph.rmat(12, 16, seed=3)
        v = fu.uniform_values(g.n, seed=4)
    else:
        g = fu.Graph.random_geometric(8000, avg_deg=8, seed=21)
        v = fu.uniform_values(g.n, seed=21)
    hub, mega = dist_thresholds(kind)
    a_rounds = oracle_rounds(g.arrays(), v, ERR_DIST_R)
    plans = [partition(g.rowptr, g.col, g.rev, world, r) for r in range(world)]
    kinds, D = [], []
    for p in plans:
        deg = np.diff(p.rowptr)
        has_ghost = rows_with_ghosts(p)
        light = deg <= min(hub, mega)
        mine = {"first": 0, "last": p.n_local - 1,
                "ghost": int(np.nonzero(has_ghost & light)[0][int(np.count_nonzero(has_ghost & light)) // 2]),
                "longest": int(np.argmax(deg))}
        if kind == "rgg":
            inside = np.concatenate([[False], light & ~has_ghost, [False]])
            edges = np.flatnonzero(inside[1:] != inside[:-1])  # run starts and ends, alternating
            k = int(np.argmax(edges[1::2] - edges[::2]))
            assert edges[2 * k + 1] - edges[2 * k] > 2 * MAX_TILE_NODES
            mine["interior"] = int(edges[2 * k] + edges[2 * k + 1]) // 2
        else:
            mine["no_ghost"] = int(np.nonzero(~has_ghost & light & (deg > 0))[0][0])
        if kind == "rmat":
            cand = np.nonzero(has_ghost & (deg > mega))[0]
            mine["mega_ghost"] = int(cand[np.argmin(deg[cand])])
        kinds.append(mine)
        D.append(planted_D(a_rounds, shift=p.rank))  # from all rows: distinct by construction
    names = list(kinds[0])
    probes = [[kinds[q][names[(k + q) % len(names)]] for q in range(world)] for k in range(len(names))]
    return g, v, a_rounds, plans, probes, D, kinds


@functools.lru_cache(maxsize=None)
def err_rccl_case():
    """Section 4's RCCL case at one rank: (g, v, a_rounds, probes)."""
    g = fu.Graph.random_geometric(20_000, avg_deg=8, seed=3)
    v = fu.uniform_values(g.n, seed=1)
    probes = _unique([0, g.n - 1, int(np.argmax(g.degrees))])
    return g, v, oracle_rounds(g.arrays(), v, ERR_R), probes


ERR_REDUCER_R = 3
ERR_GRID = 1024  # blocks of k_max_err / kb_max_err; the rest is reached by striding


@functools.lru_cache(maxsize=None)
def err_scalar_reducer_case():
    """Section 5, fu_max_err: (g, v, a_rounds, probes, new_of_old). Probes are device indices:
    the first and last thread of block 0, the first of block 1, the last index of the first
    stride, the first of the second (grid 1024 x 256) and n-1. Under layout "degree" the test
    plants them at the caller ids they map to (new_of_old: the degree relabelling) as well as
    at these caller ids."""
    g = fu.Graph.erdos_renyi(300_000, 600_000, seed=2)
    v = fu.uniform_values(g.n, seed=2)
    assert g.n > ERR_GRID * 256
    probes = [0, 255, 256, ERR_GRID * 256 - 1, ERR_GRID * 256, g.n - 1]
    _, new_of_old = g.relabel("degree")
    return g, v, oracle_rounds(g.arrays(), v, ERR_REDUCER_R), probes, np.asarray(new_of_old, dtype=np.int64)


ERR_CHURN_DECOY = 2.0 ** 20  # a dead decoy's target sits this many D off its estimate


@functools.lru_cache(maxsize=None)
def err_churn_reducer_case():
    """Section 5, kc_max_err (fu_churn.hip): (g, v, alive, a_rounds, probes, decoys). The graph,
    values and probes of err_scalar_reducer_case under a static topology with about a tenth of
    the nodes dead (the probes kept alive), set before round 0: a_rounds is the C oracle on the
    live subgraph, and a dead node stays at 0.0. decoys: a dead node of block 0, one of the last
    block of the first stride and one of the second stride."""
    from churn_cases import compact, live_np, random_masks

    g, v, _, probes, _ = err_scalar_reducer_case()
    alive, _ = random_masks(g, 0.1, 0.0, 5, keep=probes)
    rp, col, rev, _ = compact(*g.arrays(), live_np(*g.arrays(), alive, None))
    a_rounds = oracle_rounds((rp, col, rev), v, ERR_REDUCER_R)
    a_rounds[:, alive == 0] = 0.0
    dead = np.flatnonzero(alive == 0)
    stride = ERR_GRID * 256
    decoys = [int(dead[0]), int(dead[dead >= stride - 256][0]), int(dead[dead >= stride][0])]
    return g, v, alive, a_rounds, probes, decoys


def with_decoys(t, a_last, decoys, D):
    """t with every decoy's target ERR_CHURN_DECOY * D above its estimate."""
    t = t.copy()
    t[decoys] = a_last[decoys] + ERR_CHURN_DECOY * D
    return t


ERR_BATCH_KS = (16, 7, 3)


@functools.lru_cache(maxsize=None)
def err_batch_case(K):
    """Section 5, kb_max_err: (g, vs, a_rounds per column, probes as (node, column), D per
    column). A block uses tb = (256 / K) K threads; the probes in flat index q = i K + c are 0,
    tb-1, tb, 1024 tb - 1, 1024 tb (the first of the second stride), 1024 tb + K - 1 and
    n K - 1."""
    if K == 16:
        g = _width_graph()
    elif K == 7:
        g = fu.Graph.erdos_renyi(40_000, 160_000, seed=1)
    else:
        g = fu.Graph.erdos_renyi(90_000, 360_000, seed=1)
    tb = (256 // K) * K
    assert g.n * K > ERR_GRID * tb + K
    vs = [fu.uniform_values(g.n, seed=c) for c in range(K)]
    a_rounds = [oracle_rounds(g.arrays(), v, ERR_REDUCER_R) for v in vs]
    flat = [0, tb - 1, tb, ERR_GRID * tb - 1, ERR_GRID * tb, ERR_GRID * tb + K - 1, g.n * K - 1]
    probes = [divmod(q, K) for q in flat]
    base = max(planted_D(a) for a in a_rounds)  # one base, so the columns' D are distinct
    D = [base * 2.0 ** c for c in range(K)]
    return g, vs, a_rounds, probes, D


def err_batch_nonfinite_rows():
    """Section 6, batched: (g, the highest-degree row, a row of degree 0) of the K = 7 graph."""
    g = err_batch_case(7)[0]
    deg = g.degrees
    return g, int(np.argmax(deg)), int(np.nonzero(deg == 0)[0][0])


def err_batch_trace_probes(K, n):
    """One probe node per column for the batched trace: spread over the rows, one per column."""
    return [(c * (n // K) + c) % n for c in range(K)]


def planted_conditions(case):
    """Every (a_rounds, probe, D) that tests/test_err_paths.py plants for `case`, for the CPU
    check of the uniqueness condition (planted_targets asserts it)."""
    if case == "classes":
        _, _, a, probes = err_class_case()
        return [(a, p, planted_D(a)) for p in probes]
    if case.startswith("isolated:"):
        _, _, a, probes = err_isolated_case(case.split(":")[1])
        return [(a, p, planted_D(a)) for p in probes]
    if case == "rmat":
        _, _, a, probes = err_rmat_case()
        return [(a, p, planted_D(a)) for p in probes]
    if case.startswith("dist:"):
        _, kind, world = case.split(":")
        _, _, a, plans, probes, D, _ = err_dist_case(kind, int(world))
        return [(a[:, pl.lo:pl.hi], row[pl.rank], D[pl.rank]) for row in probes for pl in plans]
    if case == "rccl":
        _, _, a, probes = err_rccl_case()
        return [(a, p, planted_D(a)) for p in probes]
    if case == "scalar_reducer":
        g, _, a, probes, new_of_old = err_scalar_reducer_case()
        old_of_new = np.argsort(new_of_old)
        return [(a, p, planted_D(a)) for p in _unique(probes + [old_of_new[q] for q in probes])]
    if case == "churn_reducer":
        _, _, _, a, probes, _ = err_churn_reducer_case()
        return [(a, p, planted_D(a)) for p in probes]
    if case.startswith("batch:"):
        K = int(case.split(":")[1])
        g, _, a, probes, D = err_batch_case(K)
        out = [(a[c], i, D[c]) for i, c in probes]
        if K == 7:
            out += [(a[c], p, D[c]) for c, p in enumerate(err_batch_trace_probes(K, g.n))]
        return out
    raise KeyError(case)


PLANTED_CASES = (["classes", "rmat", "rccl", "scalar_reducer", "churn_reducer"] + [f"isolated:{t}" for t in ISO_TAILS]
                 + [f"dist:{k}:{w}" for k, w in ERR_DIST_CASES] + [f"batch:{K}" for K in ERR_BATCH_KS])
