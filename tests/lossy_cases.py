"""Shared by the lossy-engine tests (fu.CollectAllLossy): three restatements of the lossy
synchronous round that do not run the engine.

(a) `lossy_trace` / `oracle_lossy`: the round as a synthetic tick trace for the pinned C oracle
    (coracle.replay, events RECV / FIRE_CA): one tick per round, one task per node; a delivered
    slot is a RECV of the neighbour's message of the round before (CA:98-99), a lost one is no
    event at all, so FIRE_CA runs on the pair the node stored at its last fire (CA:117-119).
(b) `lossy_python`: the rule on Python lists and floats, for graphs of about 100 nodes; the
    values may change from round to round.
(c) `delivered_py`: the loss decision on Python ints; `delivered_np` is the same on numpy
    uint64 arrays (wrapping arithmetic) for whole rounds of large graphs.

`tile_census` restates the host's plan of light tiles (fu_lossy_create), from rowptr alone.
"""
import functools

import numpy as np

import coracle
import fu

M64 = (1 << 64) - 1
SEED = 11  # the loss seed of the GPU cases and of the conditions on their inputs
GOLDEN = 0x9E3779B97F4A7C15


# ------------------------------------------------------------------------------------
# (c) the loss hash
# ------------------------------------------------------------------------------------
def mix64_py(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def splitmix_at_py(seed, i):
    return mix64_py((seed + (i + 1) * GOLDEN) & M64)


def delivered_py(seed, r, first, count, p):
    """[1 if slot first + q is delivered in round r]: lost iff u01(splitmix_at(splitmix_at(seed,
    r), k)) < p, u01(x) = (x >> 11) * 2^-53; round 0 delivers nothing."""
    if r == 0:
        return [0] * count
    key = splitmix_at_py(seed & M64, r)
    return [0 if (splitmix_at_py(key, first + q) >> 11) * 2.0 ** -53 < p else 1 for q in range(count)]


def delivered_np(seed, r, E, p):
    """bool[E] for slots 0 .. E-1 of round r: delivered_py on uint64 arrays."""
    if r == 0:
        return np.zeros(E, dtype=bool)
    key = splitmix_at_py(seed & M64, r)
    with np.errstate(over="ignore"):
        z = np.uint64(key) + (np.arange(E, dtype=np.uint64) + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return ~(u < p)


def hashed(p, seed, E, down=None):
    """The `delivered` callable of a run at (p, seed) with an optional link mask."""
    def delivered(r):
        d = delivered_np(seed, r, E, p)
        return d if down is None else d & (np.asarray(down) == 0)
    return delivered


# ------------------------------------------------------------------------------------
# (a) the round as a trace for coracle.replay
# ------------------------------------------------------------------------------------
def lossy_trace(rowptr, col, rev, rounds, delivered):
    """tick_task_off, tasks, events, out_ids, n_msgs for coracle.replay. Message slot r * E + k
    holds what slot k's owner sent over k in round r; the receiver's slot rev[k] reads it in
    round r + 1. delivered(r) -> bool[E] says which slots of round r got their message
    (ignored for round 0, which delivers nothing)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    rev = np.asarray(rev, dtype=np.int64)
    n, E = len(rowptr) - 1, int(rowptr[-1])
    assert rounds * max(E, 1) < 2 ** 31 and len(col) == E
    deg = np.diff(rowptr)
    src = np.repeat(np.arange(n, dtype=np.int64), deg)
    local = np.arange(E, dtype=np.int64) - rowptr[src]
    tasks, events = [], []
    ev_base = 0
    for r in range(rounds):
        D = np.zeros(E, dtype=bool) if r == 0 else np.asarray(delivered(r), dtype=bool)
        assert D.shape == (E,)
        ks = np.flatnonzero(D)  # ascending: grouped by row, slot order within a row
        cnt = np.bincount(src[ks], minlength=n).astype(np.int64)
        ev_begin = ev_base + np.concatenate([[0], np.cumsum(cnt + 1)[:-1]])
        first_of_row = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        ev = np.zeros((int(cnt.sum()) + n, 4), dtype=np.int64)
        pos = ev_begin[src[ks]] - ev_base + (np.arange(len(ks)) - first_of_row[src[ks]])
        ev[pos, 0] = 0
        ev[pos, 1] = local[ks]
        ev[pos, 2] = (r - 1) * E + rev[ks]
        fire = ev_begin - ev_base + cnt
        ev[fire, 0] = 1
        ev[fire, 1] = deg
        ev[fire, 2] = r * E + rowptr[:-1]
        events.append(ev)
        tasks.append(np.stack([np.arange(n, dtype=np.int64), ev_begin, ev_begin + cnt + 1], axis=1))
        ev_base += len(ev)
    assert ev_base < 2 ** 31
    return {"tick_task_off": np.arange(rounds + 1, dtype=np.int64) * n,
            "tasks": np.concatenate(tasks).astype(np.int32),
            "events": np.concatenate(events).astype(np.int32),
            "out_ids": np.arange(rounds * E, dtype=np.int32),
            "n_msgs": rounds * E}


def oracle_lossy(rowptr, col, rev, values, rounds, delivered, snaps=()):
    """(a, f, {r: a after round r}) after `rounds` lossy rounds from zero, through the C
    oracle's replay. snaps: round indices (0-based) whose estimates to keep."""
    t = lossy_trace(rowptr, col, rev, rounds, delivered)
    last, flow, _, sn = coracle.replay(rowptr, values, t["tick_task_off"], t["tasks"], t["events"], t["out_ids"],
                                       t["n_msgs"], snap_ticks=tuple(snaps))
    return last, np.ascontiguousarray(flow, dtype=np.float64), {r: sn[r].copy() for r in snaps}


# ------------------------------------------------------------------------------------
# (b) the rule on Python floats
# ------------------------------------------------------------------------------------
def lossy_python(rowptr, col, rev, values, rounds, delivered, keep=None):
    """(a, f) after `rounds` rounds. values: one array, or a callable r -> array (the inputs of
    round r). keep: a list that gets (a, f) after every round, in order."""
    rp, col, rev = [int(x) for x in rowptr], [int(x) for x in col], [int(x) for x in rev]
    n, E = len(rp) - 1, rp[-1]
    a_old, f_old = [0.0] * n, [0.0] * E
    for r in range(rounds):
        v = [float(x) for x in (values(r) if callable(values) else values)]
        D = [False] * E if r == 0 else [bool(x) for x in delivered(r)]
        a_new, f_new = [0.0] * n, [0.0] * E
        for i in range(n):
            Fs, Es = [], []
            for k in range(rp[i], rp[i + 1]):
                if D[k]:
                    Fs.append(-f_old[rev[k]])
                    Es.append(a_old[col[k]])
                else:
                    Fs.append(f_old[k])
                    Es.append(a_old[i])
            S = T = 0.0
            for F in Fs:
                S = S + F
            for X in Es:
                T = T + X
            a = ((v[i] - S) + T) / float(len(Fs) + 1)
            a_new[i] = a
            for q, k in enumerate(range(rp[i], rp[i + 1])):
                f_new[k] = (Fs[q] + a) - Es[q]
        a_old, f_old = a_new, f_new
        if keep is not None:
            keep.append((np.array(a_old, dtype=np.float64), np.array(f_old, dtype=np.float64)))
    return np.array(a_old, dtype=np.float64), np.array(f_old, dtype=np.float64)


# ------------------------------------------------------------------------------------
# graphs
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hub60():
    """60 nodes: node 0 has 49 neighbours, the rest a sparse random graph."""
    rng = np.random.default_rng(5)
    leaves = 1 + rng.choice(59, size=49, replace=False)
    s = np.concatenate([np.zeros(49, dtype=np.int64), rng.integers(1, 60, 70)])
    d = np.concatenate([leaves, rng.integers(1, 60, 70)])
    g = fu.Graph.from_edges(60, s, d)
    assert int(g.degrees[0]) == 49 and int(g.degrees[1:].max()) < 49
    return g


# ------------------------------------------------------------------------------------
# the light tiles of fu_lossy_create, and a graph that closes them in every way
# ------------------------------------------------------------------------------------
TILE_ROWS, TILE_SLOTS, TILE_HEAVY_DEG = 256, 2048, 128


def tile_census(rowptr):
    """[(first row, end row, slots, why)] of the light tiles that fu_lossy_create plans: rows
    above degree 128 get a block each and belong to no tile; a tile takes consecutive rows
    until the graph ends ("end"), it holds 256 rows ("rows"), the next row is above degree 128
    ("heavy") or the next row would take it past 2048 slots ("slots"), tested in that order."""
    rp = [int(x) for x in rowptr]
    n = len(rp) - 1
    out, i = [], 0
    while i < n:
        if rp[i + 1] - rp[i] > TILE_HEAVY_DEG:
            i += 1
            continue
        j = i
        while True:
            if j == n:
                why = "end"
            elif j - i == TILE_ROWS:
                why = "rows"
            elif rp[j + 1] - rp[j] > TILE_HEAVY_DEG:
                why = "heavy"
            elif rp[j + 1] - rp[i] > TILE_SLOTS:
                why = "slots"
            else:
                j += 1
                continue
            break
        assert j > i  # a light row alone always fits
        out.append((i, j, rp[j] - rp[i], why))
        i = j
    return out


def _undirected(g, first):
    """The edges (i < j) of g with `first` added to every id."""
    src = np.repeat(np.arange(g.n), np.diff(g.rowptr))
    keep = src < g.col
    return first + src[keep], first + g.col[keep].astype(np.int64)


# (name, rows) in id order; the first three end on multiples of 256, so each of their tiles
# starts where a segment's rows do.
TILE_SEGMENTS = [("isolated", 256), ("rr3", 1024), ("rr8", 256), ("ring", 64), ("heavy", 1), ("er12", 1000),
                 ("isolated_tail", 40)]


def tile_segment(name):
    """(first row, rows) of a segment of tile_limit_graph()."""
    first = 0
    for s, rows in TILE_SEGMENTS:
        if s == name:
            return first, rows
        first += rows
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def tile_limit_graph():
    """2641 nodes in segments of consecutive ids: 256 isolated rows (a tile of 256 rows and no
    slot), a random 3-regular graph on 1024 rows (four tiles of 256 rows and 768 slots), a random
    8-regular graph on 256 rows (256 rows and exactly 2048 slots), a ring of 64 rows that the
    next row, of degree 129, closes, that row's neighbours being among the 1000 rows of
    ER(1000, 6000) which follow it (tiles closed by the slot limit), and 40 isolated rows at the
    end of the last tile."""
    rng = np.random.default_rng(9)
    src, dst = [], []
    for name, make in (("rr3", lambda: fu.Graph.random_regular(1024, 3, seed=2)),
                       ("rr8", lambda: fu.Graph.random_regular(256, 8, seed=1)),
                       ("er12", lambda: fu.Graph.erdos_renyi(1000, 6000, seed=4))):
        s, d = _undirected(make(), tile_segment(name)[0])
        src.append(s)
        dst.append(d)
    r0, rows = tile_segment("ring")
    src.append(r0 + np.arange(rows))
    dst.append(r0 + (np.arange(rows) + 1) % rows)
    e0, rows = tile_segment("er12")
    src.append(np.full(129, tile_segment("heavy")[0]))
    dst.append(e0 + rng.choice(rows, size=129, replace=False))
    n = sum(rows for _, rows in TILE_SEGMENTS)
    g = fu.Graph.from_edges(n, np.concatenate(src), np.concatenate(dst))
    deg = g.degrees
    for name, want in (("isolated", 0), ("rr3", 3), ("rr8", 8), ("ring", 2), ("heavy", 129), ("isolated_tail", 0)):
        first, rows = tile_segment(name)
        assert (deg[first:first + rows] == want).all(), name
    assert int(deg[e0:e0 + 1000].max()) <= TILE_HEAVY_DEG
    return g
