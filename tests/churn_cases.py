"""Shared by the churn-engine tests (fu.CollectAllChurn): the rule of the fu_churn section of
include/fu.h restated on Python lists and floats (`churn_python`; it shares no code with the
engine and does not run it), the live subgraph of a topology as a CSR of its own (`compact`),
the masks and scripts of the cases, and their graphs.

The rule. Slot k = (i -> j) is live iff link_up[k] and alive[i] and alive[j]. A topology moves a
slot live -> not live: DOWN (flow entry gone: +0.0), not live -> live: FRESH, live -> live: as it
was. Round, alive node i, row order, DOWN slots skipped: UP: F = -f_old[rev k], E = a_old[col k];
FRESH: F = E = 0.0; S = 0.0 + F.., T = 0.0 + E..; a = ((v - S) + T) / (live slots + 1);
f = (F + a) - E; a DOWN slot's flow is +0.0; FRESH becomes UP. A dead node keeps its estimate.
After create and reset: zero state, every live slot FRESH."""
import collections
import functools

import numpy as np

import coracle
import fu
from parity_util import assert_same_bits
from lossy_cases import TILE_HEAVY_DEG, TILE_ROWS, TILE_SLOTS, hub60, tile_census, tile_limit_graph, tile_segment  # noqa: F401

UP, DOWN, FRESH = 0, 1, 2
HEAVY_CHUNK = 2048  # slots of a heavy row (degree > TILE_HEAVY_DEG) staged per chunk (fu_churn.hip kChunk)
# chunk_edge_graph()'s heavy rows: the first heavy degree, one slot short of a chunk, a chunk, a chunk and one
# slot, two chunks, two chunks and one slot
CHUNK_EDGE_DEGREES = (TILE_HEAVY_DEG + 1, HEAVY_CHUNK - 1, HEAVY_CHUNK, HEAVY_CHUNK + 1, 2 * HEAVY_CHUNK, 2 * HEAVY_CHUNK + 1)

Step = collections.namedtuple("Step", "a f state alive_nodes live_slots")
Result = collections.namedtuple("Result", "a f state a_rounds f_rounds steps")


def _arr(x):
    return np.array(x, dtype=np.float64)


def churn_python(rowptr, col, rev, values, script):
    """The rule on Python lists and floats. script: a list of ("run", R), ("topology", alive,
    link_up) (None = all ones), ("values", v) and ("reset",). Returns Result(a, f, state,
    a_rounds, f_rounds, steps): the final estimates, flows and slot states (0 UP, 1 DOWN,
    2 FRESH), the estimates and flows after every round run, in order, and a Step(a, f, state,
    alive_nodes, live_slots) after every script step."""
    rp, col, rev = [int(x) for x in rowptr], [int(x) for x in col], [int(x) for x in rev]
    n, E = len(rp) - 1, rp[-1]
    v = [float(x) for x in values]
    a, f = [0.0] * n, [0.0] * E
    alive, state = [True] * n, [FRESH] * E
    a_rounds, f_rounds, steps = [], [], []
    for step in script:
        if step[0] == "run":
            for _ in range(step[1]):
                a_new, f_new = list(a), [0.0] * E
                for i in range(n):
                    if not alive[i]:
                        continue
                    ks = [k for k in range(rp[i], rp[i + 1]) if state[k] != DOWN]
                    Fs = [-f[rev[k]] if state[k] == UP else 0.0 for k in ks]
                    Es = [a[col[k]] if state[k] == UP else 0.0 for k in ks]
                    S = T = 0.0
                    for F in Fs:
                        S = S + F
                    for X in Es:
                        T = T + X
                    a_new[i] = ((v[i] - S) + T) / float(len(ks) + 1)
                    for q, k in enumerate(ks):
                        f_new[k] = (Fs[q] + a_new[i]) - Es[q]
                a, f = a_new, f_new
                state = [UP if s == FRESH else s for s in state]
                a_rounds.append(_arr(a))
                f_rounds.append(_arr(f))
        elif step[0] == "topology":
            alive = [True] * n if step[1] is None else [bool(x) for x in step[1]]
            up = [True] * E if step[2] is None else [bool(x) for x in step[2]]
            assert len(alive) == n and len(up) == E and all(up[k] == up[rev[k]] for k in range(E))
            for i in range(n):
                for k in range(rp[i], rp[i + 1]):
                    if up[k] and alive[i] and alive[col[k]]:
                        if state[k] == DOWN:
                            state[k] = FRESH
                    else:
                        state[k] = DOWN
                        f[k] = 0.0
        elif step[0] == "values":
            v = [float(x) for x in step[1]]
            assert len(v) == n
        elif step[0] == "reset":
            a, f = [0.0] * n, [0.0] * E
            state = [DOWN if s == DOWN else FRESH for s in state]
        else:
            raise ValueError(step[0])
        steps.append(Step(_arr(a), _arr(f), np.array(state, dtype=np.uint8), sum(alive), sum(s != DOWN for s in state)))
    return Result(_arr(a), _arr(f), np.array(state, dtype=np.uint8), a_rounds, f_rounds, steps)


def live_np(rowptr, col, rev, alive=None, link_up=None):
    """bool[E]: the liveness rule in numpy."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n, E = len(rowptr) - 1, int(rowptr[-1])
    src = np.repeat(np.arange(n), np.diff(rowptr))
    alive = np.ones(n, dtype=bool) if alive is None else np.asarray(alive) != 0
    up = np.ones(E, dtype=bool) if link_up is None else np.asarray(link_up) != 0
    return up & alive[src] & alive[np.asarray(col)]


def compact(rowptr, col, rev, live):
    """The live subgraph on the same n nodes: (rowptr, col, rev, kmap) with the live slots only,
    row order kept; compact slot q is the caller's slot kmap[q]. A node without a live slot (a
    dead one among them) is an isolated row."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    live = np.asarray(live, dtype=bool)
    n, E = len(rowptr) - 1, int(rowptr[-1])
    assert live.shape == (E,) and np.array_equal(live, live[np.asarray(rev)])
    src = np.repeat(np.arange(n), np.diff(rowptr))
    kmap = np.flatnonzero(live)
    pos = np.full(E, -1, dtype=np.int64)
    pos[kmap] = np.arange(len(kmap))
    rp = np.concatenate([[0], np.cumsum(np.bincount(src[kmap], minlength=n))]).astype(np.int64)
    return rp, np.asarray(col)[kmap].astype(np.int32), pos[np.asarray(rev)[kmap]].astype(np.int32), kmap


def check_static(g, alive, up, v, got_a, got_f, got_state, rounds, what):
    """(a, f, state) after `rounds` rounds under a topology set before round 0: ca_sync on the
    live subgraph for the alive nodes and the live slots, +0.0 on the DOWN slots, 0.0 on the dead
    nodes."""
    live = live_np(*g.arrays(), alive, up)
    rp, col, rev, kmap = compact(*g.arrays(), live)
    a, f = coracle.ca_sync(rp, col, rev, v, rounds)
    on = np.asarray(alive) != 0
    assert_same_bits(got_a[on], a[on], what + ("alive estimates",))
    assert_same_bits(got_a[~on], np.zeros(int((~on).sum())), what + ("dead estimates",))
    assert_same_bits(got_f[kmap], f, what + ("live flows",))
    assert_same_bits(got_f[~live], np.zeros(int((~live).sum())), what + ("down flows",))
    assert np.array_equal(got_state, np.where(live, UP if rounds else FRESH, DOWN))


# ------------------------------------------------------------------------------------
# graphs and masks
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def star(leaves):
    """Node 0 with `leaves` leaves: star(2100)'s hub row spans two heavy chunks."""
    return fu.Graph.from_edges(leaves + 1, np.zeros(leaves, dtype=np.int64), 1 + np.arange(leaves))


def cut(g, link_up, slots):
    """link_up with the links of `slots` (and their reverse slots) down."""
    link_up = np.array(link_up, dtype=np.uint8)
    slots = np.asarray(slots, dtype=np.int64)
    link_up[slots] = 0
    link_up[g.rev[slots]] = 0
    return link_up


def random_masks(g, dead_frac, cut_frac, seed, keep=()):
    """(alive, link_up): about dead_frac of the nodes dead (never one of `keep`) and about
    cut_frac of the undirected links down."""
    rng = np.random.default_rng(seed)
    alive = (rng.random(g.n) >= dead_frac).astype(np.uint8)
    alive[list(keep)] = 1
    one = np.flatnonzero(np.arange(g.E) < g.rev)  # one slot per undirected link
    return alive, cut(g, np.ones(g.E, dtype=np.uint8), one[rng.random(len(one)) < cut_frac])


def heavy_rows(g):
    return [int(i) for i in np.flatnonzero(g.degrees > TILE_HEAVY_DEG)]


def row_slots(g, i):
    return np.arange(g.rowptr[i], g.rowptr[i + 1])


def scripted_run(g, seed, values2):
    """The script of the scripted GPU cases on g, whose busiest row (hub60's hub, the heavy row of
    tile_limit_graph) stays alive throughout: run(6); kill a fifth of the nodes and cut a tenth of
    the links, four of the busiest row's among them; run(1); revive half of the dead and restore
    half of the cut links; run(1); new values; run(5); a topology with other nodes dead and
    other links down, at once followed by everything on again (UP -> DOWN -> FRESH, the flow
    dropped); run(4); reset; run(3)."""
    hub = int(np.argmax(g.degrees))
    hs = row_slots(g, hub)
    alive1, up1 = random_masks(g, 0.2, 0.1, seed, keep=(hub,))
    up1 = cut(g, up1, hs[[0, len(hs) // 3, len(hs) // 2, len(hs) - 1]])
    dead = np.flatnonzero(alive1 == 0)
    alive2 = alive1.copy()
    alive2[dead[::2]] = 1
    down = np.flatnonzero((up1 == 0) & (np.arange(g.E) < g.rev))
    up2 = np.ones(g.E, dtype=np.uint8)
    up2 = cut(g, up2, down[1::2])
    alive3, up3 = random_masks(g, 0.15, 0.15, seed + 1, keep=(hub,))
    alive3 &= alive2  # what is dead stays dead over the double call
    up3 &= up2
    assert len(dead) >= 2 and len(down) >= 2
    return [("run", 6), ("topology", alive1, up1), ("run", 1), ("topology", alive2, up2), ("run", 1), ("values", values2),
            ("run", 5), ("topology", alive3, up3), ("topology", alive2, up2), ("run", 4), ("reset",), ("run", 3)]


# ------------------------------------------------------------------------------------
# heavy rows at the chunk edges
# ------------------------------------------------------------------------------------
CHUNK_EDGE_ORDER = (2049, 4096, 4097, 2048, 2047, 129)  # by id: the first three rows, the middle one, the last two
CHUNK_EDGE_CHAIN = 4  # every 4th leaf is linked to the next leaf


@functools.lru_cache(maxsize=None)
def chunk_edge_graph():
    """Six heavy rows of the degrees CHUNK_EDGE_DEGREES, pairwise linked, the rest of each row's
    degree leaves of its own (14636 leaves, taken in id order row after row), and every 4th leaf
    linked to the next one so that the light tiles hold slots whose two ends are both light. Ids:
    heavy rows at 0, 1, 2 (the first tile starts after three adjacent heavy rows), one between
    the two halves of the leaves (it closes a tile), two at n-2 and n-1 (no tile after the last
    row). A row's slots are in ascending neighbour id, so a heavy row's heavy-heavy slots are
    its first ones, the one to the middle row, and its last ones."""
    assert sorted(CHUNK_EDGE_ORDER) == list(CHUNK_EDGE_DEGREES)
    k = len(CHUNK_EDGE_ORDER)
    n_leaf = sum(CHUNK_EDGE_ORDER) - k * (k - 1)
    n = k + n_leaf
    heavy = [0, 1, 2, 3 + n_leaf // 2, n - 2, n - 1]
    leaves = np.setdiff1d(np.arange(n), heavy)
    src = [np.array([heavy[p] for p in range(k) for q in range(p + 1, k)])]
    dst = [np.array([heavy[q] for p in range(k) for q in range(p + 1, k)])]
    first = 0
    for h, d in zip(heavy, CHUNK_EDGE_ORDER):
        src.append(np.full(d - (k - 1), h))
        dst.append(leaves[first:first + d - (k - 1)])
        first += d - (k - 1)
    assert first == n_leaf
    src.append(leaves[:-1:CHUNK_EDGE_CHAIN])
    dst.append(leaves[1::CHUNK_EDGE_CHAIN])
    g = fu.Graph.from_edges(n, np.concatenate(src), np.concatenate(dst))
    assert [int(g.degrees[h]) for h in heavy] == list(CHUNK_EDGE_ORDER) and heavy_rows(g) == heavy
    return g


def chunk_edge_rows():
    """{degree: id} of chunk_edge_graph()'s heavy rows."""
    g = chunk_edge_graph()
    return {int(g.degrees[h]): h for h in heavy_rows(g)}


@functools.lru_cache(maxsize=None)
def chunk_edge_topology(which):
    """(alive, link_up) on chunk_edge_graph(): about a tenth of the leaves dead and a twentieth of
    the links down (the heavy rows kept alive), and on top, slots picked by their position in
    the row:
      "A": on the rows above one chunk (2049, 4096, 4097) slots 0, 2047, 2048 and d-1 DOWN; the
           2048 row alive with every link cut; the 2047 row dead, all its neighbours alive;
      "B": slot 2048 the only live slot of the 2049 row; the second chunk of the 4096 row (slots
           2048 .. 4095) DOWN;
      "C": slot 2048 the only DOWN slot of the 2049 row; the middle chunk of the 4097 row DOWN.
    tests/test_churn_case_inputs.py asserts each of these on the masks."""
    g = chunk_edge_graph()
    row = chunk_edge_rows()
    alive, up = random_masks(g, 0.1, 0.05, 30 + "ABC".index(which), keep=heavy_rows(g))
    c = HEAVY_CHUNK
    if which == "A":
        for d in (2049, 4096, 4097):
            up = cut(g, up, row_slots(g, row[d])[[0, c - 1, c, d - 1]])
        up = cut(g, up, row_slots(g, row[2048]))
        alive[g.col[row_slots(g, row[2047])]] = 1
        alive[row[2047]] = 0
    elif which == "B":
        hs = row_slots(g, row[2049])
        up = cut(g, up, np.delete(hs, c))
        alive[g.col[hs[c]]] = 1
        up[[hs[c], g.rev[hs[c]]]] = 1
        up = cut(g, up, row_slots(g, row[4096])[c:2 * c])
    else:
        up = cut(g, up, row_slots(g, row[4097])[c:2 * c])
        hs = row_slots(g, row[2049])
        alive[g.col[hs]] = 1
        up[hs] = 1
        up[g.rev[hs]] = 1
        up = cut(g, up, hs[[c]])
    alive.setflags(write=False)
    up.setflags(write=False)
    return alive, up


def chunk_edge_values(family):
    """The inputs of the chunk-edge cases. "special" plants -0.0, +inf and -inf on three leaves of
    the 4097 row that stay alive and linked throughout the script (the row's T chain reaches
    inf - inf in round 1) and a NaN on such a leaf of the 4096 row; "subn" is parity_util's."""
    from parity_util import FAMILIES

    g = chunk_edge_graph()
    if family == "uniform":
        return fu.uniform_values(g.n, seed=3)
    if family == "subn":
        return FAMILIES["subn"](g.n, 4)
    assert family == "special"
    v = fu.uniform_values(g.n, seed=3)
    alive, up = chunk_edge_topology("A")
    live = live_np(*g.arrays(), alive, up)
    row = chunk_edge_rows()
    hs = row_slots(g, row[4097])
    ok = hs[live[hs] & (g.degrees[g.col[hs]] <= 2)]
    v[g.col[ok[[10, len(ok) // 2, len(ok) - 10]]]] = [-0.0, np.inf, -np.inf]
    hs = row_slots(g, row[4096])
    v[g.col[hs[live[hs] & (g.degrees[g.col[hs]] <= 2)][20]]] = np.nan
    return v


def revival(g, alive, up):
    """(alive, link_up) with every other dead node alive again and every other cut link restored."""
    dead = np.flatnonzero(np.asarray(alive) == 0)
    down = np.flatnonzero((np.asarray(up) == 0) & (np.arange(g.E) < g.rev))
    assert len(dead) >= 2 and len(down) >= 2
    alive2 = np.array(alive, dtype=np.uint8)
    alive2[dead[::2]] = 1
    return alive2, cut(g, np.ones(g.E, dtype=np.uint8), down[1::2])


CHUNK_EDGE_REVIVAL = 4  # the index of the revival in chunk_edge_script()


def chunk_edge_script():
    """run(3); topology "A"; run(1); run(2); revive half of the dead and restore half of the cut
    links, the last slot of every row above one chunk among them; run(1); run(2); reset; run(2)."""
    g = chunk_edge_graph()
    alive, up = chunk_edge_topology("A")
    alive2, up2 = revival(g, alive, up)
    for d, h in chunk_edge_rows().items():
        if d > HEAVY_CHUNK:
            k = row_slots(g, h)[-1]
            alive2[g.col[k]] = 1
            up2[[k, g.rev[k]]] = 1
    return [("run", 3), ("topology", alive, up), ("run", 1), ("run", 2), ("topology", alive2, up2), ("run", 1), ("run", 2),
            ("reset",), ("run", 2)]


@functools.lru_cache(maxsize=None)
def chunk_edge_case(family):
    """(g, v, script, the restatement's Result) of the scripted chunk-edge run."""
    g, v, script = chunk_edge_graph(), chunk_edge_values(family), chunk_edge_script()
    return g, v, script, churn_python(*g.arrays(), v, script)


# ------------------------------------------------------------------------------------
# a topology call before every round
# ------------------------------------------------------------------------------------
FLAP_ROUNDS = 10


@functools.lru_cache(maxsize=None)
def flapping_case():
    """(g, v, script, Result) on tile_limit_graph(): FLAP_ROUNDS times a topology of fresh random
    masks (the heavy row kept alive) and one round."""
    g = tile_limit_graph()
    v = fu.uniform_values(g.n, seed=3)
    h = tile_segment("heavy")[0]
    script = []
    for r in range(FLAP_ROUNDS):
        script += [("topology",) + random_masks(g, 0.15, 0.15, 50 + r, keep=(h,)), ("run", 1)]
    return g, v, script, churn_python(*g.arrays(), v, script)


# ------------------------------------------------------------------------------------
# mask bytes other than 0 and 1
# ------------------------------------------------------------------------------------
def byte_masks(g, seed):
    """(alive, link_up) as a C caller may pass them (include/fu.h: non-zero = on): alive bytes from
    {0, 1, 2, 128, 255}; link_up bytes from {0, 7, 255}, zero on both slots of a link or on
    neither, and where on, 7 on one slot and 255 on its reverse."""
    rng = np.random.default_rng(seed)
    alive = rng.choice(np.array([0, 1, 2, 128, 255], dtype=np.uint8), size=g.n)
    on = random_masks(g, 0.0, 0.25, seed)[1] != 0
    up = np.where(on, np.where(np.arange(g.E) < g.rev, 7, 255), 0).astype(np.uint8)
    assert set(alive.tolist()) == {0, 1, 2, 128, 255} and set(up.tolist()) == {0, 7, 255}
    assert np.array_equal(up != 0, up[g.rev] != 0) and (up[on] != up[g.rev][on]).all()
    return alive, up
