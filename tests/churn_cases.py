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
