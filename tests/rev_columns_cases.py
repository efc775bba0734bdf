"""Shared by the tests of the K-column lossy and churn handles (fu.CollectAllLossyBatch,
fu.CollectAllChurnBatch; csrc/fu_rev_round.h k_light_cols / k_heavy_cols): the K-dependent plan of
light tiles restated from rowptr alone, graphs built per K that close those tiles in every way and
put heavy rows on both sides of a chunk of 2048 // K slots, the scripts of the cases, and the
per-column references. A reference never runs the engine: column c of a K-column run is
churn_cases.churn_python or lossy_cases.oracle_lossy / lossy_python on column c alone."""
import functools

import numpy as np

import fu
from churn_cases import Step, churn_python, cut, random_masks, revival, row_slots
from lossy_cases import TILE_HEAVY_DEG, TILE_ROWS, TILE_SLOTS, hashed, lossy_python, oracle_lossy
from parity_util import assert_same_bits

WIDTHS = (1, 2, 3, 5, 8, 16)
HEAVY_WIDTHS = (2, 3, 16)
LOSS_SEED = 11


def columns(n, K, first=0):
    """(n, K) inputs: column c is fu.uniform_values at seed first + c."""
    return np.ascontiguousarray(np.stack([fu.uniform_values(n, seed=first + c) for c in range(K)], axis=1))


# ------------------------------------------------------------------------------------
# the plan of light tiles for K columns (csrc/fu_rev_round.h plan_rows)
# ------------------------------------------------------------------------------------
def tile_census_k(rowptr, K):
    """[(first row, end row, slots, why)] of the light tiles planned for K columns: as
    lossy_cases.tile_census with at most 256 // K rows and 2048 // K slots per tile."""
    rp = [int(x) for x in rowptr]
    n = len(rp) - 1
    max_rows, max_slots = TILE_ROWS // K, TILE_SLOTS // K
    out, i = [], 0
    while i < n:
        if rp[i + 1] - rp[i] > TILE_HEAVY_DEG:
            i += 1
            continue
        j = i
        while True:
            if j == n:
                why = "end"
            elif j - i == max_rows:
                why = "rows"
            elif rp[j + 1] - rp[j] > TILE_HEAVY_DEG:
                why = "heavy"
            elif rp[j + 1] - rp[i] > max_slots:
                why = "slots"
            else:
                j += 1
                continue
            break
        assert j > i  # a light row alone always fits: 128 * 16 = 2048
        out.append((i, j, rp[j] - rp[i], why))
        i = j
    return out


def _stars(n, centres, degrees, leaves):
    """Edges that give centres[q] degrees[q] leaves of its own, taken from `leaves` in order."""
    src, dst, first = [], [], 0
    for h, d in zip(centres, degrees):
        src.append(np.full(d, h))
        dst.append(leaves[first:first + d])
        first += d
    assert first <= len(leaves)
    return np.concatenate(src), np.concatenate(dst), first


@functools.lru_cache(maxsize=None)
def light_boundary_graph(K):
    """Rows in id order, R = 256 // K and S = 2048 // K: R isolated rows (a tile closed by the row
    limit, no slot); 2 R rows of degree 1, linked in pairs (two tiles closed by the row limit);
    S slots split over max(2, ceil(S / 128)) rows (a tile of exactly S slots that the next row
    closes on the slot limit); three rows of degree 128 (each alone in a tile at K = 16, the first
    two closed by the slot limit); a row of
    degree 129, a row of degree 128 and a row of degree 129 (a row alone in a tile at every K,
    between two heavy rows); then the leaves of all of these, of degree 1. Returns (g, info)."""
    R, S = TILE_ROWS // K, TILE_SLOTS // K
    m = max(2, -(-S // TILE_HEAVY_DEG))
    split = [S // m + (1 if q < S % m else 0) for q in range(m)]
    assert sum(split) == S and max(split) <= TILE_HEAVY_DEG
    c0 = 3 * R
    centres = list(range(c0, c0 + m + 6))
    degrees = split + [128, 128, 128, 129, 128, 129]
    first_leaf = c0 + len(centres)
    n = first_leaf + sum(degrees)
    pair = R + 2 * np.arange(R)
    s, d, used = _stars(n, centres, degrees, np.arange(first_leaf, n))
    assert used == n - first_leaf
    g = fu.Graph.from_edges(n, np.concatenate([pair, s]), np.concatenate([pair + 1, d]))
    deg = [int(x) for x in g.degrees]
    assert deg[:R] == [0] * R and deg[R:3 * R] == [1] * (2 * R) and deg[c0:first_leaf] == degrees
    return g, {"split": (c0, c0 + m), "alone": c0 + m + 4, "R": R, "S": S}


def check_light_boundary_plan(K):
    """The boundary graph of K really closes its tiles on the row limit, on the slot limit with
    exactly 2048 // K slots, and holds a row alone in a tile."""
    g, info = light_boundary_graph(K)
    tiles = tile_census_k(g.rowptr, K)
    R, S = info["R"], info["S"]
    assert tiles[0] == (0, R, 0, "rows") and tiles[1] == (R, 2 * R, R, "rows") and tiles[2][3] == "rows"
    assert (info["split"][0], info["split"][1], S, "slots") in tiles
    assert (info["alone"], info["alone"] + 1, 128, "heavy") in tiles
    if K == 16:
        assert sum(1 for t in tiles if t[1] - t[0] == 1 and t[2] == 128 and t[3] == "slots") == 2
    for i, j, slots, _ in tiles:
        assert j - i <= R and slots <= S and slots * K <= TILE_SLOTS
    return tiles


# ------------------------------------------------------------------------------------
# heavy rows on both sides of a chunk of 2048 // K slots
# ------------------------------------------------------------------------------------
def chunk_slots(K):
    return TILE_SLOTS // K


def heavy_degrees(K):
    """129, ce - 1, ce, ce + 1, 2 ce and 2 ce + 1 for ce = 2048 // K, those above 128: at K = 16,
    ce + 1 = 129 is both the first heavy degree and the first row of two chunks."""
    ce = chunk_slots(K)
    return sorted({d for d in (TILE_HEAVY_DEG + 1, ce - 1, ce, ce + 1, 2 * ce, 2 * ce + 1) if d > TILE_HEAVY_DEG})


@functools.lru_cache(maxsize=None)
def heavy_boundary_graph(K):
    """(g, {degree: id}): star centres of heavy_degrees(K), linked to each other, all but two at
    the first ids and two at n - 2 and n - 1; the rest of each degree is leaves of its own, every
    4th leaf linked to the next one. A row's slots are in ascending neighbour id."""
    degs = heavy_degrees(K)
    k = len(degs)
    n_leaf = sum(degs) - k * (k - 1)
    n = k + n_leaf
    order = degs[2:] + degs[:2]  # the two smallest rows go last
    heavy = list(range(k - 2)) + [n - 2, n - 1]
    leaves = np.setdiff1d(np.arange(n), heavy)
    s, d, used = _stars(n, heavy, [x - (k - 1) for x in order], leaves)
    assert used == n_leaf
    hs = np.array([heavy[p] for p in range(k) for q in range(p + 1, k)])
    hd = np.array([heavy[q] for p in range(k) for q in range(p + 1, k)])
    g = fu.Graph.from_edges(n, np.concatenate([hs, s, leaves[:-1:4]]), np.concatenate([hd, d, leaves[1::4]]))
    rows = {int(g.degrees[h]): h for h in heavy}
    assert sorted(rows) == degs and [int(i) for i in np.flatnonzero(g.degrees > TILE_HEAVY_DEG)] == sorted(heavy)
    return g, rows


def heavy_boundary_script(K):
    """run(2); topology A; run(1); run(2); topology B; run(1); topology C; run(2); reset; run(2).
    A: a tenth of the leaves dead and a twentieth of the links down (heavy rows alive); on every
       row of more than one chunk the slots at positions 0, ce - 1, ce and d - 1 DOWN (both sides
       of the chunk boundary); on the row of degree 2 ce the whole second chunk DOWN.
    B: every other dead node alive again and every other cut link restored: UP, DOWN and FRESH
       slots in one chunk.
    C: B, and the smallest heavy row alive with every link cut, the largest heavy row dead.
    Returns (script, the events as [(alive, link_up)])."""
    g, rows = heavy_boundary_graph(K)
    ce = chunk_slots(K)
    heavy = list(rows.values())
    alive, up = random_masks(g, 0.1, 0.05, 40 + K, keep=heavy)
    for d, h in rows.items():
        if d > ce:
            ks = row_slots(g, h)
            beside = ks[[ce - 2, min(ce + 1, d - 1)]]  # live slots next to the DOWN ones
            alive[g.col[beside]] = 1
            up[beside] = 1
            up[g.rev[beside]] = 1
            up = cut(g, up, ks[[0, ce - 1, ce, d - 1]])
    up = cut(g, up, row_slots(g, rows[2 * ce])[ce:2 * ce])
    alive2, up2 = revival(g, alive, up)
    alive3, up3 = alive2.copy(), cut(g, up2, row_slots(g, rows[min(rows)]))
    alive3[rows[max(rows)]] = 0
    events = [(alive, up), (alive2, up2), (alive3, up3)]
    script = [("run", 2), ("topology",) + events[0], ("run", 1), ("run", 2), ("topology",) + events[1], ("run", 1),
              ("topology",) + events[2], ("run", 2), ("reset",), ("run", 2)]
    return script, events


# ------------------------------------------------------------------------------------
# references per column, and an engine driven through a script
# ------------------------------------------------------------------------------------
def column_script(script, c):
    """The script of column c: a ("values", (n, K)) step becomes ("values", column c)."""
    return [("values", np.asarray(s[1])[:, c]) if s[0] == "values" else s for s in script]


def churn_reference(g, V, script):
    """[Step] after every script step for (n, K) inputs V: churn_python once per column, the
    estimates and flows stacked to (n, K) and (E, K); states and counts agree over the columns."""
    V = np.asarray(V)
    per = [churn_python(*g.arrays(), V[:, c], column_script(script, c)).steps for c in range(V.shape[1])]
    out = []
    for q in range(len(script)):
        s0 = per[0][q]
        for s in (p[q] for p in per[1:]):
            assert np.array_equal(s.state, s0.state) and (s.alive_nodes, s.live_slots) == (s0.alive_nodes, s0.live_slots)
        out.append(Step(np.stack([s[q].a for s in per], axis=1), np.stack([s[q].f for s in per], axis=1), s0.state,
                        s0.alive_nodes, s0.live_slots))
    return out


def drive_churn(eng, script, steps, what, after=None):
    """Apply the script to a churn engine (scalar or K columns) and compare estimates, flows, slot
    states and stats with steps[q] after every step."""
    for q, s in enumerate(script):
        if s[0] == "run":
            eng.run(s[1])
        elif s[0] == "topology":
            eng.set_topology(s[1], s[2])
        elif s[0] == "values":
            eng.set_values(s[1])
        else:
            eng.reset()
        want = steps[q]
        assert_same_bits(eng.estimates(), want.a, what + ("estimates", q, s[0]))
        assert_same_bits(eng.flows(), want.f, what + ("flows", q, s[0]))
        assert np.array_equal(eng.slot_state(), want.state), what + ("states", q)
        assert eng.stats == (want.alive_nodes, want.live_slots), what + ("stats", q)
        if after is not None:
            after(q)


def lossy_reference(g, V, stops, p, seed=LOSS_SEED, down=None, python=False):
    """{stop: (a (n, K), f (E, K))} after `stop` rounds from zero under (p, seed, down): the C
    oracle's replay (or lossy_python) once per column and stop."""
    V = np.asarray(V)
    delivered = hashed(p, seed, g.E, down)
    out = {}
    for stop in stops:
        if python:
            per = [lossy_python(*g.arrays(), V[:, c], stop, delivered) for c in range(V.shape[1])]
        else:
            per = [oracle_lossy(*g.arrays(), V[:, c], stop, delivered)[:2] for c in range(V.shape[1])]
        out[stop] = (np.stack([a for a, _ in per], axis=1), np.stack([f for _, f in per], axis=1))
    return out


def link_mask(g, frac, seed):
    """down[E]: about `frac` of the undirected links lost in every round, both directions."""
    return (random_masks(g, 0.0, frac, seed)[1] == 0).astype(np.uint8)
