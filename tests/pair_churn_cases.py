"""Shared by the tests of the pairwise engine under churn (fu.PairwiseSync.set_topology):
restatements of the rounds under a topology that never run the engine, the case graphs and the
scripts of events.

A topology is the pair (alive[n], link_up[E]), None = all ones; slot k = (i -> j) is live iff
link_up[k] and alive[i] and alive[j]. A script is {round: (alive, link_up)}: the topology set
before that round. At an event a slot that stops being live loses f and c on both ends; one
that becomes live keeps the +0.0 it holds.

(a) `live_np`: the liveness rule on numpy; `matching_live_py`: the matching of a round on the
    live subgraph, on Python ints (a proposer takes its p-th live slot in row order,
    p = (h >> 1) % ldeg); `pairs_live` the pairs [(i, s, j, t)] of it, s and t row-relative.
(b) `pair_churn_python`: the rule on Python lists and floats, pair_cases.pair_python /
    pair_loss_cases.pair_loss_python with the script: the same fire, except that the sum runs
    over the live slots only, as the reference's `neighbors` would hold them. Without a script
    it returns what those two return (test_pair_churn_case_inputs.py).
(c) `subgraph`: the live subgraph as a CSR of its own (same n and ids, each row its live slots
    in row order) with the map from its slots back to the caller's.
"""
import functools

import numpy as np

import fu
from lossy_cases import M64, splitmix_at_py
from pair_cases import SEED  # noqa: F401  (the matching seed of the cases)

_MATCHINGS = {}

K_CASES = (2, 3, 16)
# The engine's degree boundaries under a topology: kLightDeg, kChunk, and kColsChunk / K slots
# per chunk of the K-column heavy kernel at K = 2, 3 and 16 (1024, 682, 128).
EDGE_DEGREES = [64, 65, 1024, 1025]
COLS_EDGE_DEGREES = sorted({2048 // K + d for K in K_CASES for d in (0, 1)})  # 128, 129, 682, 683, 1024, 1025
CLASS_DEGREES = [0, 1, 2, 7, 8, 9, 63, 64, 65, 128, 129, 682, 683, 1023, 1024, 1025, 2500]
ONLY_LAST, NO_LIVE, DEAD_HEAVY = 3, 2, 16  # centres: degree 7, all but the last slot down; degree 2, both down; degree 2500, dead
CLASS_ROUNDS, CLASS_EVENTS = 40, (10, 20, 30)


# ------------------------------------------------------------------------------------
# (a) liveness and the matching
# ------------------------------------------------------------------------------------
def live_np(rowptr, col, alive=None, link_up=None):
    """bool[E]."""
    rp = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n, E = len(rp) - 1, len(col)
    a = np.ones(n, dtype=bool) if alive is None else np.asarray(alive) != 0
    u = np.ones(E, dtype=bool) if link_up is None else np.asarray(link_up) != 0
    src = np.repeat(np.arange(n), np.diff(rp))
    return u & a[src] & a[col]


def matching_live_py(rowptr, col, live, seed, r):
    """(mate, initiator, slot) of round r on the live subgraph: slot[i] is the absolute slot a
    matched initiator fires on, else -1."""
    rp, col = [int(x) for x in rowptr], [int(x) for x in col]
    n = len(rp) - 1
    key = splitmix_at_py(int(seed) & M64, r)
    h = [splitmix_at_py(key, i) for i in range(n)]
    best = {}  # listener -> (priority, proposer, slot)
    for i in range(n):
        if not h[i] & 1:
            continue  # a listener
        mine = [k for k in range(rp[i], rp[i + 1]) if live[k]]
        if not mine:
            continue  # idle: dead, or no live slot
        ks = mine[(h[i] >> 1) % len(mine)]
        j = col[ks]
        if h[j] & 1:
            continue  # j proposes too
        pri = ((h[i] >> 32) << 32) | i
        if j not in best or pri < best[j][0]:
            best[j] = (pri, i, ks)
    mate, initiator, slot = [-1] * n, [0] * n, [-1] * n
    for j, (_, i, ks) in best.items():
        mate[i], mate[j], initiator[i], slot[i] = j, i, 1, ks
    return mate, initiator, slot


def pairs_live(rowptr, col, rev, live, seed, r):
    """[(i, s, j, t)] of round r under `live` (bool[E]), by listener."""
    rp = np.asarray(rowptr, dtype=np.int64)
    live = np.asarray(live, dtype=bool)
    k = (rp.tobytes(), np.asarray(col, dtype=np.int32).tobytes(), live.tobytes(), int(seed), r)
    if k not in _MATCHINGS:
        _MATCHINGS[k] = matching_live_py(rp, col, live, seed, r)
    mate, initiator, slot = _MATCHINGS[k]
    out = []
    for j in range(len(rp) - 1):
        i = mate[j]
        if i < 0 or initiator[j]:
            continue
        ks = slot[i]
        out.append((i, ks - int(rp[i]), j, int(rev[ks]) - int(rp[j])))
    return out


def topology_at(script, r, n, E):
    """(alive, link_up) as uint8 arrays in force in round r: the last event at or before it."""
    alive, link_up = np.ones(n, dtype=np.uint8), np.ones(E, dtype=np.uint8)
    for at in sorted(script):
        if at <= r:
            a, u = script[at]
            alive = np.ones(n, dtype=np.uint8) if a is None else (np.asarray(a) != 0).astype(np.uint8)
            link_up = np.ones(E, dtype=np.uint8) if u is None else (np.asarray(u) != 0).astype(np.uint8)
    return alive, link_up


def live_at(rowptr, col, script, r):
    a, u = topology_at(script, r, len(rowptr) - 1, len(col))
    return live_np(rowptr, col, a, u)


# ------------------------------------------------------------------------------------
# (b) the rule on Python floats
# ------------------------------------------------------------------------------------
def pair_churn_python(rowptr, col, rev, values, rounds, seed, script, lost=None, keep=None, err=None):
    """(last, f, c) after `rounds` rounds under `script`. lost: None, or r -> bool[E] as in
    pair_loss_cases. keep: a list that gets a copy of `last` after every round. err: None, or
    (targets of round r as a callable r -> array, list) that gets max |last - target| over the
    alive nodes after every round (0.0 where none is alive)."""
    rp = [int(x) for x in rowptr]
    n, E = len(rp) - 1, rp[-1]
    f, c, last = [0.0] * E, [0.0] * E, [0.0] * n
    live = [True] * E
    v = [float(x) for x in values]

    def fire(node, slot):
        S = 0.0
        for k in range(rp[node], rp[node + 1]):
            if live[k]:  # the reference sums over `neighbors`, which holds the live ones
                S = S + f[k]
        x = v[node] - S
        k = rp[node] + slot
        a = (c[k] + x) / 2.0
        f[k] = (f[k] + a) - c[k]
        c[k] = a
        last[node] = a
        return f[k], a

    for r in range(rounds):
        if r in script:
            new = live_at(rowptr, col, script, r)
            for k in range(E):
                if live[k] and not new[k]:
                    f[k] = c[k] = 0.0  # the entry is deleted; it comes back as the defaultdict's 0.0
            live = [bool(x) for x in new]
        L = lost(r) if lost is not None else None
        for i, s, j, t in pairs_live(rowptr, col, rev, live, seed, r):
            ks, kt = rp[i] + s, rp[j] + t
            assert live[ks] and live[kt]
            F, A = fire(i, s)
            if L is not None and L[kt]:
                continue  # m1 lost
            c[kt], f[kt] = A, -F
            F, A = fire(j, t)
            if L is not None and L[ks]:
                continue  # m2 lost
            c[ks], f[ks] = A, -F
        if keep is not None:
            keep.append(np.array(last, dtype=np.float64))
        if err is not None:
            tg, out = err
            a, _ = topology_at(script, r, n, E)
            d = np.abs(np.array(last) - np.asarray(tg(r)))[a != 0]
            out.append(float(d.max()) if len(d) else 0.0)
    return np.array(last, dtype=np.float64), np.array(f, dtype=np.float64), np.array(c, dtype=np.float64)


# ------------------------------------------------------------------------------------
# (c) the live subgraph
# ------------------------------------------------------------------------------------
def subgraph(rowptr, col, live):
    """(rowptr', col', rev', slots): the live subgraph with the same n and ids, each row holding
    its live slots in row order; slots[k'] is the caller's slot of k'."""
    rp = np.asarray(rowptr, dtype=np.int64)
    live = np.asarray(live, dtype=bool)
    n = len(rp) - 1
    src = np.repeat(np.arange(n), np.diff(rp))
    slots = np.flatnonzero(live)
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(src[live], minlength=n))]).astype(np.int64)
    col2 = np.asarray(col, dtype=np.int32)[slots]
    return rp2, col2, slots


def sub_rev(rev, live, slots):
    """rev of the subgraph: the caller's rev through the slot map."""
    back = np.full(len(live), -1, dtype=np.int64)
    back[slots] = np.arange(len(slots))
    out = back[np.asarray(rev, dtype=np.int64)[slots]]
    assert (out >= 0).all()  # liveness is symmetric
    return out.astype(np.int32)


# ------------------------------------------------------------------------------------
# graphs and scripts
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def class_graph():
    """pair_cases.class_graph with the centres of CLASS_DEGREES (node c has degree
    CLASS_DEGREES[c]): the leaves are drawn from a random background graph of 3000 nodes that
    never touches a centre."""
    rng = np.random.default_rng(7)
    k, n_leaf = len(CLASS_DEGREES), 3000
    src, dst = [], []
    for c, d in enumerate(CLASS_DEGREES):
        src.append(np.full(d, c))
        dst.append(k + rng.choice(n_leaf, size=d, replace=False))
    src.append(k + rng.integers(0, n_leaf, 2 * n_leaf))
    dst.append(k + rng.integers(0, n_leaf, 2 * n_leaf))
    g = fu.Graph.from_edges(k + n_leaf, np.concatenate(src), np.concatenate(dst))
    assert [int(x) for x in g.degrees[:k]] == CLASS_DEGREES
    return g


def _links_down(g, slots):
    """link_up with the given slots and their reverses down."""
    up = np.ones(g.E, dtype=np.uint8)
    s = np.asarray(slots, dtype=np.int64)
    up[s] = 0
    up[np.asarray(g.rev, dtype=np.int64)[s]] = 0
    return up


@functools.lru_cache(maxsize=None)
def class_script():
    """{round: (alive, link_up)} on class_graph(), events before rounds 10, 20 and 30.
    10: the centre of degree 2500 and 5 % of the leaves die.
    20: they stay dead; a fifth of the links goes down, among them the first and the last slot of
        every centre of degree >= 8, all but the last slot of the centre of degree 7 and both
        slots of the centre of degree 2.
    30: every node is back; the links stay as they were."""
    g = class_graph()
    rp = np.asarray(g.rowptr, dtype=np.int64)
    rev = np.asarray(g.rev, dtype=np.int64)
    k = len(CLASS_DEGREES)
    rng = np.random.default_rng(19)
    alive = np.ones(g.n, dtype=np.uint8)
    alive[DEAD_HEAVY] = 0
    alive[k + np.flatnonzero(rng.random(g.n - k) < 0.05)] = 0
    one = np.flatnonzero(np.arange(g.E) < rev)
    down = list(one[rng.random(len(one)) < 0.2])
    for c, d in enumerate(CLASS_DEGREES):
        if d >= 8:
            down += [int(rp[c]), int(rp[c + 1]) - 1]
    down += list(range(int(rp[ONLY_LAST]), int(rp[ONLY_LAST + 1]) - 1))
    down += list(range(int(rp[NO_LIVE]), int(rp[NO_LIVE + 1])))
    up = _links_down(g, down)
    # the last slot of the centre of degree 7 stays, whatever the draw said
    last = int(rp[ONLY_LAST + 1]) - 1
    up[last] = up[rev[last]] = 1
    return {10: (alive, None), 20: (alive, up), 30: (None, up)}


def class_values(K=None, seed=3):
    g = class_graph()
    rng = np.random.default_rng(seed)
    return rng.random(g.n) * 100.0 if K is None else rng.random((g.n, K)) * 100.0


def random_topology(g, seed, dead=0.15, down=0.25):
    """(alive, link_up) drawn at random: a fraction `dead` of the nodes, `down` of the links."""
    rng = np.random.default_rng(seed)
    rev = np.asarray(g.rev, dtype=np.int64)
    alive = (rng.random(g.n) >= dead).astype(np.uint8)
    one = np.flatnonzero(np.arange(g.E) < rev)
    return alive, _links_down(g, one[rng.random(len(one)) < down])


# The convergence run: a connected small graph, two events, and the length after which the
# restatement's error over the alive nodes is below 1e-9 of its value at the last event
# (test_pair_churn_case_inputs.py holds CONV_ROUNDS to that).
CONV_EVENTS, CONV_ROUNDS, CONV_EVERY = (60, 120), 1200, 20


@functools.lru_cache(maxsize=None)
def conv_graph():
    return fu.Graph.random_regular(96, 6, seed=2)


@functools.lru_cache(maxsize=None)
def conv_script():
    """60: a tenth of the nodes die and a tenth of the links go down. 120: half of the dead come
    back, the links stay down."""
    g = conv_graph()
    a1, up = random_topology(g, 4, dead=0.1, down=0.1)
    a2 = a1.copy()
    dead = np.flatnonzero(a1 == 0)
    a2[dead[::2]] = 1
    return {CONV_EVENTS[0]: (a1, up), CONV_EVENTS[1]: (a2, up)}


def conv_values():
    return np.random.default_rng(8).random(conv_graph().n) * 100.0


def conv_targets(r):
    """churn_targets under the topology in force in round r."""
    g = conv_graph()
    a, u = topology_at(conv_script(), r, g.n, g.E)
    return fu.churn_targets(g, conv_values(), a, u)


# ------------------------------------------------------------------------------------
# the reference's recordings (tests/golden/rule_pair_churn_hub_mix.npz)
# ------------------------------------------------------------------------------------
def load_recording():
    """The fixture as a namespace of read-only arrays: rowptr, col, rev, values, seed, p,
    loss_seed, events (rounds), alive[event][n], link_up[event][E], lost[round][E] (bool, the
    hash at (p, loss_seed)), mate and initiator [round][n], stops, and per run (0: no loss,
    1: under `lost`) last_avg[run][stop][n], flows[run][stop][E], estimates[run][stop][E]."""
    import types

    from conftest import load_npz

    d = load_npz("rule_pair_churn_hub_mix.npz")
    out = {k: d[k] for k in d.files}
    for k in ("values", "last_avg", "flows", "estimates"):
        assert out[k].dtype == np.uint64
        out[k] = out[k].view(np.float64)
    out["rowptr"] = out["rowptr"].astype(np.int64)
    out["n"], out["E"] = len(out["rowptr"]) - 1, len(out["col"])
    out["stops"] = [int(s) for s in out["stops"]]
    out["events"] = [int(s) for s in out["events"]]
    out["lost"] = np.unpackbits(out["lost"], axis=1)[:, :out["E"]].astype(bool)
    out["alive"] = np.unpackbits(out["alive"], axis=1)[:, :out["n"]]
    out["link_up"] = np.unpackbits(out["link_up"], axis=1)[:, :out["E"]]
    out["mate"] = out["mate"].astype(np.int32)
    out["initiator"] = np.unpackbits(out["initiator"], axis=1)[:, :out["n"]]
    out["p"], out["seed"], out["loss_seed"] = float(out["p"][0]), int(out["seed"][0]), int(out["loss_seed"][0])
    out["python"] = str(np.asarray(out["python"]).reshape(-1)[0])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    ns = types.SimpleNamespace(**out)
    ns.script = {r: (ns.alive[q], ns.link_up[q]) for q, r in enumerate(ns.events)}
    return ns

