"""Shared by the pairwise-engine tests (fu.PairwiseSync): three restatements of the synchronous
pairwise round that never run the engine.

(a) `matching_py`: the matching of a round on Python ints (the hash, the proposals, the
    listener's choice).
(b) `pair_trace` / `oracle_pair`: the rounds as a synthetic tick trace for the pinned C oracle
    (coracle.replay, events RECV / FIRE_PW). A round is three ticks: the initiators'
    FIRE_PW(s, deg_i, m1); the listeners' RECV(t, m1) and FIRE_PW(t, deg_j, m2); the initiators'
    RECV(s, m2). Nobody fires on the last receive: that is the engine's one deviation from
    PW:100.
(c) `pair_python`: the rule on Python lists and floats, for graphs of about 100 nodes; the
    values may change from round to round.

`seed` is an int, or a callable r -> int where the seed changes between runs; r counts rounds
since the last reset.
"""
import functools

import numpy as np

import coracle
import fu
from lossy_cases import M64, splitmix_at_py

_MATCHINGS = {}

# The matching seed of the GPU cases and of the conditions on their inputs, and the length of
# the runs on class_graph().
SEED = 11
CLASS_ROUNDS = 40


# ------------------------------------------------------------------------------------
# (a) the matching on Python ints
# ------------------------------------------------------------------------------------
def matching_py(rowptr, col, seed, r):
    """(mate, initiator) of round r: mate[i] = partner or -1, initiator[i] = 1 for the proposer
    of a pair."""
    rp, col = [int(x) for x in rowptr], [int(x) for x in col]
    n = len(rp) - 1
    key = splitmix_at_py(seed & M64, r)
    h = [splitmix_at_py(key, i) for i in range(n)]
    best = {}  # listener -> (priority, proposer)
    for i in range(n):
        deg = rp[i + 1] - rp[i]
        if deg == 0 or not h[i] & 1:
            continue  # idle, or a listener
        j = col[rp[i] + (h[i] >> 1) % deg]
        if h[j] & 1:
            continue  # j proposes too
        pri = ((h[i] >> 32) << 32) | i
        if j not in best or pri < best[j][0]:
            best[j] = (pri, i)
    mate, initiator = [-1] * n, [0] * n
    for j, (_, i) in best.items():
        mate[i], mate[j], initiator[i] = j, i, 1
    return mate, initiator


def _seed_at(seed, r):
    return int(seed(r) if callable(seed) else seed)


class Recorded:
    """In place of a seed: the matching of every round as recorded arrays mate[r][i] and
    initiator[r][i] (tests/golden/rule_pair_hub_mix.npz), so that no hash is evaluated."""

    def __init__(self, mate, initiator):
        self.mate, self.initiator = np.asarray(mate), np.asarray(initiator)

    def pairs(self, rowptr, col, rev, r):
        """[(i, s, j, t)] of round r, by listener; s is where j stands in row i (rows hold a
        neighbour once)."""
        out = []
        for j in np.flatnonzero((self.mate[r] >= 0) & (self.initiator[r] == 0)):
            i = int(self.mate[r][j])
            assert self.initiator[r][i] and int(self.mate[r][i]) == j
            (s,) = np.flatnonzero(col[rowptr[i]:rowptr[i + 1]] == j)
            out.append((i, int(s), int(j), int(rev[rowptr[i] + s]) - int(rowptr[j])))
        return out


def pairs_of_round(rowptr, col, rev, seed, r):
    """[(i, s, j, t)] of round r, by listener: i fires on its slot s, j answers on its slot t.
    From matching_py; the slot is the proposer's pick, restated here. A `Recorded` in place of
    the seed gives its own pairs."""
    rp = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int32)
    if isinstance(seed, Recorded):
        return seed.pairs(rp, col, rev, r)
    sd = _seed_at(seed, r)
    k = (rp.tobytes(), col.tobytes(), sd, r)
    if k not in _MATCHINGS:
        _MATCHINGS[k] = matching_py(rp, col, sd, r)
    mate, initiator = _MATCHINGS[k]
    key = splitmix_at_py(sd & M64, r)
    out = []
    for j in range(len(rp) - 1):
        i = mate[j]
        if i < 0 or initiator[j]:
            continue
        s = (splitmix_at_py(key, i) >> 1) % int(rp[i + 1] - rp[i])
        assert int(col[rp[i] + s]) == j
        out.append((i, s, j, int(rev[rp[i] + s]) - int(rp[j])))
    return out


def pair_count(rowptr, col, rev, seed, rounds):
    return sum(len(pairs_of_round(rowptr, col, rev, seed, r)) for r in range(rounds))


def roles(rowptr, col, rev, seed, rounds):
    """(initiators, listeners): the sets of nodes that were one in some round < rounds."""
    ini, lis = set(), set()
    for r in range(rounds):
        for i, _, j, _ in pairs_of_round(rowptr, col, rev, seed, r):
            ini.add(i)
            lis.add(j)
    return ini, lis


# ------------------------------------------------------------------------------------
# (b) the rounds as a trace for coracle.replay
# ------------------------------------------------------------------------------------
def pair_trace(rowptr, col, rev, rounds, seed):
    """tick_task_off, tasks, events, out_ids, n_msgs for coracle.replay: ticks 3r, 3r + 1 and
    3r + 2 are round r. Pair q of the run sends message 2q (i -> j) and 2q + 1 (j -> i)."""
    rp = np.asarray(rowptr, dtype=np.int64)
    deg = np.diff(rp)
    tasks, events, tto = [], [], [0]
    q = 0
    for r in range(rounds):
        pairs = pairs_of_round(rp, col, rev, seed, r)
        for p, (i, s, _, _) in enumerate(pairs):  # tick 3r
            tasks.append((i, len(events), len(events) + 1))
            events.append((2, s, int(deg[i]), 2 * (q + p)))
        tto.append(len(tasks))
        for p, (_, _, j, t) in enumerate(pairs):  # tick 3r + 1
            tasks.append((j, len(events), len(events) + 2))
            events.append((0, t, 2 * (q + p), 0))
            events.append((2, t, int(deg[j]), 2 * (q + p) + 1))
        tto.append(len(tasks))
        for p, (i, s, _, _) in enumerate(pairs):  # tick 3r + 2
            tasks.append((i, len(events), len(events) + 1))
            events.append((0, s, 2 * (q + p) + 1, 0))
        tto.append(len(tasks))
        q += len(pairs)
    return {"tick_task_off": np.array(tto, dtype=np.int64),
            "tasks": np.array(tasks, dtype=np.int32).reshape(-1, 3),
            "events": np.array(events, dtype=np.int32).reshape(-1, 4),
            "out_ids": np.zeros(0, dtype=np.int32),
            "n_msgs": 2 * q, "pairs": q}


def oracle_pair(rowptr, col, rev, values, rounds, seed, snaps=()):
    """(last, f, c, {r: last after round r}) after `rounds` rounds from zero, through the C
    oracle's replay. snaps: round indices (0-based) whose last averages to keep."""
    t = pair_trace(rowptr, col, rev, rounds, seed)
    if len(t["tasks"]) == 0:  # nothing ever happens: the zero state
        n, E = len(rowptr) - 1, int(rowptr[-1])
        return np.zeros(n), np.zeros(E), np.zeros(E), {r: np.zeros(n) for r in snaps}
    last, flow, est, sn = coracle.replay(rowptr, values, t["tick_task_off"], t["tasks"], t["events"], t["out_ids"],
                                         t["n_msgs"], snap_ticks=tuple(3 * r + 2 for r in snaps))
    return (last, np.ascontiguousarray(flow, dtype=np.float64), np.ascontiguousarray(est, dtype=np.float64),
            {r: sn[3 * r + 2].copy() for r in snaps})


# ------------------------------------------------------------------------------------
# (c) the rule on Python floats
# ------------------------------------------------------------------------------------
def pair_python(rowptr, col, rev, values, rounds, seed):
    """(last, f, c) after `rounds` rounds. values: one array, or a callable r -> array (the
    inputs of round r)."""
    rp = [int(x) for x in rowptr]
    n, E = len(rp) - 1, rp[-1]
    f, c, last = [0.0] * E, [0.0] * E, [0.0] * n

    def fire(v, node, slot):
        S = 0.0
        for k in range(rp[node], rp[node + 1]):
            S = S + f[k]
        x = v[node] - S
        k = rp[node] + slot
        a = (c[k] + x) / 2.0
        f[k] = (f[k] + a) - c[k]
        c[k] = a
        last[node] = a
        return f[k], a

    for r in range(rounds):
        v = [float(x) for x in (values(r) if callable(values) else values)]
        for i, s, j, t in pairs_of_round(rowptr, col, rev, seed, r):
            F, A = fire(v, i, s)
            c[rp[j] + t], f[rp[j] + t] = A, -F
            F, A = fire(v, j, t)
            c[rp[i] + s], f[rp[i] + s] = A, -F
    return np.array(last, dtype=np.float64), np.array(f, dtype=np.float64), np.array(c, dtype=np.float64)


# ------------------------------------------------------------------------------------
# graphs
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rr256_d8():
    return fu.Graph.random_regular(256, 8, seed=1)


# The engine's degree boundaries: a pair with a row above 64 slots leaves the lane groups for
# one block per pair, which stages its rows in chunks of 1024 slots; the lane groups load 8
# slots per step.
BOUNDARY_DEGREES = [64, 65, 1024, 1025]
CLASS_DEGREES = [0, 1, 2, 7, 8, 9, 63] + BOUNDARY_DEGREES + [1023, 2500]


@functools.lru_cache(maxsize=None)
def class_graph():
    """Star centres of exactly CLASS_DEGREES (node c has degree CLASS_DEGREES[c]), their leaves
    drawn from a random background graph of 3000 nodes that never touches a centre."""
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


# At seed 11 the centre of degree 1025 never listens on slot 1024, the only slot of its second
# chunk, within 40 rounds; at this seed it does in round 4 (test_engine_case_inputs.py).
LAST_SLOT_SEED, LAST_SLOT_ROUNDS = 252, 6

DENSE66_N, DENSE66_HALF = 6144, 33


@functools.lru_cache(maxsize=None)
def dense66():
    """The circulant graph on 6144 nodes with neighbours i +- 1 .. i +- 33: every row has degree
    66, so every pair joins two rows above 64 slots, and a round matches more pairs than the
    1024 blocks that share the engine's list of them."""
    i = np.repeat(np.arange(DENSE66_N), DENSE66_HALF)
    j = (i + np.tile(np.arange(1, DENSE66_HALF + 1), DENSE66_N)) % DENSE66_N
    return fu.Graph.from_edges(DENSE66_N, i, j)
