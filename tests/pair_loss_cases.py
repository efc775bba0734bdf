"""Shared by the tests of the pairwise engine under message loss (fu.PairwiseSync with loss= or
a link mask): restatements of the lossy pairwise round that never run the engine.

The matching is pair_cases' and does not look at the loss. A matched pair (i, s, j, t) has two
messages, with ks = rowptr[i] + s and kt = rowptr[j] + t: m1 goes i -> j and is received on slot
kt, m2 goes j -> i and is received on slot ks. `lost(r) -> bool[E]` says per slot whether the
message received on it in round r is lost. The outcomes (M1_LOST, M2_LOST, COMPLETE):
  m1 lost:   i fires on s; j does nothing.
  m2 lost:   i fires on s, j receives and fires back; i keeps what it fired.
  complete:  pair_cases' exchange.

(a) `pair_lost_py`: the decision on Python ints; `pair_lost_np` the same on numpy uint64 arrays
    for whole rounds; `hashed` makes the `lost` callable of a run at (p, seed) with a mask.
(b) `pair_loss_python`: pair_cases.pair_python with the `lost` argument.
(c) `pair_loss_trace` / `oracle_pair_loss`: the rounds as a trace for coracle.replay. A lost m1
    omits the listener's RECV and FIRE_PW and the initiator's RECV; a lost m2 omits only the
    initiator's RECV. The messages keep pair_cases' numbering, so a lost one is written by its
    FIRE_PW and read by nobody.
"""
import numpy as np

import coracle
from lossy_cases import GOLDEN, M64, splitmix_at_py
from pair_cases import pairs_of_round

M1_LOST, M2_LOST, COMPLETE = 0, 1, 2

# The loss seed of the GPU cases and of the conditions on their inputs (the matching seed is
# pair_cases.SEED).
LOSS_SEED = 5


# ------------------------------------------------------------------------------------
# (a) the decision
# ------------------------------------------------------------------------------------
def loss_key_py(seed, r):
    """The key of round r's decisions: the complement of the seed keeps the stream apart from
    the matching's, splitmix_at(seed, r)."""
    return splitmix_at_py(~int(seed) & M64, r)


def pair_lost_py(seed, r, first, count, p):
    """[1 if the message received on slot first + q in round r is lost]: lost iff
    u01(splitmix_at(splitmix_at(~seed, r), k)) < p, u01(x) = (x >> 11) * 2^-53. Round 0 is an
    ordinary round."""
    key = loss_key_py(seed, r)
    return [1 if (splitmix_at_py(key, first + q) >> 11) * 2.0 ** -53 < p else 0 for q in range(count)]


def pair_lost_np(seed, r, E, p):
    """bool[E] for slots 0 .. E-1 of round r: pair_lost_py on uint64 arrays."""
    key = loss_key_py(seed, r)
    with np.errstate(over="ignore"):
        z = np.uint64(key) + (np.arange(E, dtype=np.uint64) + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 < p


def hashed(p, seed, E, down=None):
    """The `lost` callable of a run at (p, seed) with an optional link mask. p, seed and down may
    each be a callable r -> value where they change between runs (down: r -> array or None)."""
    def lost(r):
        at = lambda x: x(r) if callable(x) else x  # noqa: E731
        out = pair_lost_np(at(seed), r, E, at(p))
        d = at(down)
        return out if d is None else out | (np.asarray(d) != 0)
    return lost


def outcomes(rowptr, col, rev, seed, rounds, lost):
    """[[(i, s, j, t, outcome)] per round], by listener."""
    rp = [int(x) for x in rowptr]
    out = []
    for r in range(rounds):
        L = lost(r)
        out.append([(i, s, j, t, M1_LOST if L[rp[j] + t] else M2_LOST if L[rp[i] + s] else COMPLETE)
                    for i, s, j, t in pairs_of_round(rowptr, col, rev, seed, r)])
    return out


def loss_counts(rowptr, col, rev, seed, rounds, lost):
    """(first messages lost, answers lost, complete exchanges) of rounds 0 .. rounds-1."""
    cnt = [0, 0, 0]
    for pairs in outcomes(rowptr, col, rev, seed, rounds, lost):
        for *_, o in pairs:
            cnt[o] += 1
    return tuple(cnt)


def fired_nodes(rowptr, col, rev, seed, rounds, lost):
    """The nodes that fired in some round: every initiator, and the listeners that got m1."""
    out = set()
    for pairs in outcomes(rowptr, col, rev, seed, rounds, lost):
        for i, _, j, _, o in pairs:
            out.add(i)
            if o != M1_LOST:
                out.add(j)
    return out


# ------------------------------------------------------------------------------------
# (b) the rule on Python floats
# ------------------------------------------------------------------------------------
def pair_loss_python(rowptr, col, rev, values, rounds, seed, lost, keep=None):
    """(last, f, c) after `rounds` rounds. values: one array, or a callable r -> array. keep: a
    list that gets a copy of `last` after every round."""
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
        L = lost(r)
        for i, s, j, t in pairs_of_round(rowptr, col, rev, seed, r):
            ks, kt = rp[i] + s, rp[j] + t
            F, A = fire(v, i, s)
            if L[kt]:
                continue  # m1 lost: j never hears of it
            c[kt], f[kt] = A, -F
            F, A = fire(v, j, t)
            if L[ks]:
                continue  # m2 lost: i keeps what it fired
            c[ks], f[ks] = A, -F
        if keep is not None:
            keep.append(np.array(last, dtype=np.float64))
    return np.array(last, dtype=np.float64), np.array(f, dtype=np.float64), np.array(c, dtype=np.float64)


# ------------------------------------------------------------------------------------
# (c) the rounds as a trace for coracle.replay
# ------------------------------------------------------------------------------------
def pair_loss_trace(rowptr, col, rev, rounds, seed, lost):
    """tick_task_off, tasks, events, out_ids, n_msgs for coracle.replay: ticks 3r, 3r + 1 and
    3r + 2 are round r. Pair q of the run sends message 2q (i -> j) and, if m1 arrives, 2q + 1
    (j -> i)."""
    rp = np.asarray(rowptr, dtype=np.int64)
    deg = np.diff(rp)
    tasks, events, tto = [], [], [0]
    q = 0
    for r in range(rounds):
        pairs = pairs_of_round(rp, col, rev, seed, r)
        L = lost(r)
        got1 = [not L[rp[j] + t] for _, _, j, t in pairs]
        got2 = [g and not L[rp[i] + s] for g, (i, s, _, _) in zip(got1, pairs)]
        for p, (i, s, _, _) in enumerate(pairs):  # tick 3r: every initiator fires
            tasks.append((i, len(events), len(events) + 1))
            events.append((2, s, int(deg[i]), 2 * (q + p)))
        tto.append(len(tasks))
        for p, (_, _, j, t) in enumerate(pairs):  # tick 3r + 1: the listeners that got m1
            if got1[p]:
                tasks.append((j, len(events), len(events) + 2))
                events.append((0, t, 2 * (q + p), 0))
                events.append((2, t, int(deg[j]), 2 * (q + p) + 1))
        tto.append(len(tasks))
        for p, (i, s, _, _) in enumerate(pairs):  # tick 3r + 2: the initiators that got m2
            if got2[p]:
                tasks.append((i, len(events), len(events) + 1))
                events.append((0, s, 2 * (q + p) + 1, 0))
        tto.append(len(tasks))
        q += len(pairs)
    return {"tick_task_off": np.array(tto, dtype=np.int64),
            "tasks": np.array(tasks, dtype=np.int32).reshape(-1, 3),
            "events": np.array(events, dtype=np.int32).reshape(-1, 4),
            "out_ids": np.zeros(0, dtype=np.int32),
            "n_msgs": 2 * q, "pairs": q}


def oracle_pair_loss(rowptr, col, rev, values, rounds, seed, lost, snaps=()):
    """(last, f, c, {r: last after round r}) after `rounds` rounds from zero, through the C
    oracle's replay. snaps: round indices (0-based) whose last averages to keep."""
    t = pair_loss_trace(rowptr, col, rev, rounds, seed, lost)
    if len(t["tasks"]) == 0:  # nothing ever happens: the zero state
        n, E = len(rowptr) - 1, int(rowptr[-1])
        return np.zeros(n), np.zeros(E), np.zeros(E), {r: np.zeros(n) for r in snaps}
    last, flow, est, sn = coracle.replay(rowptr, values, t["tick_task_off"], t["tasks"], t["events"], t["out_ids"],
                                         t["n_msgs"], snap_ticks=tuple(3 * r + 2 for r in snaps))
    return (last, np.ascontiguousarray(flow, dtype=np.float64), np.ascontiguousarray(est, dtype=np.float64),
            {r: sn[3 * r + 2].copy() for r in snaps})


# ------------------------------------------------------------------------------------
# the reference's recording (tests/golden/rule_pair_lossy_hub_mix.npz)
# ------------------------------------------------------------------------------------
def load_recording():
    """The fixture as a namespace of read-only arrays: rowptr, col, rev, values, p, seed (the
    matching's), loss_seed, down[E], lost[round][E] (bool: hash or mask), mate and initiator
    [round][n], stops, last_avg[stop][n], flows[stop][E], estimates[stop][E], python."""
    import types

    from conftest import load_npz

    d = load_npz("rule_pair_lossy_hub_mix.npz")
    out = {k: d[k] for k in d.files}
    for k in ("values", "last_avg", "flows", "estimates"):
        assert out[k].dtype == np.uint64
        out[k] = out[k].view(np.float64)
    out["rowptr"] = out["rowptr"].astype(np.int64)
    out["n"], out["E"] = len(out["rowptr"]) - 1, len(out["col"])
    out["stops"] = [int(s) for s in out["stops"]]
    out["lost"] = np.unpackbits(out["lost"], axis=1)[:, :out["E"]].astype(bool)
    out["p"], out["seed"], out["loss_seed"] = float(out["p"][0]), int(out["seed"][0]), int(out["loss_seed"][0])
    out["python"] = str(np.asarray(out["python"]).reshape(-1)[0])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return types.SimpleNamespace(**out)


# ------------------------------------------------------------------------------------
# the inputs of the GPU cases (conditions on them: test_pair_loss_case_inputs.py)
# ------------------------------------------------------------------------------------
CLASS_P = 0.3    # degree boundaries, dense66, value domain
CONV_P, CONV_ROUNDS = 0.1, 1500  # the error trace: the reference is below 1e-6 of its first error after 1500 rounds
MASK_CLEARED_AT = 20  # the mask-alone run: 40 rounds, the mask dropped from this round on
VD_ROUNDS = 16


def link_mask(g, seed=1, both=0.2, one_way=0.2):
    """uint8[E]: a fraction `both` of the links down in both directions, a fraction `one_way` down
    in one direction only (which one is drawn too)."""
    rev = np.asarray(g.rev, dtype=np.int64)
    one = np.flatnonzero(np.arange(g.E) < rev)
    rng = np.random.default_rng(seed)
    u = rng.random(len(one))
    flip = rng.random(len(one)) < 0.5
    down = np.zeros(g.E, dtype=np.uint8)
    b = one[u < both]
    down[b] = 1
    down[rev[b]] = 1
    o = (u >= both) & (u < both + one_way)
    down[np.where(flip[o], one[o], rev[one[o]])] = 1
    return down


def census(g, oc):
    """{"heavy_i" | "heavy_j" | "light": [m1 lost, m2 lost, complete]} over outcomes `oc`: the
    pairs whose initiator's row is above 64 slots, whose listener's row is, and the pairs that
    stay in the lane groups."""
    deg = g.degrees
    c = {"heavy_i": [0, 0, 0], "heavy_j": [0, 0, 0], "light": [0, 0, 0]}
    for pairs in oc:
        for i, _, j, _, o in pairs:
            if deg[i] > 64:
                c["heavy_i"][o] += 1
            if deg[j] > 64:
                c["heavy_j"][o] += 1
            if deg[i] <= 64 and deg[j] <= 64:
                c["light"][o] += 1
    return c
