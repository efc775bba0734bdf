#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ from the REFERENCE's own arithmetic.

This script is test infrastructure. It runs only in the build container, where the
reference checkout exists at /root/reference (override with FU_REFERENCE). Elsewhere it
prints a message and exits 0. Nothing in `tests -m gpu`, `smoke()` or `bench.py` runs it.

How it works
------------
SimGrid 4.0 (requirements.txt:2 of the reference) cannot be installed offline. So this
script puts a small stub `simgrid` module into `sys.modules` and then loads
`flowupdating-collectall.py` / `flowupdating-pairwise.py` with
`importlib.util.spec_from_file_location`. Loading only defines classes; the scripts'
`__main__` blocks (CA:151-166, PW:140-155) do not run. `sys.dont_write_bytecode` is set
first, so no `__pycache__` is written into the reference tree. Only data is written, and
only into tests/golden/.

The script then drives the reference's own `Peer.__init__`, `on_receive`, `tick` and
`avg_and_send` (CA:26-128, PW:26-117) in two ways:

* generation-synchronous rounds (collect-all): every message of generation r is delivered
  before any message of generation r+1. Delivery inside a generation is shuffled. On a
  symmetric graph the result does not depend on that order.
* tick-level emulation of `Peer.loop` (CA:70-85 / PW:69-84) with the mailbox rendez-vous
  model of SURVEY.md Appendix B. The simulated transfer time on every route is in (0, 1) s,
  so a message matched at tick t can be consumed at tick t+1 at the earliest.

Three more drivers run the rules of the lossy, pair and churn engines through the same Peers
on the graph hub_mix: `ca_lossy_sync` (generations in which a recorded mask decides which
messages arrive), `pw_sync` (the pairwise exchange over a recorded matching) and
`ca_churn_sync` (topology events between generations). The masks, matchings and live slots
come from the engines' host-only helpers (`fu.lossy_delivered`, `fu.pair_matching`; no GPU), so
libfu.so must be built.

A last stage, `value_domain_fixtures`, sends signed zeros, subnormals, values that overflow and
non-finite inputs through all of these drivers (vd_*.npz; manifest key "value_domain"): the
families subn, huge, wide, special and special_off through `ca_sync` on hub_mix, subn and special
through the three rule drivers on the recorded masks, matchings and topologies, and planted values
through `tick_emulation` on the asym12 and rr32_d4 actors. Every float in those files is stored as
its bit pattern. `--only-value-domain` runs that stage alone on the files of the earlier ones.

`row_order_fixtures` adds two collect-all recordings with shuffled rows (a hub-heavy R-MAT and a
star), from an rng of its own; `--only-row-order` runs it alone and leaves every other file as
it is.

The reference adds with the builtin `sum` (CA:106, PW:103). From CPython 3.12 on that sum is
compensated and no longer the left-to-right chain, so the script writes nothing there.

The stub stands in for SimGrid only. The arithmetic and the control flow of `on_receive`,
`tick` and `avg_and_send` are the reference's own code.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import types
from collections import deque

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("FU_REFERENCE", "/root/reference")
CA_FILE = "flowupdating-collectall.py"
PW_FILE = "flowupdating-pairwise.py"

MASK64 = (1 << 64) - 1


# ----------------------------------------------------------------------------------------
# Tie-order RNG shared with the product's trace generator (fu_trace.cpp) and the oracle.
# SplitMix64; a per-tick Fisher-Yates shuffle with j = r % (i + 1).
# ----------------------------------------------------------------------------------------
def splitmix64(state: int) -> tuple[int, int]:
    state = (state + 0x9E3779B97F4A7C15) & MASK64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return state, z ^ (z >> 31)


def tick_orders(n: int, order: str, ticks: int):
    """Yield the actor order for each tick (same spec as fu_trace.cpp)."""
    base = list(range(n))
    if order == "fwd":
        for _ in range(ticks):
            yield base
    elif order == "rev":
        rev = base[::-1]
        for _ in range(ticks):
            yield rev
    elif order.startswith("rand:"):
        st = int(order.split(":", 1)[1]) & MASK64
        for _ in range(ticks):
            perm = list(base)
            for i in range(n - 1, 0, -1):
                st, r = splitmix64(st)
                j = r % (i + 1)
                perm[i], perm[j] = perm[j], perm[i]
            yield perm
    else:
        raise ValueError(order)


# ----------------------------------------------------------------------------------------
# Stub simgrid
# ----------------------------------------------------------------------------------------
class World:
    current_host = "?"
    router = None
    errors = 0


def _install_stub() -> types.ModuleType:
    sg = types.ModuleType("simgrid")

    class Host:
        def __init__(self, name):
            self.name = name

        @staticmethod
        def by_name(name):
            return Host(name)

    class _Comm:
        pass

    class Mailbox:
        def __init__(self, name):
            self.name = name

        @staticmethod
        def by_name(name):
            return Mailbox(name)

        def put_async(self, payload, size):
            World.router(self.name, payload, size)
            return _Comm()

        def get_async(self):  # the harness emulates the receive side itself
            raise RuntimeError("get_async is driven by the harness")

    class ActivitySet:
        def __init__(self):
            self.count = 0

        def push(self, comm):  # do not keep comms alive (CA:122 FIXME)
            self.count += 1

    class Engine:
        clock = 0.0

    class Actor:
        pass

    class _ThisActor:
        @staticmethod
        def get_host():
            return Host(World.current_host)

        @staticmethod
        def info(msg):
            pass

        @staticmethod
        def error(msg):
            World.errors += 1

    sg.Host = Host
    sg.Mailbox = Mailbox
    sg.ActivitySet = ActivitySet
    sg.Engine = Engine
    sg.Actor = Actor
    sg.this_actor = _ThisActor()
    sys.modules["simgrid"] = sg
    return sg


_counter = 0


def load_reference(fname: str):
    """Load one reference script as a fresh module (fresh `global_values`)."""
    global _counter
    sg = _install_stub()
    _counter += 1
    path = os.path.join(REF, fname)
    spec = importlib.util.spec_from_file_location(f"_fu_ref_{_counter}", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, sg


# ----------------------------------------------------------------------------------------
# Generation-synchronous collect-all driver
# ----------------------------------------------------------------------------------------
def ca_sync(rowptr, col, values, rounds, seed):
    """Run the reference collect-all Peers generation-synchronously.

    Round 0 is the timeout fire on zero state (CA:87-91 -> CA:105-128). Round r >= 1 fires
    inside `on_receive` once every neighbour has been heard (CA:102-103).
    Returns {r: (last_avg[n], flows[E])} for every r in `rounds` (r = index of the last
    round run, so r = 0 means one round).
    """
    mod, sg = load_reference(CA_FILE)
    n = len(values)
    names = [f"n{i}" for i in range(n)]
    idx = {nm: i for i, nm in enumerate(names)}
    outbox = []
    World.router = lambda dst, p, size: outbox.append((dst, p))
    peers = []
    for i in range(n):
        World.current_host = names[i]
        neigh = ",".join(names[c] for c in col[rowptr[i]:rowptr[i + 1]])
        peers.append(mod.Peer(repr(float(values[i])), neigh))
    rng = np.random.default_rng(seed)
    out = {}
    want = set(rounds)
    last = max(rounds)

    def snap(r):
        la = np.array([peers[i].last_avg for i in range(n)], dtype=np.float64)
        gv = mod.global_values["last_avg"]
        assert all(gv[names[i]] == la[i] or (gv[names[i]] != gv[names[i]]) for i in range(n))
        fl = np.zeros(len(col), dtype=np.float64)
        for i in range(n):
            for e in range(rowptr[i], rowptr[i + 1]):
                fl[e] = peers[i].flows[names[col[e]]]
        out[r] = (la, fl)

    for i in rng.permutation(n):
        peers[i].avg_and_send()
    if 0 in want:
        snap(0)
    for r in range(1, last + 1):
        msgs = outbox[:]
        outbox.clear()
        order = rng.permutation(len(msgs))
        for k in order:
            dst, p = msgs[k]
            peers[idx[dst]].on_receive(p)
        # every non-isolated node fired exactly once in this generation
        assert len(outbox) == len(msgs), (len(outbox), len(msgs))
        if r in want:
            snap(r)
    return out


# ----------------------------------------------------------------------------------------
# The rules of the lossy, pair and churn engines, run through the reference's Peers
# ----------------------------------------------------------------------------------------
def _peers(mod, rowptr, col, values):
    """(names, idx, peers, slot_of): one reference Peer per row, its neighbours in row order;
    slot_of[(i, j)] is the slot of row i that holds neighbour j."""
    n = len(values)
    names = [f"n{i}" for i in range(n)]
    idx = {nm: i for i, nm in enumerate(names)}
    peers, slot_of = [], {}
    for i in range(n):
        World.current_host = names[i]
        row = [int(c) for c in col[rowptr[i]:rowptr[i + 1]]]
        peers.append(mod.Peer(repr(float(values[i])), ",".join(names[c] for c in row)))
        for q, c in enumerate(row):
            slot_of[(i, c)] = int(rowptr[i]) + q
    return names, idx, peers, slot_of


def _slot_snapshot(peers, names, rowptr, col, attr):
    """float64[E]: peers[i].<attr>[neighbour] per slot; 0.0 where the peer does not hold that
    neighbour (nothing is inserted into the peer's dicts)."""
    out = np.zeros(len(col), dtype=np.float64)
    for i, p in enumerate(peers):
        d = getattr(p, attr)
        for k in range(rowptr[i], rowptr[i + 1]):
            nm = names[col[k]]
            if nm in p.neighbors:
                out[k] = d.get(nm, 0.0)
    return out


def _ca_generation(mod, peers, idx, outbox, deliver, driven, rng):
    """One collect-all generation on the reference's own methods. The held messages (`outbox`,
    emptied here) for which deliver(sender, receiver) holds go through `on_receive` in a shuffled
    order; a peer that has then heard all its neighbours fires inside it (CA:102-103). Every
    driven peer that has not fired then gets `tick()` until it fires, TICK_TIMEOUT calls
    (CA:87-91). What the peers send is left in `outbox` for the next generation. Asserts that
    every driven peer fired exactly once and nobody else did."""
    held = [(dst, p) for dst, p in outbox if deliver(idx[p.sender], idx[dst])]
    outbox.clear()
    fired = set()
    for k in rng.permutation(len(held)):
        dst, p = held[k]
        before = len(outbox)
        peers[idx[dst]].on_receive(p)
        if len(outbox) > before:
            assert idx[dst] not in fired
            fired.add(idx[dst])
    for i in driven:
        if i in fired:
            continue
        assert peers[i].ticks_since_last_avg == 0
        calls = 0
        while True:
            peers[i].tick()
            calls += 1
            if peers[i].ticks_since_last_avg == 0:  # avg_and_send ran (CA:128)
                break
            assert calls < mod.Peer.TICK_TIMEOUT
        assert calls == mod.Peer.TICK_TIMEOUT
    sent = {}
    for _, p in outbox:
        sent[p.sender] = sent.get(p.sender, 0) + 1
    want = {peers[i].name: len(peers[i].neighbors) for i in driven if len(peers[i].neighbors)}
    assert sent == want  # one message per neighbour from every driven peer that has one
    assert World.errors == 0


def ca_lossy_sync(rowptr, col, rev, values, delivered, stops, seed):
    """Collect-all generations under loss, on the reference's Peers.

    delivered[r][k] says whether slot k (row i, neighbour j) gets j's message of generation r-1
    in round r; row 0 is ignored: round 0 delivers nothing and every peer fires on its timeout
    (CA:87-91), as in `ca_sync`. A peer that misses a message keeps what it stored for that
    neighbour at its own last fire (CA:117-119) and fires on its timeout.
    Returns {stop: (last_avg[n], flows[E])} after `stop` rounds."""
    mod, sg = load_reference(CA_FILE)
    World.errors = 0
    n = len(values)
    names, idx, peers, slot_of = _peers(mod, rowptr, col, values)
    outbox = []
    World.router = lambda dst, p, size: outbox.append((dst, p))
    rng = np.random.default_rng(seed)
    out = {}
    for r in range(max(stops)):
        D = delivered[r]
        _ca_generation(mod, peers, idx, outbox,
                       (lambda s, d: False) if r == 0 else (lambda s, d: bool(D[rev[slot_of[(s, d)]]])),
                       range(n), rng)
        if r + 1 in stops:
            out[r + 1] = (np.array([p.last_avg for p in peers], dtype=np.float64),
                          _slot_snapshot(peers, names, rowptr, col, "flows"))
    return out


def ca_churn_sync(rowptr, col, values, topologies, stops, seed):
    """Collect-all generations with topology events between rounds, on the reference's Peers.

    topologies: {round: (alive[n], link_up[E])}, applied before that round. Slot k = (i -> j) is
    live iff link_up[k] and alive[i] and alive[j]. At an event every peer's `neighbors` is rebuilt
    as a dict over its live slots IN CSR ROW ORDER, the `flows` and `estimates` entries of dropped
    neighbours are popped (they come back as `defaultdict` zeros, CA:33-34), those of neighbours
    that stayed are left alone, and held messages over a slot that is no longer live are dropped.
    A dead peer has no live slot and is not driven: it keeps its `last_avg`; a revived one finds
    every slot fresh.

    The row-order rebuild is the churn engine's model, not the reference's behaviour: an
    untouched Peer that loses a neighbour by `del` and gets it back at CA:94-96 holds it LAST in
    its dict, and CA:106 / CA:110 then add in that order. Everything else, the arithmetic and
    who fires when, is the reference's: a peer with a fresh neighbour cannot satisfy CA:102, so
    it fires by `tick()` (CA:87-91) on the pairs it received from its other neighbours and the
    `defaultdict` zeros of the fresh one.

    Returns ({stop: (last_avg[n], flows[E])}, {round: (live[E], fresh[E])}): fresh marks the slots
    whose neighbour entry the event created."""
    mod, sg = load_reference(CA_FILE)
    World.errors = 0
    n, E = len(values), len(col)
    names, idx, peers, slot_of = _peers(mod, rowptr, col, values)
    src = np.repeat(np.arange(n), np.diff(rowptr))
    outbox = []
    World.router = lambda dst, p, size: outbox.append((dst, p))
    rng = np.random.default_rng(seed)
    alive = np.ones(n, dtype=bool)
    out, events = {}, {}
    for r in range(max(stops)):
        if r in topologies:
            alive = np.asarray(topologies[r][0]) != 0
            live = (np.asarray(topologies[r][1]) != 0) & alive[src] & alive[col]
            fresh = np.zeros(E, dtype=bool)
            for i, p in enumerate(peers):
                old, new = p.neighbors, {}
                for k in range(rowptr[i], rowptr[i + 1]):
                    if live[k]:
                        nm = names[col[k]]
                        fresh[k] = nm not in old
                        new[nm] = old[nm] if nm in old else sg.Mailbox.by_name(nm)
                for nm in old:
                    if nm not in new:
                        p.flows.pop(nm, None)
                        p.estimates.pop(nm, None)
                        p.msg_recvd_ids.discard(nm)
                p.neighbors = new
            outbox[:] = [(dst, p) for dst, p in outbox if live[slot_of[(idx[p.sender], idx[dst])]]]
            events[r] = (live, fresh)
        _ca_generation(mod, peers, idx, outbox, lambda s, d: True, [int(i) for i in np.flatnonzero(alive)], rng)
        if r + 1 in stops:
            out[r + 1] = (np.array([p.last_avg for p in peers], dtype=np.float64),
                          _slot_snapshot(peers, names, rowptr, col, "flows"))
    return out, events


def _no_fire(*args):
    pass


def pw_sync(rowptr, col, values, mates, initiators, stops, seed):
    """The pairwise exchange over a recorded matching, on the reference's Peers.

    Round r, pair (i, j) with i the initiator: (1) `peers[i].avg_and_send(j)` (PW:102-117), the
    router holds the message; (2) `peers[j].on_receive(msg)` (PW:93-100), which fires back by
    itself; (3) `peers[i].on_receive(answer)`, i's own method, with `avg_and_send` shadowed by a
    no-op instance attribute for that one call: the pair engine's one declared deviation from
    PW:100, where every receive is answered and two peers ping-pong for ever. The pairs of a
    round touch disjoint peers and run in a shuffled order.
    Returns {stop: (last_avg[n], flows[E], estimates[E])} after `stop` rounds."""
    mod, sg = load_reference(PW_FILE)
    World.errors = 0
    names, idx, peers, _ = _peers(mod, rowptr, col, values)
    outbox = []
    World.router = lambda dst, p, size: outbox.append((dst, p))
    rng = np.random.default_rng(seed)
    out = {}
    for r in range(max(stops)):
        sg.Engine.clock = float(r)
        mate, ini = mates[r], initiators[r]
        listeners = [j for j in range(len(values)) if mate[j] >= 0 and not ini[j]]
        for q in rng.permutation(len(listeners)):
            j = listeners[q]
            i = int(mate[j])
            assert ini[i] and mate[i] == j and not outbox
            peers[i].avg_and_send(names[j])
            (dst, msg), = outbox
            outbox.clear()
            assert dst == names[j] and msg.sender == names[i]
            peers[j].on_receive(msg)
            (dst, answer), = outbox
            outbox.clear()
            assert dst == names[i] and answer.sender == names[j]
            peers[i].avg_and_send = _no_fire
            try:
                peers[i].on_receive(answer)
            finally:
                del peers[i].avg_and_send
            assert not outbox and World.errors == 0
        if r + 1 in stops:
            out[r + 1] = (np.array([p.last_avg for p in peers], dtype=np.float64),
                          _slot_snapshot(peers, names, rowptr, col, "flows"),
                          _slot_snapshot(peers, names, rowptr, col, "estimates"))
    return out


# ----------------------------------------------------------------------------------------
# Tick-level emulation of Peer.loop
# ----------------------------------------------------------------------------------------
def tick_emulation(mode, actors, ticks, order, track_flows=False, log_payloads=False):
    """Drive reference Peers through the emulated SimGrid loop for ticks 0..ticks-1.

    actors: list of (host_name, value_str, neighbours_str) in deployment order.
    Returns a dict with per-tick snapshots (after every actor acted at that tick) of
    global_values['last_avg'] (as ordered key/value lists), the event log, the final
    neighbour order per actor, final flows/estimates and fire counts.
    log_payloads adds "recv_payloads": (flow, estimate) of every receive event, in event order.
    """
    mod, sg = load_reference(CA_FILE if mode == "ca" else PW_FILE)
    names = [a[0] for a in actors]
    aidx = {nm: i for i, nm in enumerate(names)}
    n = len(actors)
    peers = []
    World.errors = 0
    for nm, val, neigh in actors:
        World.current_host = nm
        peers.append(mod.Peer(val, neigh))
    fifo = [deque() for _ in range(n)]
    comm = [None] * n  # None | [matched: bool, payload, match_tick]
    events = []  # (tick, actor, kind, other): kind 0 = receive (other = sender), 1 = fire (other = neighbour or -1)
    payloads = []  # (event index, flow, estimate) of every receive
    cur = {"t": 0}

    def router(dst, payload, size):
        d = aidx[dst]
        c = comm[d]
        if c is not None and not c[0]:
            c[0] = True
            c[1] = payload
            c[2] = cur["t"]
        else:
            fifo[d].append(payload)

    World.router = router
    fires = [0] * n

    def wrap(i):
        orig = peers[i].avg_and_send

        def counted(*args):
            fires[i] += 1
            events.append((cur["t"], i, 1, aidx[args[0]] if args else -1))
            return orig(*args)

        peers[i].avg_and_send = counted

    for i in range(n):
        wrap(i)

    snaps_keys = []
    snaps_vals = []
    for t, perm in enumerate(tick_orders(n, order, ticks)):
        cur["t"] = t
        sg.Engine.clock = float(t)
        for i in perm:
            World.current_host = names[i]
            c = comm[i]
            if c is None:
                if fifo[i]:
                    c = [True, fifo[i].popleft(), t]
                else:
                    c = [False, None, -1]
                comm[i] = c
            if c[0] and c[2] < t:
                msg = c[1]
                comm[i] = None
                if type(msg) is mod.FlowUpdatingMsg:
                    payloads.append((len(events), msg.flow, msg.estimate))
                    events.append((t, i, 0, aidx[msg.sender]))
                    peers[i].on_receive(msg)
            peers[i].tick()
        la = mod.global_values["last_avg"]
        snaps_keys.append([aidx[k] for k in la.keys()])
        snaps_vals.append([la[k] for k in la.keys()])
    res = {
        "names": names,
        "values": [mod.global_values["value"][nm] for nm in names],
        "value_keys": [aidx[k] for k in mod.global_values["value"].keys()],
        "snap_keys": snaps_keys,
        "snap_vals": snaps_vals,
        "events": events,
        "fires": fires,
        "neighbors": [[aidx[k] for k in p.neighbors.keys()] for p in peers],
        "flows": [[p.flows[k] for k in p.neighbors.keys()] for p in peers],
        "estimates": [[p.estimates[k] for k in p.neighbors.keys()] for p in peers],
        "errors_logged": World.errors,
        "queued_at_end": [len(q) for q in fifo],
    }
    if log_payloads:
        res["recv_payloads"] = payloads
    return res


# ----------------------------------------------------------------------------------------
# Graphs used for fixtures (the fixture stores the graph, so these need not match the
# product's generators)
# ----------------------------------------------------------------------------------------
def csr_from_pairs(n, pairs, rng=None, shuffle_rows=False):
    adj = [set() for _ in range(n)]
    for u, v in pairs:
        if u == v:
            continue
        adj[u].add(v)
        adj[v].add(u)
    rowptr = [0]
    col = []
    for i in range(n):
        row = sorted(adj[i])
        if shuffle_rows and rng is not None:
            row = list(rng.permutation(row)) if row else []
        col.extend(int(c) for c in row)
        rowptr.append(len(col))
    return np.array(rowptr, dtype=np.int32), np.array(col, dtype=np.int32)


def random_regular_pairs(n, d, rng):
    # configuration model with retries until simple
    while True:
        stubs = np.repeat(np.arange(n), d)
        rng.shuffle(stubs)
        pairs = stubs.reshape(-1, 2)
        if np.any(pairs[:, 0] == pairs[:, 1]):
            continue
        key = np.minimum(pairs[:, 0], pairs[:, 1]) * n + np.maximum(pairs[:, 0], pairs[:, 1])
        if len(np.unique(key)) == len(key):
            return [tuple(map(int, p)) for p in pairs]


def er_pairs(n, m, rng):
    return [(int(rng.integers(n)), int(rng.integers(n))) for _ in range(m)]


def rmat_pairs(scale, ef, rng, abcd=(0.57, 0.19, 0.19, 0.05)):
    n = 1 << scale
    a, b, c, _ = abcd
    pairs = []
    for _ in range(n * ef):
        u = v = 0
        for _lvl in range(scale):
            r = rng.random()
            u <<= 1
            v <<= 1
            if r < a:
                pass
            elif r < a + b:
                v |= 1
            elif r < a + b + c:
                u |= 1
            else:
                u |= 1
                v |= 1
        pairs.append((u, v))
    return n, pairs


def values_for(n, rng, special=False):
    v = rng.random(n) * 100.0
    if special and n >= 8:
        v[0] = -37.25
        v[1] = 1e15 + 0.5
        v[2] = 1e-300
        v[3] = 0.0
        v[4] = 123456789.123456789
    return v


def build_rev(rowptr, col):
    """rev[k] = the slot of row col[k] that points back at k's row."""
    n = len(rowptr) - 1
    pos = {}
    for i in range(n):
        for k in range(rowptr[i], rowptr[i + 1]):
            pos[(i, int(col[k]))] = k
    rev = np.empty(len(col), dtype=np.int32)
    for i in range(n):
        for k in range(rowptr[i], rowptr[i + 1]):
            rev[k] = pos[(int(col[k]), i)]
    return rev


def save_npz(path, **arrays):
    """A compressed .npz whose members carry a fixed timestamp: the same arrays give the same
    bytes on every run (np.savez stamps each member with the time of day)."""
    import io
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def bits(x):
    """float64 array -> its bit patterns (uint64)."""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# The graph and the seeds of the three engine-rule fixtures. The seeds are picked so that the
# conditions of tests/test_engine_rules_golden.py hold on the recorded masks and matchings.
HUB_MIX_SEED = 20251020
LOSS_P, LOSS_SEED, LOSS_ROUNDS, LOSS_STOPS = 0.25, 11, 30, (3, 12, 30)
PAIR_SEED, PAIR_ROUNDS, PAIR_STOPS = 11, 40, (5, 20, 40)
CHURN_ROUNDS, CHURN_STOPS, CHURN_EVENTS = 32, (8, 16, 24, 32), (8, 16, 24)
MAX_FIXTURE_BYTES = 452_000  # no new fixture above the largest one committed before


def hub_mix():
    """(rowptr, col, values): 2400 nodes, rows sorted by id. Node 0 is adjacent to node 1 and to
    nodes 2 .. 2101 (degree 2101: past one 2048-slot chunk and two 1024-slot chunks), node 1 to
    node 0 and to nodes 2 .. 130 (degree 130: above the 128 and 64 light/heavy edges), 1200
    distinct random links among nodes 2 .. 2349, and nodes 2350 .. 2399 are isolated."""
    rng = np.random.default_rng(HUB_MIX_SEED)
    n = 2400
    links = set()
    while len(links) < 1200:
        u, v = (int(x) for x in rng.integers(2, 2350, 2))
        if u != v:
            links.add((min(u, v), max(u, v)))
    pairs = [(0, 1)] + [(0, i) for i in range(2, 2102)] + [(1, i) for i in range(2, 131)] + sorted(links)
    rowptr, col = csr_from_pairs(n, pairs)
    deg = np.diff(rowptr)
    assert len(col) == 6860 and deg[0] == 2101 and deg[1] == 130 and not deg[2350:].any()
    return rowptr, col, rng.random(n) * 100.0


def one_slot_per_link(rev):
    return np.flatnonzero(np.arange(len(rev)) < rev)


def engine_rule_fixtures(manifest):
    """The lossy, pair and churn runs on hub_mix; one .npz each."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "simgrid-flow-updating-implementation_amd"))
    import fu  # host-only helpers: the engines' own loss decision, matching and liveness rule

    rowptr, col, vals = hub_mix()
    rev = build_rev(rowptr, col)
    n, E = len(vals), len(col)
    one = one_slot_per_link(rev)
    graph = {"rowptr": rowptr, "col": col, "rev": rev, "values": bits(vals)}
    manifest["engine_rules"] = {}

    def write(kind, **arrays):
        fn = f"rule_{kind}_hub_mix.npz"
        path = os.path.join(HERE, fn)
        save_npz(path, **graph, **arrays)
        size = os.path.getsize(path)
        assert size <= MAX_FIXTURE_BYTES, (fn, size)
        manifest["engine_rules"][kind] = {"file": fn, "n": int(n), "E": int(E), "max_deg": int(np.diff(rowptr).max())}
        print("engine rule", kind, fn, size, "bytes")

    # ---- lossy: the hash at (p, seed) AND a fixed link-down mask over about 5 % of the links
    rng = np.random.default_rng(HUB_MIX_SEED + 1)
    down = np.zeros(E, dtype=np.uint8)
    cut = one[rng.random(len(one)) < 0.05]
    down[cut] = 1
    down[rev[cut]] = 1
    D = np.stack([fu.lossy_delivered(LOSS_SEED, r, 0, E, LOSS_P).astype(bool) & (down == 0) for r in range(LOSS_ROUNDS)])
    D[0] = False  # round 0 delivers nothing
    res = ca_lossy_sync(rowptr, col, rev, vals, D, LOSS_STOPS, seed=1)
    write("lossy", loss=np.array([LOSS_P]), seed=np.array([LOSS_SEED], dtype=np.int64), down=down,
          delivered=np.packbits(D, axis=1), stops=np.array(LOSS_STOPS, dtype=np.int32),
          last_avg=np.stack([bits(res[s][0]) for s in LOSS_STOPS]), flows=np.stack([bits(res[s][1]) for s in LOSS_STOPS]))

    # ---- pair: the recorded matching of every round
    mm = [fu.pair_matching((rowptr, col), PAIR_SEED, r) for r in range(PAIR_ROUNDS)]
    mates = np.stack([m for m, _ in mm]).astype(np.int32)
    inits = np.stack([i for _, i in mm]).astype(np.uint8)
    res = pw_sync(rowptr, col, vals, mates, inits, PAIR_STOPS, seed=2)
    write("pair", seed=np.array([PAIR_SEED], dtype=np.int64), mate=mates, initiator=inits,
          stops=np.array(PAIR_STOPS, dtype=np.int32), last_avg=np.stack([bits(res[s][0]) for s in PAIR_STOPS]),
          flows=np.stack([bits(res[s][1]) for s in PAIR_STOPS]), estimates=np.stack([bits(res[s][2]) for s in PAIR_STOPS]))

    # ---- churn: all alive for rounds 0-7, events before rounds 8, 16 and 24
    rng = np.random.default_rng(HUB_MIX_SEED + 2)
    row0 = np.arange(rowptr[0], rowptr[1])
    edge = row0[[2046, 2047, 2048, len(row0) - 1]]  # both sides of the 2048-slot chunk edge, and the row's last slot
    deg = np.diff(rowptr)
    lonely = int(np.flatnonzero((np.arange(n) >= 2102) & (deg >= 2))[0])  # alive through rounds 8-15 with every link cut
    alive1 = (rng.random(n) >= 0.10).astype(np.uint8)
    alive1[[0, lonely] + [int(c) for c in col[edge]]] = 1
    alive1[1] = 0
    up1 = np.ones(E, dtype=np.uint8)
    cut = np.concatenate([one[rng.random(len(one)) < 0.05], edge, np.arange(rowptr[lonely], rowptr[lonely + 1])])
    up1[cut] = 0
    up1[rev[cut]] = 0
    alive2 = ((rng.random(n) >= 0.10) | (alive1 == 0)).astype(np.uint8)  # the dead of round 8 come back, others die
    alive2[0] = 0
    ones_n, ones_e = np.ones(n, dtype=np.uint8), np.ones(E, dtype=np.uint8)
    topo = {8: (alive1, up1), 16: (alive2, ones_e), 24: (ones_n, ones_e)}
    res, events = ca_churn_sync(rowptr, col, vals, topo, CHURN_STOPS, seed=3)
    events[0] = (np.ones(E, dtype=bool), np.ones(E, dtype=bool))  # before round 0 every neighbour is new
    ev = (0,) + CHURN_EVENTS
    write("churn", event_rounds=np.array(ev, dtype=np.int32),
          alive=np.stack([ones_n] + [topo[r][0] for r in CHURN_EVENTS]), link_up=np.stack([ones_e] + [topo[r][1] for r in CHURN_EVENTS]),
          live=np.stack([events[r][0] for r in ev]).astype(np.uint8), fresh=np.stack([events[r][1] for r in ev]).astype(np.uint8),
          stops=np.array(CHURN_STOPS, dtype=np.int32), last_avg=np.stack([bits(res[s][0]) for s in CHURN_STOPS]),
          flows=np.stack([bits(res[s][1]) for s in CHURN_STOPS]))


# ----------------------------------------------------------------------------------------
# The fp64 value domain: signed zeros, subnormals, overflow order, NaN placement
# ----------------------------------------------------------------------------------------
VD_SEED = 20261020
VD_ROUNDS = (0, 2, 7, 16)  # round key r = index of the last round run: r + 1 rounds, as in ca_sync_*.npz
VD_CA_FAMILIES = ("subn", "huge", "wide", "special", "special_off")
VD_RULE_FAMILIES = ("subn", "special")
VD_TICKS, VD_TICK_ORDER = 120, "rand:11"
NEG_ZERO = np.uint64(1 << 63)


def components(rowptr, col):
    """Component label (the smallest node id of the component) per node."""
    n = len(rowptr) - 1
    lab = np.full(n, -1, dtype=np.int64)
    for s in range(n):
        if lab[s] >= 0:
            continue
        lab[s] = s
        todo = [s]
        while todo:
            i = todo.pop()
            for c in col[rowptr[i]:rowptr[i + 1]]:
                if lab[c] < 0:
                    lab[c] = s
                    todo.append(int(c))
    return lab


def vd_counts(x):
    """[-0.0, +inf, -inf, NaN] counts of a float64 array."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return [int((x.view(np.uint64) == NEG_ZERO).sum()), int(np.isposinf(x).sum()), int(np.isneginf(x).sum()),
            int(np.isnan(x).sum())]


def vd_hub_leaf(rowptr, col, churn_alive):
    """The first node adjacent to node 0 alone that the churn fixture kills before round 8: its
    one slot is down in rounds 8-23 and FRESH before round 24."""
    deg = np.diff(rowptr)
    for i in range(131, 2102):
        if deg[i] == 1 and col[rowptr[i]] == 0 and churn_alive[1][i] == 0:
            return i
    raise AssertionError("no dead hub leaf")


def vd_values(family, rowptr, col, churn_alive):
    """(values[n], planted[]) of a family on hub_mix. planted: the nodes whose input the family
    sets by hand (special, special_off), or whose input is a zero (subn); empty otherwise.

    special: uniform [0, 100) with -0.0, +inf, -inf and NaN on the four nodes of the two two-node
    components outside node 0's (-0.0 beside +inf, -inf beside NaN), -0.0, 5e-324, -5e-324, +inf and NaN on the
    isolated nodes 2350 .. 2354, and +inf on a node whose only neighbour is node 0. special_off is
    special without that last +inf: nothing non-finite in node 0's component."""
    n = len(rowptr) - 1
    k = ("subn", "huge", "wide", "special").index("special" if family == "special_off" else family)
    rng = np.random.default_rng(VD_SEED + k)
    none = np.zeros(0, dtype=np.int32)
    if family == "subn":
        m = rng.integers(-50, 50, n)
        v = m * 5e-324
        zeros = np.flatnonzero(m == 0)
        v[zeros[::2]] = -0.0
        return v, zeros.astype(np.int32)
    if family == "huge":
        return rng.uniform(-1.0, 1.0, n) * 1.7e308, none
    if family == "wide":
        return rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(-60.0, 60.0, n), none
    v = rng.random(n) * 100.0
    lab = components(rowptr, col)
    deg = np.diff(rowptr)
    small = sorted((int(i) for i in range(n) if lab[i] != lab[0] and deg[i] >= 1), key=lambda i: (lab[i], i))
    assert len(small) == 4 and not deg[2350:2355].any()  # hub_mix has two such components, of two nodes each
    planted = {}
    for i, x in zip(small, (-0.0, np.inf, -np.inf, np.nan)):
        planted[i] = x
    for i, x in zip(range(2350, 2355), (-0.0, 5e-324, -5e-324, np.inf, np.nan)):
        planted[i] = x
    if family == "special":
        planted[vd_hub_leaf(rowptr, col, churn_alive)] = np.inf
    for i, x in planted.items():
        v[i] = x
    return v, np.array(sorted(planted), dtype=np.int32)


def vd_check_ca(family, rowptr, col, v, planted, la, fl):
    """The conditions on the reference's output that tests/test_value_domain_golden.py asserts
    again from the files. la[stop][n], fl[stop][E] in the order of VD_ROUNDS."""
    if family == "subn":
        assert vd_counts(la[-1])[0] >= 1 and vd_counts(fl[-1])[0] >= 1, "subn: no -0.0 at the last stop"
    elif family == "huge":
        assert np.isposinf(fl).any() and np.isneginf(fl).any() and np.isnan(la).any(), "huge: no +-inf flow or NaN estimate"
    elif family in ("special", "special_off"):
        assert np.isnan(la[-1]).any(), "special: no NaN at the last stop"
        iso = [int(i) for i in planted if rowptr[i] == rowptr[i + 1] and bits(v[i:i + 1])[0] == NEG_ZERO]
        assert iso, "special: no isolated node with input -0.0"
        if family == "special":
            leaf = [int(i) for i in planted if rowptr[i + 1] - rowptr[i] == 1 and col[rowptr[i]] == 0]
            assert leaf and np.isposinf(v[leaf[0]]) and not np.isfinite(la[1:, 0]).any() and np.isfinite(la[0, 0]), \
                "special: the hub-leaf inf does not reach row 0"
        else:
            assert np.isfinite(la[-1]).sum() >= 1000, "special_off: fewer than 1000 finite estimates at the last stop"


def value_domain_fixtures(manifest):
    """Signed zeros, subnormals, overflow and non-finite inputs through every driver above, on the
    graphs, masks, matchings and topologies of the fixtures written before. Every float array is
    stored as uint64 bit patterns, inputs included."""
    rule = {k: np.load(os.path.join(HERE, manifest["engine_rules"][k]["file"])) for k in ("lossy", "pair", "churn")}
    rowptr, col, rev = (rule["lossy"][k] for k in ("rowptr", "col", "rev"))
    n, E = len(rowptr) - 1, len(col)
    churn_alive = rule["churn"]["alive"]
    out = manifest["value_domain"] = {"rounds_key": "ca files: rounds[k] = r is the state after r + 1 rounds; rule files: "
                                      "stops[k] = s is the state after s rounds, as in the rule file",
                                      "counts": "[-0.0, +inf, -inf, NaN] in the reference's estimates / flows per stop",
                                      "ca": {}, "rule": {}, "tick": {}}

    def write(fn, **arrays):
        path = os.path.join(HERE, fn)
        save_npz(path, **arrays)
        size = os.path.getsize(path)
        assert size <= MAX_FIXTURE_BYTES, (fn, size)
        print("value domain", fn, size, "bytes")

    def counts(stops, la, fl):
        return {str(int(s)): {"estimates": vd_counts(la[q]), "flows": vd_counts(fl[q])} for q, s in enumerate(stops)}

    # ---- collect-all: one file per family
    for family in VD_CA_FAMILIES:
        v, planted = vd_values(family, rowptr, col, churn_alive)
        res = ca_sync(rowptr, col, v, VD_ROUNDS, seed=VD_SEED)
        la = np.stack([res[r][0] for r in VD_ROUNDS])
        fl = np.stack([res[r][1] for r in VD_ROUNDS])
        vd_check_ca(family, rowptr, col, v, planted, la, fl)
        fn = f"vd_ca_{family}_hub_mix.npz"
        write(fn, values=bits(v), planted=planted, rounds=np.array(VD_ROUNDS, dtype=np.int32), last_avg=bits(la), flows=bits(fl))
        out["ca"][family] = {"file": fn, "graph": manifest["engine_rules"]["lossy"]["file"], "counts": counts(VD_ROUNDS, la, fl)}

    # ---- the lossy, pair and churn rules on the recorded masks, matchings and topologies
    src = np.repeat(np.arange(n), np.diff(rowptr))
    for family in VD_RULE_FAMILIES:
        v, planted = vd_values(family, rowptr, col, churn_alive)
        isp = np.zeros(n, dtype=bool)
        isp[planted] = True

        d = rule["lossy"]
        stops = tuple(int(s) for s in d["stops"])
        D = np.unpackbits(d["delivered"], axis=1)[:, :E].astype(bool)
        res = ca_lossy_sync(rowptr, col, rev, v, D, stops, seed=1)
        la, fl = np.stack([res[s][0] for s in stops]), np.stack([res[s][1] for s in stops])
        odd = (bits(fl) == NEG_ZERO) | ~np.isfinite(fl)
        assert any((odd[q] & ~D[s]).any() for q, s in enumerate(stops[:-1])), "lossy: no loss on a -0.0 or non-finite stored flow"
        fn = f"vd_lossy_{family}_hub_mix.npz"
        write(fn, values=bits(v), planted=planted, stops=d["stops"], last_avg=bits(la), flows=bits(fl))
        out["rule"][f"lossy_{family}"] = {"file": fn, "rule": manifest["engine_rules"]["lossy"]["file"], "counts": counts(stops, la, fl)}

        d = rule["pair"]
        stops = tuple(int(s) for s in d["stops"])
        res = pw_sync(rowptr, col, v, d["mate"], d["initiator"], stops, seed=2)
        la, fl, es = (np.stack([res[s][k] for s in stops]) for k in range(3))
        assert (d["mate"][:, planted] >= 0).any() and (d["mate"] < 0).all(axis=0).any(), "pair: no planted pair or no never-fired node"
        fn = f"vd_pair_{family}_hub_mix.npz"
        write(fn, values=bits(v), planted=planted, stops=d["stops"], last_avg=bits(la), flows=bits(fl), estimates=bits(es))
        out["rule"][f"pair_{family}"] = {"file": fn, "rule": manifest["engine_rules"]["pair"]["file"], "counts": counts(stops, la, fl)}

        d = rule["churn"]
        stops = tuple(int(s) for s in d["stops"])
        ev = [int(r) for r in d["event_rounds"]]
        topo = {r: (d["alive"][e], d["link_up"][e]) for e, r in enumerate(ev) if r > 0}
        res, events = ca_churn_sync(rowptr, col, v, topo, stops, seed=3)
        for e, r in enumerate(ev[1:], 1):
            assert np.array_equal(events[r][0], d["live"][e] != 0) and np.array_equal(events[r][1], d["fresh"][e] != 0)
        la, fl = np.stack([res[s][0] for s in stops]), np.stack([res[s][1] for s in stops])
        fresh = d["fresh"][1:] != 0
        assert (fresh & (isp[src] | isp[col])).any() and (d["alive"][:, planted] == 0).any(), "churn: no FRESH slot or dead node among the planted"
        fn = f"vd_churn_{family}_hub_mix.npz"
        write(fn, values=bits(v), planted=planted, stops=d["stops"], last_avg=bits(la), flows=bits(fl))
        out["rule"][f"churn_{family}"] = {"file": fn, "rule": manifest["engine_rules"]["churn"]["file"], "counts": counts(stops, la, fl)}

    # ---- tick level: the actors of the asym12 and rr32_d4 fixtures with planted values
    plant = {"asym12": {2: -0.0, 5: np.inf, 7: 5e-324, 9: np.nan, 11: -5e-324},
             "rr32_d4": {3: -0.0, 8: np.inf, 13: 5e-324, 19: np.nan, 24: -5e-324, 29: -np.inf}}
    for gname in ("asym12", "rr32_d4"):
        for mode in ("ca", "pw"):
            with open(os.path.join(HERE, manifest["tick"][f"{gname}_{mode}_rand11"])) as f:
                actors = [tuple(a) for a in json.load(f)["actors"]]
            names = [a[0] for a in actors]
            aidx = {nm: i for i, nm in enumerate(names)}
            actors = [(nm, repr(float(plant[gname][i])) if i in plant[gname] else val, neigh) for i, (nm, val, neigh) in enumerate(actors)]
            planted = np.array(sorted(plant[gname]), dtype=np.int32)
            res = tick_emulation(mode, actors, VD_TICKS, VD_TICK_ORDER, log_payloads=True)
            na = len(actors)
            decl = [[aidx[x] for x in a[2].split(",")] if a[2] else [] for a in actors]
            keys = res["snap_keys"]
            assert all(keys[t] == keys[-1][:len(keys[t])] for t in range(VD_TICKS))  # a dict: keys only join, at the end
            snaps = np.zeros((VD_TICKS, na), dtype=np.float64)
            for t in range(VD_TICKS):
                snaps[t, keys[t]] = res["snap_vals"][t]
            seen, dyn, dyn_pay = set(), [], []
            for q, fl_, es_ in res["recv_payloads"]:
                t, i, _, s = res["events"][q]
                if s not in decl[i] and (i, s) not in seen:  # CA:94-96 / PW:94-96: the sender joins i's neighbours
                    seen.add((i, s))
                    dyn.append((t, i, s))
                    dyn_pay.append((fl_, es_))
            assert len(dyn) == res["errors_logged"]
            if gname == "asym12":
                assert any(s in plant[gname] and not (np.isfinite(es_) and abs(es_) >= 2.0 ** -1022) for (_, _, s), (_, es_) in zip(dyn, dyn_pay)), \
                    "tick: no dynamic addition carries a planted value"
            fn = f"vd_tick_{gname}_{mode}.npz"
            write(fn, names=np.array(names), value_strs=np.array([a[1] for a in actors]), values=bits([float(a[1]) for a in actors]),
                  planted=planted, decl_rowptr=np.cumsum([0] + [len(r) for r in decl]).astype(np.int64),
                  decl_col=np.array([c for r in decl for c in r], dtype=np.int32),
                  mode=np.array([mode]), order=np.array([VD_TICK_ORDER]), ticks=np.array([VD_TICKS], dtype=np.int32),
                  key_order=np.array(keys[-1], dtype=np.int32), n_keys=np.array([len(k) for k in keys], dtype=np.int32), snaps=bits(snaps),
                  events=np.array(res["events"], dtype=np.int32).reshape(-1, 4), fires=np.array(res["fires"], dtype=np.int32),
                  union_rowptr=np.cumsum([0] + [len(r) for r in res["neighbors"]]).astype(np.int64),
                  union_col=np.array([c for r in res["neighbors"] for c in r], dtype=np.int32),
                  flows=bits([x for r in res["flows"] for x in r]), estimates=bits([x for r in res["estimates"] for x in r]),
                  dyn=np.array(dyn, dtype=np.int32).reshape(-1, 3), dyn_payload=bits(np.array(dyn_pay, dtype=np.float64).reshape(-1, 2)),
                  errors_logged=np.array([res["errors_logged"]], dtype=np.int32))
            last = np.array([snaps[-1]])
            out["tick"][f"{gname}_{mode}"] = {"file": fn, "actors": manifest["tick"][f"{gname}_{mode}_rand11"],
                                              "counts": {str(VD_TICKS - 1): {"estimates": vd_counts(last), "flows": vd_counts([x for r in res["flows"] for x in r])}}}


# ----------------------------------------------------------------------------------------
# Rows in no ascending order through the reference's Peers (ca_sync_unsorted_*.npz)
# ----------------------------------------------------------------------------------------
ROW_ORDER_SEED = 20261020
ROW_ORDER_ROUNDS = [0, 1, 2, 4, 9, 29]  # six stops: the R-MAT file stays below ca_sync_rmat9_ef8.npz's size


def row_order_fixtures(manifest):
    """Two more collect-all recordings whose rows are shuffled (csr_from_pairs(...,
    shuffle_rows=True)), so that the Peers' neighbour dicts, and with them the sums of CA:106 and
    CA:110, run in an order that is not ascending on rows of up to 257 neighbours: the graph of
    ca_sync_rmat9_ef8.npz (read back from that file) and a star with a centre of 257 leaves. The
    stage has an rng of its own and writes only its own two files and their manifest entries;
    `--only-row-order` runs it alone. The names sort after every earlier ca_sync name: the tests
    parametrised over the sorted manifest carry a fixture's position in their ids, and the earlier
    fixtures keep theirs."""
    rng = np.random.default_rng(ROW_ORDER_SEED)
    with np.load(os.path.join(HERE, "ca_sync_rmat9_ef8.npz")) as d:
        rp, c = d["rowptr"].astype(np.int64), d["col"].astype(np.int64)
    src = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    graphs = {"unsorted_rmat9_ef8": (len(rp) - 1, [(int(u), int(v)) for u, v in zip(src, c) if u < v]),
              "unsorted_star_257": (258, [(0, i) for i in range(1, 258)])}
    for name, (gn, pairs) in graphs.items():
        rowptr, col = csr_from_pairs(gn, pairs, rng, shuffle_rows=True)
        deg = np.diff(rowptr)
        assert any(list(col[rowptr[i]:rowptr[i + 1]]) != sorted(col[rowptr[i]:rowptr[i + 1]])
                   for i in np.flatnonzero(deg == deg.max()))
        vals = values_for(gn, rng)
        res = ca_sync(rowptr, col, vals, ROW_ORDER_ROUNDS, seed=int(rng.integers(1 << 31)))
        fn = f"ca_sync_{name}.npz"
        save_npz(os.path.join(HERE, fn), rowptr=rowptr, col=col, values=vals,
                 rounds=np.array(ROW_ORDER_ROUNDS, dtype=np.int32),
                 last_avg=np.stack([res[r][0] for r in ROW_ORDER_ROUNDS]),
                 flows=np.stack([res[r][1] for r in ROW_ORDER_ROUNDS]))
        manifest["ca_sync"][name] = {"file": fn, "n": int(gn), "E": int(len(col)), "max_deg": int(deg.max())}
        print("ca_sync", name, gn, len(col))


def parse_actors_xml(path):
    import xml.etree.ElementTree as ET

    root = ET.parse(path).getroot()
    out = []
    for a in root.iter("actor"):
        args = [x.get("value") for x in a.findall("argument")]
        out.append((a.get("host"), args[0], args[1] if len(args) > 1 else ""))
    return out


def platform_summary():
    """Hosts / links / routes of the reference platform (PLAT:4-193) as a JSON fixture, so
    tests can rebuild an equivalent platform without the reference tree."""
    import xml.etree.ElementTree as ET

    root = ET.parse(os.path.join(REF, "platforms", "small_platform.xml")).getroot()
    zone = next(root.iter("zone"))
    out = {
        "routing": zone.get("routing"),
        "hosts": [[h.get("id"), h.get("speed")] for h in root.iter("host")],
        "links": [[ln.get("id"), ln.get("bandwidth"), ln.get("latency"), ln.get("sharing_policy")]
                  for ln in root.iter("link")],
        "routes": [[r.get("src"), r.get("dst"), [c.get("id") for c in r.findall("link_ctn")]]
                   for r in root.iter("route")],
    }
    with open(os.path.join(HERE, "small_platform_summary.json"), "w") as f:
        json.dump(out, f, indent=0)


def main():
    if not os.path.isfile(os.path.join(REF, CA_FILE)):
        print(f"make_golden: reference not found at {REF}; nothing to do")
        return 0
    if sys.version_info >= (3, 12):
        # CA:106 / PW:103 add with the builtin sum, which compensates float sums from 3.12 on and
        # no longer equals the left-to-right chain that the fixtures pin.
        print("make_golden: the fixtures pin the reference under CPython < 3.12 (sum() over floats is "
              f"compensated from 3.12 on); this is {sys.version.split()[0]}: nothing written")
        return 2
    only = [(flag, stage) for flag, stage in (("--only-value-domain", value_domain_fixtures),
                                              ("--only-row-order", row_order_fixtures)) if flag in sys.argv]
    if only:  # one of the last stages alone, on the manifest and files of the earlier ones
        with open(os.path.join(HERE, "MANIFEST.json")) as f:
            manifest = json.load(f)
        for _, stage in only:
            stage(manifest)
        with open(os.path.join(HERE, "MANIFEST.json"), "w") as f:
            json.dump(manifest, f, indent=1)
        return 0
    platform_summary()
    if "--only-platform" in sys.argv:
        return 0
    rng = np.random.default_rng(20250629)

    # ---------------- generation-synchronous collect-all ----------------
    graphs = {}
    n = 64
    graphs["rr64_d4"] = (n, random_regular_pairs(n, 4, rng), False)
    graphs["rr256_d8_shuffled"] = (256, random_regular_pairs(256, 8, rng), True)
    graphs["er300_m450"] = (300, er_pairs(300, 450, rng), False)  # isolated nodes + small comps
    graphs["star_257"] = (258, [(0, i) for i in range(1, 258)], False)  # hub deg 257 > wave
    graphs["star_1500"] = (1501, [(0, i) for i in range(1, 1501)], False)  # hub deg 1500
    graphs["k8"] = (8, [(i, j) for i in range(8) for j in range(i + 1, 8)], False)
    graphs["path40"] = (40, [(i, i + 1) for i in range(39)], False)
    ns, rp = rmat_pairs(9, 8, rng)
    graphs["rmat9_ef8"] = (ns, rp, False)
    rounds = [0, 1, 2, 4, 9, 29, 59]
    manifest = {"python": sys.version, "ca_sync": {}, "tick": {}}
    for name, (gn, pairs, shuf) in graphs.items():
        rowptr, col = csr_from_pairs(gn, pairs, rng, shuffle_rows=shuf)
        vals = values_for(gn, rng, special=(name == "rr64_d4"))
        res = ca_sync(rowptr, col, vals, rounds, seed=int(rng.integers(1 << 31)))
        la = np.stack([res[r][0] for r in rounds])
        fl = np.stack([res[r][1] for r in rounds])
        fn = f"ca_sync_{name}.npz"
        np.savez_compressed(os.path.join(HERE, fn), rowptr=rowptr, col=col, values=vals,
                            rounds=np.array(rounds, dtype=np.int32), last_avg=la, flows=fl)
        manifest["ca_sync"][name] = {"file": fn, "n": int(gn), "E": int(len(col)),
                                     "max_deg": int(np.diff(rowptr).max())}
        print("ca_sync", name, gn, len(col))

    # ---------------- tick-level emulation ----------------
    actors = parse_actors_xml(os.path.join(REF, "actors.xml"))
    for mode in ("ca", "pw"):
        for order in ("fwd", "rev", "rand:7"):
            res = tick_emulation(mode, actors, 1001, order)
            tag = order.replace(":", "")
            fn = f"tick_small_platform_{mode}_{tag}.json"
            with open(os.path.join(HERE, fn), "w") as f:
                json.dump({"mode": mode, "order": order, "ticks": 1001, "actors": actors, **res}, f)
            manifest["tick"][f"small_platform_{mode}_{tag}"] = fn
            print("tick", mode, order, "fires", res["fires"])

    # small random-regular graph and a random asymmetric digraph, both modes
    def actors_from_csr(rowptr, col, vals, prefix="h"):
        return [(f"{prefix}{i}", repr(float(vals[i])),
                 ",".join(f"{prefix}{c}" for c in col[rowptr[i]:rowptr[i + 1]]))
                for i in range(len(vals))]

    rowptr, col = csr_from_pairs(32, random_regular_pairs(32, 4, rng), rng, shuffle_rows=True)
    rr_actors = actors_from_csr(rowptr, col, values_for(32, rng))
    # asymmetric: each node declares a random subset of out-neighbours
    na = 12
    asym = []
    avals = values_for(na, rng)
    for i in range(na):
        k = int(rng.integers(0, 4))
        outs = [int(x) for x in rng.choice([j for j in range(na) if j != i], size=k, replace=False)]
        asym.append((f"a{i}", repr(float(avals[i])), ",".join(f"a{j}" for j in outs)))
    for gname, acts, ticks in (("rr32_d4", rr_actors, 400), ("asym12", asym, 400)):
        for mode in ("ca", "pw"):
            for order in ("fwd", "rand:11"):
                res = tick_emulation(mode, acts, ticks, order)
                tag = order.replace(":", "")
                fn = f"tick_{gname}_{mode}_{tag}.json"
                with open(os.path.join(HERE, fn), "w") as f:
                    json.dump({"mode": mode, "order": order, "ticks": ticks, "actors": acts, **res}, f)
                manifest["tick"][f"{gname}_{mode}_{tag}"] = fn
                print("tick", gname, mode, order, "events", len(res["events"]))

    # ---------------- the lossy, pair and churn rules ----------------
    engine_rule_fixtures(manifest)

    # ---------------- the fp64 value domain through every driver ----------------
    value_domain_fixtures(manifest)

    # ---------------- shuffled rows through the collect-all driver ----------------
    row_order_fixtures(manifest)

    with open(os.path.join(HERE, "MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
