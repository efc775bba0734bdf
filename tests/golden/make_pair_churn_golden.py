#!/usr/bin/env python3
"""Generate tests/golden/rule_pair_churn_hub_mix.npz: the pairwise exchange while nodes and links
leave and join, as the reference's own Peer methods compute it.

Like make_pair_lossy_golden.py this is test infrastructure: it runs only where the reference
checkout exists (FU_REFERENCE, see make_golden.py), under CPython 3.10 (from 3.12 on the builtin
`sum` of PW:103 is compensated and no longer the left-to-right chain, so nothing is written
there). Nothing in `tests -m gpu`, `smoke()` or `bench.py` runs it, and MANIFEST.json is not
touched. libfu.so must be built: the matchings come from the engine's host-only helper
(`fu.pair_matching` with a topology) and the loss decisions from `fu.pair_lost`; no GPU.

The run: hub_mix (make_golden.hub_mix), 40 rounds under PAIR_SEED, a topology event before
rounds 10, 20 and 30, the state recorded after 10, 20, 30 and 40 rounds:
  10: nodes die, the hub of degree 130 (node 1) among them;
  20: they stay dead and links go down, some of hub 0's among them;
  30: everything comes back.
Slot k = (i -> j) is live iff link_up[k] and alive[i] and alive[j]. At an event every peer's
`neighbors` is rebuilt as a dict over its live slots IN CSR ROW ORDER, and the `flows` and
`estimates` entries of the dropped neighbours are deleted: they come back as the `defaultdict`
zeros (PW:33-34), which is what PW:94-96 leaves for a neighbour it adds. Entries of neighbours
that stayed are left alone. As in make_golden.ca_churn_sync, the row-order rebuild is the
engine's model and not the reference's behaviour: an untouched Peer that loses a neighbour and
gets it back at PW:94-96 holds it LAST in its dict, and PW:103 then adds in that order.
Everything else is the reference's: PW:103 sums over `self.neighbors.keys()`, so a dropped
neighbour is out of the sum.

A pair (i, j), i the initiator, runs as in make_pair_lossy_golden.pw_lossy_sync: (1)
`peers[i].avg_and_send(j)`, (2) `peers[j].on_receive(m1)`, (3) `peers[i].on_receive(m2)` with
`avg_and_send` shadowed by a no-op for that one call (the pair engine's one declared deviation
from PW:100, as in make_golden.pw_sync). The file holds two recordings of the same script: run 0
delivers everything, run 1 drops m1 where lost[r][kt] and m2 where lost[r][ks], `lost` being the
hash at (LOSS_P, LOSS_SEED). Only the recorded arrays go into the file; every float as its bit
pattern.
"""
from __future__ import annotations

import os
import platform
import sys

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden import World, _peers, _slot_snapshot, bits, build_rev, hub_mix, load_reference, save_npz  # noqa: E402

LOSS_P, LOSS_SEED = 0.25, 3
ROUNDS, EVENTS, STOPS = 40, (10, 20, 30), (10, 20, 30, 40)
FILE = "rule_pair_churn_hub_mix.npz"
MAX_BYTES = 1 << 20  # the limit for a committed file


def _no_fire(*args):
    pass


def live_of(rowptr, col, alive, link_up):
    src = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    a = np.asarray(alive) != 0
    return (np.asarray(link_up) != 0) & a[src] & a[col]


def pw_churn_sync(rowptr, col, rev, values, mates, initiators, topologies, lost, stops, seed):
    """{stop: (last_avg[n], flows[E], estimates[E])} after `stop` rounds. topologies: {round:
    (alive, link_up)}, applied before that round. lost: None, or bool[round][E]. The pairs of a
    round touch disjoint peers and run in a shuffled order."""
    mod, sg = load_reference(mg.PW_FILE)
    World.errors = 0
    names, idx, peers, slot_of = _peers(mod, rowptr, col, values)
    outbox = []
    World.router = lambda dst, p, size: outbox.append((dst, p))
    rng = np.random.default_rng(seed)
    live = np.ones(len(col), dtype=bool)
    out = {}
    for r in range(max(stops)):
        sg.Engine.clock = float(r)
        if r in topologies:
            live = live_of(rowptr, col, *topologies[r])
            for i, p in enumerate(peers):
                old, new = p.neighbors, {}
                for k in range(rowptr[i], rowptr[i + 1]):
                    if live[k]:
                        nm = names[col[k]]
                        new[nm] = old[nm] if nm in old else sg.Mailbox.by_name(nm)
                for nm in old:
                    if nm not in new:
                        p.flows.pop(nm, None)
                        p.estimates.pop(nm, None)
                p.neighbors = new
        mate, ini = mates[r], initiators[r]
        listeners = [j for j in range(len(values)) if mate[j] >= 0 and not ini[j]]
        for q in rng.permutation(len(listeners)):
            j = listeners[q]
            i = int(mate[j])
            assert ini[i] and mate[i] == j and not outbox
            ks, kt = slot_of[(i, j)], slot_of[(j, i)]
            assert rev[ks] == kt and live[ks] and live[kt]
            assert names[j] in peers[i].neighbors and names[i] in peers[j].neighbors
            peers[i].avg_and_send(names[j])
            (dst, msg), = outbox
            outbox.clear()
            assert dst == names[j] and msg.sender == names[i]
            if lost is not None and lost[r][kt]:
                continue
            peers[j].on_receive(msg)
            (dst, answer), = outbox
            outbox.clear()
            assert dst == names[i] and answer.sender == names[j]
            if lost is not None and lost[r][ks]:
                continue
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


def topologies_of(rowptr, col, rev):
    """The three events. Rows hold a neighbour once, so a link is one slot and its reverse."""
    n, E = len(rowptr) - 1, len(col)
    rng = np.random.default_rng(mg.HUB_MIX_SEED + 9)
    alive = np.ones(n, dtype=np.uint8)
    alive[1] = 0
    alive[2 + np.flatnonzero(rng.random(n - 2) < 0.1)] = 0
    one = mg.one_slot_per_link(rev)
    cut = one[rng.random(len(one)) < 0.1]
    up = np.ones(E, dtype=np.uint8)
    up[cut] = 0
    up[rev[cut]] = 0
    assert not up[rowptr[0]:rowptr[1]].all()
    return {10: (alive, np.ones(E, dtype=np.uint8)), 20: (alive, up), 30: (np.ones(n, dtype=np.uint8), np.ones(E, dtype=np.uint8))}


def main():
    if sys.version_info[:2] != (3, 10):
        print("make_pair_churn_golden.py: runs under CPython 3.10 only; nothing written")
        return 0
    if not os.path.isdir(mg.REF):
        print("make_pair_churn_golden.py: no reference checkout at", mg.REF, "- nothing written")
        return 0
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "simgrid-flow-updating-implementation_amd"))
    import fu  # host-only helpers: the engine's own matching and loss decision

    rowptr, col, vals = hub_mix()
    rev = build_rev(rowptr, col)
    n, E = len(vals), len(col)
    topo = topologies_of(rowptr, col, rev)
    alive, up = np.ones(n, dtype=np.uint8), np.ones(E, dtype=np.uint8)
    mm = []
    for r in range(ROUNDS):
        if r in topo:
            alive, up = topo[r]
        mm.append(fu.pair_matching((rowptr, col), mg.PAIR_SEED, r, alive=alive, link_up=up))
    mates = np.stack([m for m, _ in mm]).astype(np.int32)
    inits = np.stack([i for _, i in mm]).astype(np.uint8)
    lost = np.stack([fu.pair_lost(LOSS_SEED, r, 0, E, LOSS_P).astype(bool) for r in range(ROUNDS)])
    runs = [pw_churn_sync(rowptr, col, rev, vals, mates, inits, topo, lo, STOPS, seed=5) for lo in (None, lost)]
    for h in (0, 1):
        print("hub", h, "matched in rounds", [r for r in range(ROUNDS) if mates[r][h] >= 0])
    path = os.path.join(HERE, FILE)
    save_npz(path, rowptr=rowptr, col=col, rev=rev, values=bits(vals), p=np.array([LOSS_P]),
             seed=np.array([mg.PAIR_SEED], dtype=np.int64), loss_seed=np.array([LOSS_SEED], dtype=np.int64),
             events=np.array(EVENTS, dtype=np.int32), alive=np.packbits(np.stack([topo[r][0] for r in EVENTS]), axis=1),
             link_up=np.packbits(np.stack([topo[r][1] for r in EVENTS]), axis=1), lost=np.packbits(lost, axis=1),
             mate=mates.astype(np.int16), initiator=np.packbits(inits, axis=1), stops=np.array(STOPS, dtype=np.int32),
             last_avg=np.stack([np.stack([bits(res[s][0]) for s in STOPS]) for res in runs]),
             flows=np.stack([np.stack([bits(res[s][1]) for s in STOPS]) for res in runs]),
             estimates=np.stack([np.stack([bits(res[s][2]) for s in STOPS]) for res in runs]),
             python=np.array(platform.python_version()))
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (FILE, size)
    print(FILE, size, "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
