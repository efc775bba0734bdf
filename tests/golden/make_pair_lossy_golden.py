#!/usr/bin/env python3
"""Generate tests/golden/rule_pair_lossy_hub_mix.npz: the pairwise exchange under message loss as
the reference's own Peer methods compute it.

Like make_golden.py this is test infrastructure: it runs only where the reference checkout
exists (FU_REFERENCE, see make_golden.py), under CPython 3.10 or 3.11; from 3.12 on the builtin
`sum` of PW:103 is compensated and no longer the left-to-right chain, so nothing is written
there. Nothing in `tests -m gpu`, `smoke()` or `bench.py` runs it, and MANIFEST.json is not
touched. libfu.so must be built: the matching and the loss decision come from the engine's
host-only helpers (`fu.pair_matching`, `fu.pair_lost`; no GPU).

The run: hub_mix (make_golden.hub_mix), the recorded matching of PAIR_SEED over 40 rounds, and
per round a `lost` mask over the slots: the hash at (LOSS_P, LOSS_SEED) or a fixed link mask
over about 5 % of the links. A pair (i, j), i the initiator, with m1 received on j's slot kt and
m2 on i's slot ks:
  (1) `peers[i].avg_and_send(j)` (PW:102-117); the router holds m1. If lost[kt], m1 is dropped
      here and the pair is over: j's Peer is never called.
  (2) `peers[j].on_receive(m1)` (PW:93-100), which fires back by itself; the router holds m2. If
      lost[ks], m2 is dropped here: i's Peer is not called again.
  (3) `peers[i].on_receive(m2)` with `avg_and_send` shadowed by a no-op for that one call, as in
      make_golden.pw_sync: the pair engine's one declared deviation from PW:100.
Only the recorded arrays go into the file; every float as its bit pattern.
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
ROUNDS, STOPS = mg.PAIR_ROUNDS, mg.PAIR_STOPS  # 40 rounds, stops 5, 20 and 40
FILE = "rule_pair_lossy_hub_mix.npz"
M1_LOST, M2_LOST, COMPLETE = 0, 1, 2


def _no_fire(*args):
    pass


def pw_lossy_sync(rowptr, col, rev, values, mates, initiators, lost, stops, seed):
    """{stop: (last_avg[n], flows[E], estimates[E])} after `stop` rounds, and the outcome of
    every pair as [(round, i, j, outcome)]. The pairs of a round touch disjoint peers and run in
    a shuffled order."""
    mod, sg = load_reference(mg.PW_FILE)
    World.errors = 0
    names, idx, peers, slot_of = _peers(mod, rowptr, col, values)
    outbox = []
    World.router = lambda dst, p, size: outbox.append((dst, p))
    rng = np.random.default_rng(seed)
    out, seen = {}, []
    for r in range(max(stops)):
        sg.Engine.clock = float(r)
        mate, ini = mates[r], initiators[r]
        listeners = [j for j in range(len(values)) if mate[j] >= 0 and not ini[j]]
        for q in rng.permutation(len(listeners)):
            j = listeners[q]
            i = int(mate[j])
            assert ini[i] and mate[i] == j and not outbox
            ks, kt = slot_of[(i, j)], slot_of[(j, i)]
            assert rev[ks] == kt
            peers[i].avg_and_send(names[j])
            (dst, msg), = outbox
            outbox.clear()
            assert dst == names[j] and msg.sender == names[i]
            if lost[r][kt]:  # m1 is dropped after avg_and_send
                seen.append((r, i, j, M1_LOST))
                continue
            peers[j].on_receive(msg)
            (dst, answer), = outbox
            outbox.clear()
            assert dst == names[i] and answer.sender == names[j]
            if lost[r][ks]:  # m2 is dropped after on_receive
                seen.append((r, i, j, M2_LOST))
                continue
            peers[i].avg_and_send = _no_fire
            try:
                peers[i].on_receive(answer)
            finally:
                del peers[i].avg_and_send
            seen.append((r, i, j, COMPLETE))
            assert not outbox and World.errors == 0
        if r + 1 in stops:
            out[r + 1] = (np.array([p.last_avg for p in peers], dtype=np.float64),
                          _slot_snapshot(peers, names, rowptr, col, "flows"),
                          _slot_snapshot(peers, names, rowptr, col, "estimates"))
    return out, seen


def hub_census(seen):
    """{(node, role): [pairs with m1 lost, with m2 lost, complete]} for nodes 0 and 1."""
    cnt = {(h, role): [0, 0, 0] for h in (0, 1) for role in ("initiator", "listener")}
    for _, i, j, o in seen:
        if i in (0, 1):
            cnt[(i, "initiator")][o] += 1
        if j in (0, 1):
            cnt[(j, "listener")][o] += 1
    return cnt


def main():
    if sys.version_info >= (3, 12):
        print("make_pair_lossy_golden.py: CPython >= 3.12 sums with compensation (PW:103); nothing written")
        return 0
    if not os.path.isdir(mg.REF):
        print("make_pair_lossy_golden.py: no reference checkout at", mg.REF, "- nothing written")
        return 0
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "simgrid-flow-updating-implementation_amd"))
    import fu  # host-only helpers: the engine's own matching and loss decision

    rowptr, col, vals = hub_mix()
    rev = build_rev(rowptr, col)
    E = len(col)
    one = mg.one_slot_per_link(rev)
    rng = np.random.default_rng(mg.HUB_MIX_SEED + 4)
    down = np.zeros(E, dtype=np.uint8)
    cut = one[rng.random(len(one)) < 0.05]
    down[cut] = 1
    down[rev[cut]] = 1
    mm = [fu.pair_matching((rowptr, col), mg.PAIR_SEED, r) for r in range(ROUNDS)]
    mates = np.stack([m for m, _ in mm]).astype(np.int32)
    inits = np.stack([i for _, i in mm]).astype(np.uint8)
    lost = np.stack([fu.pair_lost(LOSS_SEED, r, 0, E, LOSS_P).astype(bool) | (down != 0) for r in range(ROUNDS)])
    res, seen = pw_lossy_sync(rowptr, col, rev, vals, mates, inits, lost, STOPS, seed=5)
    census = hub_census(seen)
    for key, c in sorted(census.items()):
        print("hub", key, "m1 lost / m2 lost / complete:", c)
        assert sum(c) == 0 or min(c) >= 1, (key, c)  # every outcome, wherever the node has the role at all
    total = [sum(1 for s in seen if s[3] == o) for o in (M1_LOST, M2_LOST, COMPLETE)]
    print("pairs with m1 lost / m2 lost / complete:", total)
    path = os.path.join(HERE, FILE)
    save_npz(path, rowptr=rowptr, col=col, rev=rev, values=bits(vals), p=np.array([LOSS_P]),
             seed=np.array([mg.PAIR_SEED], dtype=np.int64), loss_seed=np.array([LOSS_SEED], dtype=np.int64), down=down,
             lost=np.packbits(lost, axis=1), mate=mates, initiator=inits, stops=np.array(STOPS, dtype=np.int32),
             last_avg=np.stack([bits(res[s][0]) for s in STOPS]), flows=np.stack([bits(res[s][1]) for s in STOPS]),
             estimates=np.stack([bits(res[s][2]) for s in STOPS]), python=np.array(platform.python_version()))
    size = os.path.getsize(path)
    assert size <= mg.MAX_FIXTURE_BYTES, (FILE, size)
    print(FILE, size, "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
