"""Shared by the tests of the engine-rule fixtures (tests/golden/rule_*_hub_mix.npz): the lossy,
pair and churn rules as the reference's own Peer methods computed them on the graph hub_mix
(tests/golden/make_golden.py: ca_lossy_sync, pw_sync, ca_churn_sync). Reads tests/golden/ only.

hub_mix: 2400 nodes; node 0 has degree 2101 (past one 2048-slot chunk of kl_heavy / kc_heavy and
two 1024-slot chunks of kp_heavy), node 1 degree 130 (above the 128 and 64 light/heavy edges),
1200 random links among nodes 2 .. 2349, nodes 2350 .. 2399 isolated; E = 6860."""
import functools
import types

import numpy as np

from conftest import load_manifest, load_npz

UP, DOWN, FRESH = 0, 1, 2


@functools.lru_cache(maxsize=None)
def load(kind):
    """The fixture of "lossy", "pair" or "churn" as a namespace of read-only arrays: rowptr, col,
    rev, values, stops (rounds completed), last_avg[stop][n], flows[stop][E] and
      lossy: loss, seed, down[E], delivered[round][E] (bool; row 0 is round 0, all False);
      pair:  seed, mate[round][n], initiator[round][n], estimates[stop][E] (the cache c);
      churn: event_rounds (0, 8, 16, 24), alive[event][n], link_up[event][E], live[event][E] and
             fresh[event][E] (the slots whose neighbour entry the event created)."""
    d = load_npz(load_manifest()["engine_rules"][kind]["file"])
    out = {k: d[k] for k in d.files}
    for k in ("values", "last_avg", "flows", "estimates"):
        if k in out:
            assert out[k].dtype == np.uint64
            out[k] = out[k].view(np.float64)
    out["rowptr"] = out["rowptr"].astype(np.int64)
    out["n"], out["E"] = len(out["rowptr"]) - 1, len(out["col"])
    out["stops"] = [int(s) for s in out["stops"]]
    if kind == "lossy":
        out["delivered"] = np.unpackbits(out["delivered"], axis=1)[:, :out["E"]].astype(bool)
        out["loss"], out["seed"] = float(out["loss"][0]), int(out["seed"][0])
    elif kind == "pair":
        out["seed"] = int(out["seed"][0])
    else:
        out["event_rounds"] = [int(r) for r in out["event_rounds"]]
        out["live"], out["fresh"] = out["live"].astype(bool), out["fresh"].astype(bool)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return types.SimpleNamespace(**out)


def row(d, i):
    """The slots of row i."""
    return np.arange(d.rowptr[i], d.rowptr[i + 1])


def lost_before(d, stop):
    """Messages lost in rounds 1 .. stop-1 of the lossy fixture (round 0 offers none)."""
    return int((~d.delivered[1:stop]).sum())


def churn_script(d, upto):
    """churn_cases.churn_python's script for the first `upto` rounds of the churn fixture."""
    script, done = [], 0
    for e, r in enumerate(d.event_rounds):
        if r >= upto:
            break
        if r > done:
            script.append(("run", r - done))
            done = r
        if r > 0:
            script.append(("topology", d.alive[e], d.link_up[e]))
    script.append(("run", upto - done))
    return script


def churn_states_after_events(d):
    """[state[E]] right after each event of the churn fixture, from its live and fresh masks."""
    return [np.where(d.fresh[e], FRESH, np.where(d.live[e], UP, DOWN)).astype(np.uint8) for e in range(len(d.event_rounds))]
