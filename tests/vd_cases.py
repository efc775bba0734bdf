"""Shared by the tests of the value-domain fixtures (tests/golden/vd_*.npz, manifest key
"value_domain"): signed zeros, subnormals, overflow and non-finite inputs as the reference's own
Peer methods computed them (tests/golden/make_golden.py: value_domain_fixtures). Reads
tests/golden/ only. Every float in those files is a uint64 bit pattern, inputs included; the
loaders here view them as float64 and derive nothing.

  ca(family)          subn, huge, wide, special, special_off through ca_sync on hub_mix (the graph
                      of rule_cases); stops = rounds completed (the file's round key r is the
                      index of the last round run: stops = r + 1), here 1, 3, 8 and 17.
  rule(kind, family)  lossy, pair, churn with subn and special on the masks, matchings and
                      topologies of rule_cases.load(kind); stops as in that file.
  tick(graph, mode)   asym12, rr32_d4 x ca, pw: 120 ticks in tie order rand:11 with planted values.

special: uniform [0, 100) with -0.0, +inf, -inf, NaN on the four nodes of the two small components
beside node 0's, -0.0, 5e-324, -5e-324, +inf, NaN on five isolated nodes, +inf on one node whose only
neighbour is node 0. That last one makes node 0's whole component (2254 of 2400 nodes) non-finite
from round 2 on, so no run can hold "the inf reaches row 0" and "1000 finite estimates at the last
stop" at once; special_off is special without it and carries the second condition."""
import functools
import types

import numpy as np

import rule_cases
from conftest import load_manifest, load_npz

CA_FAMILIES = ("subn", "huge", "wide", "special", "special_off")
RULE_FAMILIES = ("subn", "special")
RULE_KINDS = ("lossy", "pair", "churn")
TICK_CASES = tuple((g, m) for g in ("asym12", "rr32_d4") for m in ("ca", "pw"))
FLOATS = ("values", "last_avg", "flows", "estimates", "snaps", "dyn_payload")
NEG_ZERO = np.uint64(1 << 63)


def manifest():
    return load_manifest()["value_domain"]


def _load(fn):
    d = load_npz(fn)
    out = {k: d[k] for k in d.files}
    for k in FLOATS:
        if k in out:
            assert out[k].dtype == np.uint64, (fn, k)
            out[k] = out[k].view(np.float64)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ca(family):
    """values[n], planted[], stops (rounds completed), last_avg[stop][n], flows[stop][E] and the
    graph of rule_cases.load("lossy"): rowptr, col, rev, n, E."""
    meta = manifest()["ca"][family]
    g = rule_cases.load("lossy")
    assert meta["graph"] == load_manifest()["engine_rules"]["lossy"]["file"]
    out = _load(meta["file"])
    out["stops"] = [int(r) + 1 for r in out.pop("rounds")]
    return types.SimpleNamespace(family=family, rowptr=g.rowptr, col=g.col, rev=g.rev, n=g.n, E=g.E, **out)


@functools.lru_cache(maxsize=None)
def rule(kind, family):
    """(d, g): d has values, planted, stops, last_avg[stop][n], flows[stop][E] (pair: estimates too);
    g = rule_cases.load(kind), whose masks, matchings or topologies the run went through."""
    meta = manifest()["rule"][f"{kind}_{family}"]
    assert meta["rule"] == load_manifest()["engine_rules"][kind]["file"]
    g = rule_cases.load(kind)
    out = _load(meta["file"])
    out["stops"] = [int(s) for s in out["stops"]]
    assert out["stops"] == g.stops
    return types.SimpleNamespace(kind=kind, family=family, **out), g


@functools.lru_cache(maxsize=None)
def tick(graph, mode):
    """The tick fixture: names, value_strs (repr of the inputs, as a deployment file holds them),
    values, planted, decl_rowptr / decl_col (declared neighbour lists), order, ticks, key_order (the
    final key order of global_values["last_avg"]; at tick t its first n_keys[t] entries exist),
    snaps[tick][n], events (tick, node, kind, other), fires, union_rowptr / union_col (neighbours
    in the peers' final dict order), flows and estimates per union slot, dyn (tick, receiver,
    sender) and dyn_payload (flow, estimate) of every dynamic addition."""
    out = _load(manifest()["tick"][f"{graph}_{mode}"]["file"])
    for k in ("mode", "order"):
        out[k] = str(out[k][0])
    for k in ("ticks", "errors_logged"):
        out[k] = int(out[k][0])
    out["names"] = [str(x) for x in out["names"]]
    out["value_strs"] = [str(x) for x in out["value_strs"]]
    out["n"] = len(out["names"])
    return types.SimpleNamespace(graph=graph, **out)


def tick_trace(d):
    """fu.Trace of a tick fixture's declared lists."""
    import fu

    return fu.Trace(d.decl_rowptr, d.decl_col, "collectall" if d.mode == "ca" else "pairwise", d.ticks, d.order)


def is_neg_zero(x):
    return np.ascontiguousarray(x).view(np.uint64) == NEG_ZERO


def counts(x):
    """[-0.0, +inf, -inf, NaN] counts, the manifest's "counts" entries."""
    x = np.ascontiguousarray(x)
    return [int(is_neg_zero(x).sum()), int(np.isposinf(x).sum()), int(np.isneginf(x).sum()), int(np.isnan(x).sum())]


def py_float_dict(names, x):
    """str() of {name: Python float}, the way the reference prints global_values' entries."""
    return str({nm: float(v) for nm, v in zip(names, x)})
