"""Shared by the value-domain tests of the K-column lossy and churn handles
(fu.CollectAllLossyBatch, fu.CollectAllChurnBatch; csrc/fu_rev_round.h k_light_cols, k_heavy_cols,
k_max_err_cols): the recordings of the reference's Peer code (tests/golden/vd_*.npz through
vd_cases) laid out as the columns of one handle, the Python rules run beside them round by round,
and special values planted at the chunk edges of rev_columns_cases.heavy_boundary_graph(K).
Nothing here runs the engine: a column's reference is its recording, or lossy_cases.lossy_python /
churn_cases.churn_python on that column alone.

kind "ca":     the five families of vd_cases.ca on hub_mix without loss and with everything alive,
               17 rounds, stops 1, 3, 8 and 17;
kind "lossy":  subn and special of vd_cases.rule("lossy", .) under the recorded loss, 30 rounds;
kind "churn":  the same of vd_cases.rule("churn", .) through the recorded topologies, 32 rounds.
A family of None in a layout is a filler column, fu.uniform_values at seed FILL_SEED + column."""
import functools

import numpy as np

import fu
import rule_cases
import vd_cases
from churn_cases import churn_python
from lossy_cases import lossy_python
from parity_util import FAMILIES
from rev_columns_cases import (chunk_slots, churn_reference, heavy_boundary_graph, heavy_boundary_script,
                               lossy_reference)
from vd_cases import CA_FAMILIES, RULE_FAMILIES

FILL_SEED = 200
ENGINES = ("lossy", "churn")

# The layouts of the lossless runs. K = 16: the families three times, in three orders, around one
# filler column.
CA_LAYOUTS = {
    "k5": CA_FAMILIES,
    "k2-huge-special": ("huge", "special"),
    "k2-subn-special_off": ("subn", "special_off"),
    "k3": ("special", None, "subn"),
    "k16": CA_FAMILIES + CA_FAMILIES[::-1] + (None,) + ("wide", "special_off", "subn", "special", "huge"),
}
# The layouts under the recorded loss and topologies: (K, place) of vd_columns.
RULE_LAYOUTS = {"k2": (2, "first"), "k3-first": (3, "first"), "k16-first": (16, "first"), "k16-last": (16, "last")}
ERR_SPEC = ("special", None, "subn")  # the columns of the error reduction cases


def graph(kind):
    """The recording that holds the graph (and the masks or topologies) of `kind`."""
    return rule_cases.load("lossy" if kind == "ca" else kind)


def fixture(kind, family):
    """The recording of `family`: values, stops, last_avg[stop][n], flows[stop][E]."""
    return vd_cases.ca(family) if kind == "ca" else vd_cases.rule(kind, family)[0]


def stops(kind):
    return fixture(kind, "subn").stops


def column_values(kind, name):
    """The inputs of a column: a family of `kind`, or fu.uniform_values at the seed `name`."""
    if isinstance(name, int):
        return fu.uniform_values(graph(kind).n, seed=name)
    return fixture(kind, name).values


@functools.lru_cache(maxsize=None)
def layout(kind, spec):
    """(V (n, K), {column: family}) for a tuple of families, None = a filler column."""
    V = np.stack([column_values(kind, FILL_SEED + c if f is None else f) for c, f in enumerate(spec)], axis=1)
    V = np.ascontiguousarray(V)
    V.setflags(write=False)
    return V, {c: f for c, f in enumerate(spec) if f is not None}


def vd_columns(kind, K, place):
    """(V (n, K), {column: family}): the families of `kind` (CA_FAMILIES for "ca", RULE_FAMILIES
    for "lossy" and "churn") in K columns, "first": from column 0 up in the families' order,
    "last": ending at column K - 1 in reverse order (the first family in column K - 1); filler
    columns take the rest."""
    fams = CA_FAMILIES if kind == "ca" else RULE_FAMILIES
    assert K >= len(fams) and place in ("first", "last")
    fill = (None,) * (K - len(fams))
    return layout(kind, fams + fill if place == "first" else fill + fams[::-1])


def fill_name(c):
    return FILL_SEED + c


@functools.lru_cache(maxsize=None)
def reference_rounds(engine, kind, name):
    """[(a, f)] after every round of the Python rule of `engine` on one column (`name`: a family
    or a filler's seed). kind "ca": every message delivered / everything alive, 17 rounds; kind
    = engine: the recorded `delivered` masks (30 rounds) or the recorded topologies (32)."""
    assert engine in ENGINES and kind in ("ca", engine)
    g = graph(kind)
    v = column_values(kind, name)
    rounds = stops(kind)[-1]
    if engine == "lossy":
        everything = np.ones(g.E, dtype=bool)
        out = []
        lossy_python(g.rowptr, g.col, g.rev, v, rounds, (lambda r: everything) if kind == "ca" else (lambda r: g.delivered[r]),
                     keep=out)
    else:
        script = [("run", rounds)] if kind == "ca" else rule_cases.churn_script(g, rounds)
        res = churn_python(g.rowptr, g.col, g.rev, v, script)
        out = list(zip(res.a_rounds, res.f_rounds))
    assert len(out) == rounds
    for a, f in out:
        a.setflags(write=False)
        f.setflags(write=False)
    return out


def wanted(engine, kind, fams, c, q):
    """(a, f) that column c must hold after stop q: the recording for a family column, the Python
    rule for a filler."""
    if c in fams:
        d = fixture(kind, fams[c])
        return d.last_avg[q], d.flows[q]
    return reference_rounds(engine, kind, fill_name(c))[stops(kind)[q] - 1]


def alive_in_round(r):
    """bool[n]: the alive nodes of round r of the churn recording."""
    g = graph("churn")
    e = max(q for q, first in enumerate(g.event_rounds) if first <= r)
    return np.asarray(g.alive[e]) != 0


@functools.lru_cache(maxsize=None)
def error_case(engine):
    """(V, target (n, 3), want (rounds, 3), the rule's estimates (rounds, n, 3)) of the error
    reduction at the columns ERR_SPEC under the recorded loss or topologies. The targets are the
    reference's estimates of the last stop (the recording's; the Python rule's for the filler);
    in the `special` column a non-finite one is replaced by 0.0, so that an entry of the trace is
    NaN because an estimate of that round is and not because the target is. want[r] is numpy's
    max |a - target| over the Python rule's estimates of round r (np.max propagates NaN), under
    churn over the nodes alive in round r."""
    V, fams = layout(engine, ERR_SPEC)
    per = [reference_rounds(engine, engine, fams.get(c, fill_name(c))) for c in range(len(ERR_SPEC))]
    rounds = len(per[0])
    a_rounds = np.stack([np.stack([per[c][r][0] for c in range(len(ERR_SPEC))], axis=1) for r in range(rounds)])
    target = a_rounds[-1].copy()
    for c, f in fams.items():
        target[:, c] = fixture(engine, f).last_avg[-1]
    target[~np.isfinite(target)] = 0.0
    want = np.empty((rounds, len(ERR_SPEC)))
    for r in range(rounds):
        on = alive_in_round(r) if engine == "churn" else np.ones(V.shape[0], dtype=bool)
        with np.errstate(invalid="ignore"):
            want[r] = np.max(np.abs(a_rounds[r] - target)[on], axis=0)
    return V, target, want, a_rounds


# ------------------------------------------------------------------------------------
# special values at the chunk edges of heavy_boundary_graph(K)
# ------------------------------------------------------------------------------------
HEAVY_STOPS = (1, 2, 5, 10)
HEAVY_LOSS = 0.5
# K = 2 has no room for subn, huge and the planted column at once: two handles.
HEAVY_LAYOUTS = {
    "k2-subn": (2, ("subn", "planted")),
    "k2-huge": (2, ("huge", "planted")),
    "k3": (3, ("subn", "huge", "planted")),
    "k16": (16, ("subn", "huge") + (None,) * 13 + ("planted",)),
}


@functools.lru_cache(maxsize=None)
def planted_column(K):
    """(v, claims): uniform values with, on every row of heavy_boundary_graph(K) of more than one
    chunk (degree d > ce = 2048 // K), +inf on the neighbour at slot position ce - 1 (the last
    slot of the first chunk), -0.0 on the one at position ce (the first slot of the second chunk)
    and NaN on the one at position d - 1. claims: [(row, position, value)] as they hold in v; on
    the row of degree ce + 1 positions ce and d - 1 are one slot, which carries the NaN."""
    g, rows = heavy_boundary_graph(K)
    ce = chunk_slots(K)
    v = fu.uniform_values(g.n, seed=FILL_SEED + 50)
    claims = []
    for d, h in sorted(rows.items()):
        if d > ce:
            claims.append((h, ce - 1, np.inf))
            if ce != d - 1:
                claims.append((h, ce, -0.0))
    claims += [(h, d - 1, np.nan) for d, h in sorted(rows.items()) if d > ce]
    for h, pos, x in claims:
        v[g.col[g.rowptr[h] + pos]] = x
    v.setflags(write=False)
    return v, claims


@functools.lru_cache(maxsize=None)
def heavy_columns(name):
    """(g, V (n, K), spec) of HEAVY_LAYOUTS[name]: parity_util's subn and huge, the planted column
    and filler columns."""
    K, spec = HEAVY_LAYOUTS[name]
    g, _ = heavy_boundary_graph(K)
    cols = []
    for c, f in enumerate(spec):
        if f == "planted":
            cols.append(planted_column(K)[0])
        elif f is None:
            cols.append(fu.uniform_values(g.n, seed=FILL_SEED + c))
        else:
            cols.append(FAMILIES[f](g.n, 4))
    V = np.ascontiguousarray(np.stack(cols, axis=1))
    V.setflags(write=False)
    return g, V, spec


def fillers(spec):
    return [c for c, f in enumerate(spec) if f is None]


@functools.lru_cache(maxsize=None)
def heavy_churn_steps(name):
    """[Step] of heavy_boundary_script(K) on the columns of HEAVY_LAYOUTS[name], churn_python per column."""
    g, V, _ = heavy_columns(name)
    return churn_reference(g, V, heavy_boundary_script(HEAVY_LAYOUTS[name][0])[0])


@functools.lru_cache(maxsize=None)
def heavy_lossy_stops(name):
    """{stop: (a, f)} at p = 0.5 and rev_columns_cases.LOSS_SEED, lossy_python per column."""
    g, V, _ = heavy_columns(name)
    return lossy_reference(g, V, HEAVY_STOPS, HEAVY_LOSS, python=True)
