"""Command line: the two reference scripts as one CLI.

    python -m fu collectall [--platform P] [--deployment D] [--until 1000] [--interval 10]
    python -m fu pairwise   ...
    python -m fu collectall --sync --rounds 200         # synchronous rounds (hot path)
    python -m fu bench-graph er:n=1000000,m=4000000 --rounds 1000
    python -m fu bench-graph er:n=1000000,m=4000000 --rounds 1000 --loss 0.1 [--loss-seed 7]
    python -m fu bench-graph er:n=1000000,m=4000000 --rounds 1000 --pairs [--pair-seed 7]
    python -m fu bench-graph er:n=1000000,m=4000000 --rounds 1000 --pairs --loss 0.1 [--loss-seed 7]
    python -m fu bench-graph er:n=1000000,m=4000000 --rounds 1000 --pairs --pair-columns 4 [--loss 0.1]
    python -m fu bench-graph er:n=1000000,m=4000000 --rounds 1000 --pairs --pair-churn 0.1 [--churn-seed 7]
    python -m fu bench-graph er:n=1000000,m=4000000 --rounds 1000 --churn 0.1 [--churn-seed 7]
    python -m fu bench-graph er:n=1000000,m=4000000 --rounds 1000 --churn 0.1 --columns 4   # or --loss

Defaults mirror flowupdating-collectall.py:154,157 (./platforms/small_platform.xml,
./actors.xml, watcher 1000.0 / 10.0 at CA:162).
"""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from .engine import (CollectAll, CollectAllChurn, CollectAllChurnBatch, CollectAllLossy, CollectAllLossyBatch, PairwiseSync,
                     PairwiseSyncBatch,                      churn_targets)
from .graph import Graph, component_means, uniform_values
from .sim import CollectAllPeer, Engine, run_reference_main


def _columns(n: int, k: int):
    """(n, k) inputs of --columns: column 0 the usual uniform values, column 1 the COUNT
    indicator (node 0 holds 1), every further column c a uniform stream at seed c."""
    cols = [uniform_values(n, seed=0)]
    if k > 1:
        one = np.zeros(n)
        one[0] = 1.0
        cols.append(one)
    cols += [uniform_values(n, seed=c) for c in range(2, k)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def _columns_note(a) -> str:
    return "" if a.columns is None else f" columns={a.columns}"


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m fu")
    ap.add_argument("mode", choices=["collectall", "pairwise", "bench-graph"])
    ap.add_argument("spec", nargs="?", help="graph spec for bench-graph (er:/rr:/rmat:/rgg:)")
    ap.add_argument("--platform", default="./platforms/small_platform.xml")
    ap.add_argument("--deployment", default="./actors.xml")
    ap.add_argument("--until", type=float, default=1000.0)
    ap.add_argument("--interval", type=float, default=10.0)
    ap.add_argument("--order", default="fwd", help="intra-tick actor order: fwd|rev|rand:<seed>")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sync", action="store_true", help="generation-synchronous rounds")
    ap.add_argument("--rounds", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--kernel", default="auto")
    ap.add_argument("--loss", type=float, default=None, help="bench-graph: message loss probability (lossy engine; with --pairs the pair engine)")
    ap.add_argument("--loss-seed", type=int, default=0)
    ap.add_argument("--pairs", action="store_true", help="bench-graph: synchronous pairwise rounds (pair engine)")
    ap.add_argument("--pair-seed", type=int, default=0)
    ap.add_argument("--churn", type=float, default=None,
                    help="bench-graph: fraction of the nodes that dies after half of the rounds (churn engine)")
    ap.add_argument("--churn-seed", type=int, default=0)
    ap.add_argument("--columns", type=int, default=None,
                    help="bench-graph with --loss or --churn: K value columns in one handle (1..16)")
    ap.add_argument("--pair-columns", type=int, default=None,
                    help="bench-graph with --pairs: K value columns over one matching (1..16)")
    ap.add_argument("--pair-churn", type=float, default=None,
                    help="bench-graph with --pairs: fraction of the nodes that dies after half of the rounds (pair engine)")
    a = ap.parse_args(argv)
    if a.pair_churn is not None:
        if a.mode != "bench-graph" or not a.pairs:
            ap.error("--pair-churn needs bench-graph with --pairs")
        if not 0.0 <= a.pair_churn < 1.0:
            ap.error("--pair-churn must be in [0, 1)")
    if a.pair_columns is not None:
        if a.mode != "bench-graph" or not a.pairs:
            ap.error("--pair-columns needs bench-graph with --pairs")
        if not 1 <= a.pair_columns <= 16:
            ap.error("--pair-columns must be in 1..16")
    if a.columns is not None:
        if a.mode != "bench-graph" or (a.loss is None and a.churn is None):
            ap.error("--columns needs bench-graph with --loss or --churn")
        if not 1 <= a.columns <= 16:
            ap.error("--columns must be in 1..16")
    if a.mode == "bench-graph" and a.churn is not None:
        if a.loss is not None or a.pairs:
            ap.error("--churn is exclusive with --loss and --pairs")
        g = Graph.from_spec(a.spec, seed=a.seed)
        if a.columns is None:
            v = uniform_values(g.n, seed=0)
            eng = CollectAllChurn(g, v, device=a.device)
        else:
            v = _columns(g.n, a.columns)
            eng = CollectAllChurnBatch(g, v, device=a.device)
        # node i dies iff U_i < FRACTION, U the fu_values_uniform stream at the churn seed
        alive = ~(uniform_values(g.n, seed=a.churn_seed, lo=0.0, hi=1.0) < a.churn)
        t0 = time.perf_counter()
        ms = eng.run_timed(a.rounds // 2)
        eng.set_topology(alive=alive)
        eng.set_targets(churn_targets(g, v, alive))
        ms += eng.run_timed(a.rounds - a.rounds // 2)
        wall = time.perf_counter() - t0
        print(f"graph n={g.n} E={g.E} max_deg={g.max_deg} rounds={a.rounds} "
              f"device_ms={ms:.3f} wall_s={wall:.3f} edge_updates/s={g.E * a.rounds / (ms / 1e3):.4e} "
              f"max_err={np.max(eng.max_err()):.3e} alive={eng.stats[0]}" + _columns_note(a))
        return 0
    if a.mode == "bench-graph" and a.pairs:
        if a.columns is not None:
            ap.error("--columns needs --loss or --churn without --pairs")
        g = Graph.from_spec(a.spec, seed=a.seed)
        if a.pair_columns is None:
            v = uniform_values(g.n, seed=0)
            eng = PairwiseSync(g, v, seed=a.pair_seed, device=a.device)
        else:
            v = _columns(g.n, a.pair_columns)
            eng = PairwiseSyncBatch(g, v, seed=a.pair_seed, device=a.device)
        if a.loss is not None:
            eng.set_loss(a.loss, a.loss_seed)
        t0 = time.perf_counter()
        if a.pair_churn is None:
            ms = eng.run_timed(a.rounds)
        else:
            # node i dies iff U_i < FRACTION, U the fu_values_uniform stream at the churn seed
            alive = ~(uniform_values(g.n, seed=a.churn_seed, lo=0.0, hi=1.0) < a.pair_churn)
            ms = eng.run_timed(a.rounds // 2)
            eng.set_topology(alive=alive)
            ms += eng.run_timed(a.rounds - a.rounds // 2)
        wall = time.perf_counter() - t0
        if a.pair_churn is not None:
            tgt = churn_targets(g, v, alive)
        elif a.pair_columns is None:
            tgt, _ = component_means(g.rowptr, g.col, v)
        else:
            tgt = churn_targets(g, v)  # everything alive: component_means per column
        eng.set_targets(tgt)
        print(f"graph n={g.n} E={g.E} max_deg={g.max_deg} rounds={a.rounds} "
              f"device_ms={ms:.3f} wall_s={wall:.3f} edge_updates/s={g.E * a.rounds / (ms / 1e3):.4e} "
              f"max_err={np.max(eng.max_err()):.3e} pairs={eng.stats[0]}"
              + ("" if a.pair_churn is None else f" alive={eng.topology_stats[0]}")
              + ("" if a.loss is None else f" lost={sum(eng.loss_stats[:2])}")
              + ("" if a.pair_columns is None else f" columns={a.pair_columns}"))
        return 0
    if a.mode == "bench-graph" and a.loss is not None:
        g = Graph.from_spec(a.spec, seed=a.seed)
        if a.columns is None:
            v = uniform_values(g.n, seed=0)
            eng = CollectAllLossy(g, v, loss=a.loss, seed=a.loss_seed, device=a.device)
        else:
            v = _columns(g.n, a.columns)
            eng = CollectAllLossyBatch(g, v, loss=a.loss, seed=a.loss_seed, device=a.device)
        t0 = time.perf_counter()
        ms = eng.run_timed(a.rounds)
        wall = time.perf_counter() - t0
        eng.set_targets(churn_targets(g, v))  # everything alive: component_means per column
        print(f"graph n={g.n} E={g.E} max_deg={g.max_deg} rounds={a.rounds} "
              f"device_ms={ms:.3f} wall_s={wall:.3f} edge_updates/s={g.E * a.rounds / (ms / 1e3):.4e} "
              f"max_err={np.max(eng.max_err()):.3e} lost={eng.stats[1]}" + _columns_note(a))
        return 0
    if a.mode == "bench-graph":
        g = Graph.from_spec(a.spec, seed=a.seed)
        v = uniform_values(g.n, seed=0)
        eng = CollectAll(g, v, device=a.device, kernel=a.kernel)
        t0 = time.perf_counter()
        ms = eng.run_timed(a.rounds)
        wall = time.perf_counter() - t0
        tgt, _ = component_means(g.rowptr, g.col, v)
        eng.set_targets(tgt)
        print(f"graph n={g.n} E={g.E} max_deg={g.max_deg} rounds={a.rounds} "
              f"device_ms={ms:.3f} wall_s={wall:.3f} edge_updates/s={g.E * a.rounds / (ms / 1e3):.4e} "
              f"max_err={eng.max_err():.3e}")
        return 0
    if a.sync:
        e = Engine([], device=a.device, sync=True)
        e.load_platform(a.platform)
        e.register_actor("peer", CollectAllPeer)
        e.load_deployment(a.deployment)
        e.add_watcher(a.rounds, a.interval)
        e.run_until(a.rounds)
        return 0
    run_reference_main(a.mode, a.platform, a.deployment, a.until, a.interval, a.order, a.device)
    return 0


if __name__ == "__main__":
    sys.exit(main())
