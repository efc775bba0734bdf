#!/usr/bin/env python3
"""The churn collect-all engine (fu.CollectAllChurn) beside the lossy one at loss = 0, in one
process, on the headline graph: ER(n, m, seed 1), uniform values (seed 0), from zero, rounds
0 .. R-1 with rounds 1 .. R-1 timed on the device.

Before any timing, an all-alive churn run is checked against coracle.ca_sync bit for bit. Then
one JSON line with the box's copy rate and the lossy engine's window at loss = 0, and one JSON
line per churn setting:
  all_alive: every node alive and every link up;
  dead:      --dead of the nodes dead from round 0 on (node i dead iff U_i < dead on the
             fu_values_uniform stream at --seed), so their rows do not fire and every slot at
             them is DOWN,
each with us_per_round, bytes = 41 E + 25 n for all_alive (the lossy round's 40 E + 24 n plus one
state byte per slot and one alive byte per node; a DOWN slot moves no gather, so the figure is
an upper bound for `dead`), roofline = bytes / 8 TB/s / time, and ratio = t_churn / t_lossy.
Every time is the median of --reps windows, each after a reset; the engines alternate within a
repetition.

    python tools/bench_churn.py [--n 1000000] [--m 4000000] [--rounds 20] [--dead 0.1]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "simgrid-flow-updating-implementation_amd"))

import numpy as np  # noqa: E402

import coracle  # noqa: E402
import fu  # noqa: E402

PEAK = 8.0e12  # bytes / s


def window_us(eng, rounds):
    """Device microseconds per round over rounds 1 .. rounds-1, from zero."""
    eng.reset()
    eng.run(1)
    eng.synchronize()
    return eng.run_timed(rounds - 1) * 1e3 / (rounds - 1)


def check_parity(g, v, rounds):
    with fu.CollectAllChurn(g, v) as eng:
        eng.run(rounds)
        a, f = eng.estimates(), eng.flows()
    a_ref, f_ref = coracle.ca_sync(*g.arrays(), v, rounds, nthreads=coracle.max_threads())
    for got, ref in ((a, a_ref), (f, f_ref)):
        if not np.array_equal(got.view(np.uint64), ref.view(np.uint64)):
            raise SystemExit("bench_churn: the all-alive run differs from the oracle")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--dead", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.rounds < 2:
        ap.error("--rounds must be at least 2 (round 0 is not timed)")
    g = fu.Graph.erdos_renyi(a.n, a.m, seed=1)
    v = fu.uniform_values(g.n, seed=0)
    check_parity(g, v, a.rounds)
    alive = ~(fu.uniform_values(g.n, seed=a.seed, lo=0.0, hi=1.0) < a.dead)
    with fu.CollectAllLossy(g, v) as lossy, fu.CollectAllChurn(g, v) as up, fu.CollectAllChurn(g, v) as dead:
        dead.set_topology(alive=alive)
        engines = {"lossy": lossy, "all_alive": up, "dead": dead}
        for eng in engines.values():
            eng.run(a.rounds)  # warm
        t = {k: [] for k in engines}
        for _ in range(a.reps):
            for k, eng in engines.items():
                t[k].append(window_us(eng, a.rounds))
        med = {k: statistics.median(x) for k, x in t.items()}
        print(json.dumps({"graph": f"er(n={a.n},m={a.m},seed=1)", "n": g.n, "E": g.E, "rounds_timed": [1, a.rounds - 1],
                          "reps": a.reps, "parity": "all alive bitwise vs coracle.ca_sync",
                          "copy_GBs": round(fu.copy_bandwidth(0), 1), "lossy_us_per_round": round(med["lossy"], 2),
                          "lossy_us_per_round_min": round(min(t["lossy"]), 2)}), flush=True)
        nbytes = 41 * g.E + 25 * g.n
        for k in ("all_alive", "dead"):
            nodes, slots = engines[k].stats
            print(json.dumps({"setting": k, "alive_nodes": nodes, "live_slots": slots, "us_per_round": round(med[k], 2),
                              "us_per_round_min": round(min(t[k]), 2), "bytes_upper": nbytes,
                              "floor_us_at_8TBs": round(nbytes / PEAK * 1e6, 2),
                              "roofline": round(nbytes / PEAK / (med[k] * 1e-6), 4),
                              "lossy_us_per_round": round(med["lossy"], 2), "ratio": round(med[k] / med["lossy"], 4)}), flush=True)


if __name__ == "__main__":
    main()
