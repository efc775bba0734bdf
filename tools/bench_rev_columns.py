#!/usr/bin/env python3
"""K value columns in one lossy or churn handle (fu.CollectAllLossyBatch, fu.CollectAllChurnBatch)
beside the scalar handle of the same engine, in one process, on the headline graph: ER(n, m,
seed 1), column c uniform values at seed c, from zero, rounds 0 .. R-1 with rounds 1 .. R-1 timed
on the device.

Before any timing, column 1 of a K = 4 run of either engine is checked against the scalar handle
run on that column, bit for bit. Then one JSON line with the box's copy rate, and per setting
  lossy p = 0, lossy p = 0.1, churn all alive, churn with --dead of the nodes dead from round 0 on
one JSON line per K with us_per_round, us_per_round_per_column, ratio = t(K) / (K t_scalar) for the
scalar handle of that setting, and model_ratio = bytes(K) / (K bytes(1)) from
  bytes(K) = shared + K (32 E + 16 n),  shared = 8 E + 8 n (col, rev, rowptr), + E + n under churn
(the state and alive bytes); 32 E + 16 n are a column's two gathers, its flow write, its value and
its estimate write. K = 1 is a handle of the K-column create, which runs the scalar kernels.
Every time is the median of --reps windows, each after a reset; the handles of a setting alternate
within a repetition.

    python tools/bench_rev_columns.py [--n 1000000] [--m 4000000] [--rounds 20] [--dead 0.1]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simgrid-flow-updating-implementation_amd"))

import numpy as np  # noqa: E402

import fu  # noqa: E402

WIDTHS = (1, 2, 4, 8, 16)


def window_us(eng, rounds):
    """Device microseconds per round over rounds 1 .. rounds-1, from zero."""
    eng.reset()
    eng.run(1)
    eng.synchronize()
    return eng.run_timed(rounds - 1) * 1e3 / (rounds - 1)


def model_bytes(engine, n, E, K):
    shared = 8 * E + 8 * n + (E + n if engine == "churn" else 0)
    return shared + K * (32 * E + 16 * n)


def check_parity(g, V, rounds, alive):
    for engine in ("lossy", "churn"):
        if engine == "lossy":
            wide, one = fu.CollectAllLossyBatch(g, V, loss=0.1, seed=7), fu.CollectAllLossy(g, V[:, 1], loss=0.1, seed=7)
        else:
            wide, one = fu.CollectAllChurnBatch(g, V), fu.CollectAllChurn(g, np.ascontiguousarray(V[:, 1]))
            wide.set_topology(alive=alive)
            one.set_topology(alive=alive)
        with wide, one:
            wide.run(rounds)
            one.run(rounds)
            for got, ref in ((wide.estimates()[:, 1], one.estimates()), (wide.flows()[:, 1], one.flows())):
                if not np.array_equal(np.ascontiguousarray(got).view(np.uint64), ref.view(np.uint64)):
                    raise SystemExit(f"bench_rev_columns: column 1 of the {engine} K = 4 run differs from the scalar handle")
            if wide.stats != one.stats:
                raise SystemExit(f"bench_rev_columns: {engine} stats differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--dead", type=float, default=0.1)
    ap.add_argument("--loss", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.rounds < 2:
        ap.error("--rounds must be at least 2 (round 0 is not timed)")
    g = fu.Graph.erdos_renyi(a.n, a.m, seed=1)
    V = np.ascontiguousarray(np.stack([fu.uniform_values(g.n, seed=c) for c in range(max(WIDTHS))], axis=1))
    alive = ~(fu.uniform_values(g.n, seed=a.seed, lo=0.0, hi=1.0) < a.dead)
    check_parity(g, np.ascontiguousarray(V[:, :4]), a.rounds, alive)
    print(json.dumps({"graph": f"er(n={a.n},m={a.m},seed=1)", "n": g.n, "E": g.E, "rounds_timed": [1, a.rounds - 1],
                      "reps": a.reps, "parity": "column 1 of K = 4 bitwise vs the scalar handle, both engines",
                      "copy_GBs": round(fu.copy_bandwidth(0), 1)}), flush=True)
    settings = (("lossy", "p=0", {"loss": 0.0}), ("lossy", f"p={a.loss}", {"loss": a.loss, "seed": a.seed}),
                ("churn", "all_alive", None), ("churn", f"dead={a.dead}", alive))
    for engine, name, arg in settings:
        v0 = np.ascontiguousarray(V[:, 0])
        if engine == "lossy":
            handles = {"scalar": fu.CollectAllLossy(g, v0, **arg)}
            handles.update({K: fu.CollectAllLossyBatch(g, np.ascontiguousarray(V[:, :K]), **arg) for K in WIDTHS})
        else:
            handles = {"scalar": fu.CollectAllChurn(g, v0)}
            handles.update({K: fu.CollectAllChurnBatch(g, np.ascontiguousarray(V[:, :K])) for K in WIDTHS})
            if arg is not None:
                for eng in handles.values():
                    eng.set_topology(alive=arg)
        try:
            for eng in handles.values():
                eng.run(a.rounds)  # warm
            t = {k: [] for k in handles}
            for _ in range(a.reps):
                for k, eng in handles.items():
                    t[k].append(window_us(eng, a.rounds))
            med = {k: statistics.median(x) for k, x in t.items()}
            for K in WIDTHS:
                print(json.dumps({"engine": engine, "setting": name, "K": K, "us_per_round": round(med[K], 2),
                                  "us_per_round_min": round(min(t[K]), 2),
                                  "us_per_round_per_column": round(med[K] / K, 2),
                                  "scalar_us_per_round": round(med["scalar"], 2),
                                  "ratio": round(med[K] / (K * med["scalar"]), 4),
                                  "model_ratio": round(model_bytes(engine, g.n, g.E, K) / (K * model_bytes(engine, g.n, g.E, 1)), 4),
                                  "GBs_by_model": round(model_bytes(engine, g.n, g.E, K) / (med[K] * 1e-6) / 1e9, 1)}),
                      flush=True)
        finally:
            for eng in handles.values():
                eng.close()


if __name__ == "__main__":
    main()
