#!/usr/bin/env python3
"""The batched collect-all engine (fu.CollectAllBatch) against K runs of the scalar one, in
one process, on the headline window: ER(n, m, seed 1), uniform values per column (seed =
column), from zero, rounds 0 .. R-1 with rounds 1 .. R-1 timed on the device.

Before any timing, column 0 of a K = 4 run is checked against coracle.ca_sync bit for bit.
Then one JSON line with the box's copy rate and the scalar engine's window (kernel auto:
tune(), reset(), then the window), and one JSON line per K with
  us_per_round, bytes = E (4 + 16 K) + n (8 + 24 K) (col, one K-wide gather, own flows read
  and written; row pointer, values, a_{r-2} read, a_r written), roofline = bytes / 8 TB/s /
  time, and ratio = t_batch(K) / (K t_scalar): below 1, a column costs less here than a
  scalar run of its own.
Every time is the median of --reps windows, each after a reset.

    python tools/bench_batch.py [--n 1000000] [--m 4000000] [--rounds 20] [--columns 1,2,4,8,16]
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


def window_us(eng, rounds, reps):
    """Median device microseconds per round over rounds 1 .. rounds-1, from zero each time."""
    t = []
    for _ in range(reps):
        eng.reset()
        eng.run(1)
        eng.synchronize()
        t.append(eng.run_timed(rounds - 1) * 1e3 / (rounds - 1))
    return statistics.median(t), min(t)


def check_parity(g, rounds):
    vs = [fu.uniform_values(g.n, seed=c) for c in range(4)]
    with fu.CollectAllBatch(g, np.stack(vs, axis=1)) as eng:
        eng.run(rounds)
        a, f = eng.estimates(), eng.flows()
    a_ref, f_ref = coracle.ca_sync(*g.arrays(), vs[0], rounds, nthreads=coracle.max_threads())
    for got, ref in ((a[:, 0], a_ref), (f[:, 0], f_ref)):
        if not np.array_equal(np.ascontiguousarray(got).view(np.uint64), ref.view(np.uint64)):
            raise SystemExit("bench_batch: column 0 of the K = 4 run differs from the oracle")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--columns", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.rounds < 2:
        ap.error("--rounds must be at least 2 (round 0 is not timed)")
    ks = [int(x) for x in a.columns.split(",")]
    g = fu.Graph.erdos_renyi(a.n, a.m, seed=1)
    check_parity(g, a.rounds)
    one = fu.CollectAll(g, fu.uniform_values(g.n, seed=0))
    one.tune()
    t1, t1_min = window_us(one, a.rounds, a.reps)
    kernel = one.info()["kernel"]
    one.close()
    print(json.dumps({"graph": f"er(n={a.n},m={a.m},seed=1)", "n": g.n, "E": g.E, "rounds_timed": [1, a.rounds - 1],
                      "reps": a.reps, "parity": "column 0 of K=4 bitwise vs coracle.ca_sync",
                      "copy_GBs": round(fu.copy_bandwidth(0), 1), "scalar_kernel": kernel,
                      "scalar_us_per_round": round(t1, 2), "scalar_us_per_round_min": round(t1_min, 2)}), flush=True)
    for k in ks:
        v = np.stack([fu.uniform_values(g.n, seed=c) for c in range(k)], axis=1)
        with fu.CollectAllBatch(g, v) as eng:
            eng.run(a.rounds)  # warm
            t, t_min = window_us(eng, a.rounds, a.reps)
        nbytes = g.E * (4 + 16 * k) + g.n * (8 + 24 * k)
        print(json.dumps({"K": k, "us_per_round": round(t, 2), "us_per_round_min": round(t_min, 2),
                          "us_per_round_per_column": round(t / k, 2), "bytes": nbytes,
                          "floor_us_at_8TBs": round(nbytes / PEAK * 1e6, 2),
                          "roofline": round(nbytes / PEAK / (t * 1e-6), 4),
                          "scalar_us_per_round": round(t1, 2), "ratio": round(t / (k * t1), 4)}), flush=True)


if __name__ == "__main__":
    main()
