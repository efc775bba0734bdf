#!/usr/bin/env python3
"""The synchronous pairwise engine (fu.PairwiseSync), in one process.

1. RR(65536, 8), R rounds from zero: fu_pair beside fu_replay (per-tick batches and the
   persistent kernel) on the host-built trace of the same 3 R ticks (a round is three ticks:
   the initiators' FIRE_PW; the listeners' RECV and FIRE_PW; the initiators' RECV). Both carry
   the same events; their final states are compared bit for bit before any number is printed.
   One JSON line: us per round of each, pairwise updates/s (two fires per pair), trace size and
   host build time, and ratio = t_pair / t_replay_persistent (below 0.85 a win, above 1.15 a
   loss, a tie between).
2. ER(n, 4 n) and RR(n, 8), n = 1,000,000: rounds 1 .. R-1 timed on the device, median of
   --reps windows, each after a reset, for both forms of the matching ("match" 0: proposers
   push an atomicMin, 1: listeners scan their rows). One JSON line per graph and form with
   us_per_round, pairs_per_round, the byte model
     bytes = sum over pairs of 8 (deg_i + deg_j) + 116
   (both flow rows; reads of c[s], c[t], v_i, v_j, four row pointers, one rev; writes of two
   flows, two caches, two last averages; the matching's own traffic is not in it), roofline =
   bytes / 8 TB/s / time, and the box's copy rate.

3. With --loss P [P ...]: in place of 2, the same two graphs and windows under message loss.
   One handle per p (p = 0, the lossless kernels, first), all on the "atomic_min" matching; the
   handles alternate within each repetition. One JSON line per graph and p with us_per_round,
   the outcomes per round (first messages lost, answers lost, complete) and the byte model
     bytes = sum over pairs of 8 (deg_i + deg_j) + 116, or 8 deg_i + 76 where m1 is lost
   (a lost m1 skips row j, v_j and c[t] and three of the six stores; a lost m2 moves the same
   bytes as a complete exchange; the mask-free decision reads nothing).

4. With --columns K [K ...]: in place of 2, the same two graphs and windows for one scalar handle
   (fu.PairwiseSync) and one fu.PairwiseSyncBatch per K, all on the "atomic_min" matching and
   without loss; the handles alternate within each repetition. Column 0 of every K-column handle
   is compared bit for bit with the scalar handle before any number is printed. One JSON line
   per graph and handle with us_per_round (median, min, max), k_scalar_us = K times the scalar
   handle's median of the same session, ratio = us_per_round / k_scalar_us, and the byte model
     bytes = sum over pairs of K (8 (deg_i + deg_j) + 80) + 36
   (per column both flow rows, c[s], c[t], v_i, v_j and the six stores; per pair four row
   pointers and one rev).

5. With --churn F: in place of 2, the same two graphs and windows for three scalar handles on the
   "atomic_min" matching without loss: one that never gets a topology call (the kernels without
   a topology), one with set_topology() and everything alive (the topology kernels, the same
   pairs and the same bits: compared before any number is printed), and one with node i dead iff
   U_i < F (the stream of `python -m fu bench-graph --churn`, at seed 5: independent of the
   values). reset keeps the topology; the three alternate within each repetition. One JSON line per
   graph and handle with us_per_round (median, min, max), pairs_per_round, alive, live_slots and
   ratio_over_no_topology.

    python tools/bench_pair.py [--rounds 200] [--n 1000000] [--reps 7] [--skip-replay] [--loss 0.1 0.3]
    python tools/bench_pair.py --skip-replay --columns 1 2 4 8 16
    python tools/bench_pair.py --skip-replay --churn 0.1
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simgrid-flow-updating-implementation_amd"))

import numpy as np  # noqa: E402

import fu  # noqa: E402
from fu import _lib as L  # noqa: E402

PEAK = 8.0e12  # bytes / s
SEED = 7
CHURN_SEED = 5  # --churn: which nodes die


def round_pairs(g, src, seed, r):
    """(i, s, j, t) arrays of round r from the host matching (fu_pair_matching); the slot is
    where the partner sits in the initiator's row (simple graphs)."""
    mate, ini = fu.pair_matching(g, seed, r)
    ks = np.flatnonzero((ini[src] == 1) & (g.col == mate[src]))
    i = src[ks]
    j = g.col[ks].astype(np.int64)
    return i, ks - g.rowptr[i], j, g.rev[ks] - g.rowptr[j]


def build_trace(g, seed, rounds):
    """The rounds as replay ticks (three per round), and the pairs of the run."""
    src = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(g.rowptr))
    deg = np.diff(g.rowptr)
    tasks, events, tto = [], [], [0]
    q = nt = ne = 0
    for r in range(rounds):
        i, s, j, t = round_pairs(g, src, seed, r)
        p = len(i)
        m1 = 2 * (q + np.arange(p))
        z = np.zeros(p, dtype=np.int64)
        e1 = ne + np.arange(p)
        e2 = ne + p + 2 * np.arange(p)
        e3 = ne + 3 * p + np.arange(p)
        tasks += [np.stack([i, e1, e1 + 1], 1), np.stack([j, e2, e2 + 2], 1), np.stack([i, e3, e3 + 1], 1)]
        recv_fire = np.empty((2 * p, 4), dtype=np.int64)
        recv_fire[0::2] = np.stack([z, t, m1, z], 1)
        recv_fire[1::2] = np.stack([z + 2, t, deg[j], m1 + 1], 1)
        events += [np.stack([z + 2, s, deg[i], m1], 1), recv_fire, np.stack([z, s, m1 + 1, z], 1)]
        tto += [nt + p, nt + 2 * p, nt + 3 * p]
        nt += 3 * p
        ne += 4 * p
        q += p
    return {"tick_task_off": np.array(tto, dtype=np.int64),
            "tasks": np.ascontiguousarray(np.concatenate(tasks), dtype=np.int32),
            "events": np.ascontiguousarray(np.concatenate(events), dtype=np.int32),
            "n_msgs": 2 * q, "pairs": q}


def replay_run(g, v, tr, ticks, persistent):
    """(device ms, last, flows, caches) of fu_replay on the trace."""
    h = L.vp()
    out_ids = np.zeros(1, dtype=np.int32)
    L.call("fu_replay_create", g.n, L.ptr(g.rowptr), L.ptr(v), ticks, L.ptr(tr["tick_task_off"]), len(tr["tasks"]),
           L.ptr(tr["tasks"]), len(tr["events"]), L.ptr(tr["events"]), 0, L.ptr(out_ids), tr["n_msgs"], 0, ctypes.byref(h))
    if persistent:
        L.call("fu_replay_set_option", h, b"persistent", 1)
    ms = L.f32()
    L.call("fu_replay_run_timed", h, ticks, ctypes.byref(ms))
    last, fl, es = np.empty(g.n), np.empty(g.E), np.empty(g.E)
    L.call("fu_replay_get", h, L.ptr(last), L.ptr(fl), L.ptr(es))
    L.lib.fu_replay_destroy(h)
    return float(ms.value), last, fl, es


def same_bits(a, b):
    return bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def against_replay(rounds):
    g = fu.Graph.random_regular(65536, 8, seed=1)
    v = fu.uniform_values(g.n, seed=0)
    t0 = time.perf_counter()
    tr = build_trace(g, SEED, rounds)
    t_build = time.perf_counter() - t0
    with fu.PairwiseSync(g, v, seed=SEED) as eng:
        eng.run(rounds)  # warm
        eng.reset()
        ms_pair = eng.run_timed(rounds)
        state = (eng.estimates(), eng.flows(), eng.cache())
        pairs = eng.stats[0]
    res = {}
    for pers in (False, True):
        replay_run(g, v, tr, 3 * rounds, pers)  # warm
        ms, *st = replay_run(g, v, tr, 3 * rounds, pers)
        if not all(same_bits(a, b) for a, b in zip(st, state)):
            raise SystemExit("bench_pair: fu_pair and fu_replay differ on the same events")
        res[pers] = ms
    if pairs != tr["pairs"]:
        raise SystemExit("bench_pair: the engine's pair count differs from the host matching's")
    ratio = ms_pair / res[True]
    print(json.dumps({"graph": "rr(n=65536,d=8,seed=1)", "rounds": rounds, "ticks": 3 * rounds, "pairs": pairs,
                      "parity": "fu_pair bitwise equal to fu_replay (both modes)",
                      "trace_bytes": int(tr["tasks"].nbytes + tr["events"].nbytes), "trace_build_s": round(t_build, 3),
                      "pair_us_per_round": round(ms_pair * 1e3 / rounds, 3),
                      "replay_per_tick_us_per_round": round(res[False] * 1e3 / rounds, 3),
                      "replay_persistent_us_per_round": round(res[True] * 1e3 / rounds, 3),
                      "pair_updates_per_s": round(2 * pairs / (ms_pair / 1e3), 1),
                      "replay_persistent_updates_per_s": round(2 * pairs / (res[True] / 1e3), 1),
                      "ratio_pair_over_replay_persistent": round(ratio, 4),
                      "verdict": "win" if ratio < 0.85 else "loss" if ratio > 1.15 else "tie"}), flush=True)


def window_us(eng, rounds, reps):
    """Median device microseconds per round over rounds 1 .. rounds-1, from zero each time, and
    the pairs of one such window."""
    t = []
    for _ in range(reps):
        eng.reset()
        eng.run(1)
        eng.synchronize()
        first = eng.stats[0]
        t.append(eng.run_timed(rounds - 1) * 1e3 / (rounds - 1))
    return statistics.median(t), min(t), eng.stats[0] - first


def model_bytes_per_pair(g, seed):
    """8 (deg_i + deg_j) + 116 averaged over the pairs of rounds 1-4 (host matching)."""
    deg = np.diff(g.rowptr)
    tot = cnt = 0
    for r in range(1, 5):
        mate, ini = fu.pair_matching(g, seed, r)
        i = np.flatnonzero(ini)
        tot += int(np.sum(8 * (deg[i] + deg[mate[i]]) + 116))
        cnt += len(i)
    return tot / cnt


def big(name, g, rounds, reps, copy_gbs):
    v = fu.uniform_values(g.n, seed=0)
    per_pair = model_bytes_per_pair(g, SEED)
    with fu.PairwiseSync(g, v, seed=SEED) as eng:
        eng.run(rounds)  # warm
        ref = None
        for match in (0, 1):
            eng.set_option("match", match)
            t, t_min, pairs = window_us(eng, rounds, reps)
            state = (eng.estimates(), eng.flows(), eng.cache())
            if ref is None:
                ref = state
            elif not all(same_bits(a, b) for a, b in zip(state, ref)):
                raise SystemExit("bench_pair: the two forms of the matching differ")
            ppr = pairs / (rounds - 1)
            nbytes = ppr * per_pair
            print(json.dumps({"graph": name, "n": g.n, "E": g.E, "match": ["atomic_min", "listener_scan"][match],
                              "rounds_timed": [1, rounds - 1], "reps": reps, "us_per_round": round(t, 2),
                              "us_per_round_min": round(t_min, 2), "pairs_per_round": round(ppr, 1),
                              "pairs_per_node": round(ppr / g.n, 4), "model_bytes_per_pair": round(per_pair, 1),
                              "model_bytes_per_round": int(nbytes), "roofline": round(nbytes / PEAK / (t * 1e-6), 5),
                              "pair_updates_per_s": round(2 * ppr / (t * 1e-6), 1), "copy_GBs": copy_gbs}), flush=True)


def model_bytes_under_loss(g, seed, loss_seed, p):
    """The byte model averaged over the pairs of rounds 1-4: 8 deg_i + 76 where m1 is lost (the
    host's fu_pair_lost on the listener's slot), 8 (deg_i + deg_j) + 116 otherwise."""
    deg = np.diff(g.rowptr)
    src = np.repeat(np.arange(g.n, dtype=np.int64), deg)
    tot = cnt = 0
    for r in range(1, 5):
        i, s, j, t = round_pairs(g, src, seed, r)
        lost1 = fu.pair_lost(loss_seed, r, 0, g.E, p)[g.rowptr[j] + t] != 0
        tot += int(np.sum(np.where(lost1, 8 * deg[i] + 76, 8 * (deg[i] + deg[j]) + 116)))
        cnt += len(i)
    return tot / cnt


def big_lossy(name, g, rounds, reps, copy_gbs, losses):
    """us per round at p = 0 (the lossless kernels) and at every p of `losses`, the handles
    alternating within each repetition."""
    v = fu.uniform_values(g.n, seed=0)
    ps = [0.0] + [p for p in losses if p > 0.0]
    engs = [fu.PairwiseSync(g, v, seed=SEED, loss=p, loss_seed=SEED) for p in ps]
    try:
        for eng in engs:
            eng.run(rounds)  # warm
        t = [[] for _ in engs]
        for _ in range(reps):
            for q, eng in enumerate(engs):
                eng.reset()
                eng.run(1)
                eng.synchronize()
                t[q].append(eng.run_timed(rounds - 1) * 1e3 / (rounds - 1))
        for q, (eng, p) in enumerate(zip(engs, ps)):
            per_round = lambda x: round(x / (rounds - 1), 1)  # noqa: E731
            eng.reset()
            eng.run(1)
            eng.synchronize()
            p0, l0 = eng.stats[0], eng.loss_stats
            eng.run(rounds - 1)
            ppr = (eng.stats[0] - p0) / (rounds - 1)
            out = [per_round(a - b) for a, b in zip(eng.loss_stats, l0)]
            per_pair = model_bytes_under_loss(g, SEED, SEED, p)
            us = statistics.median(t[q])
            print(json.dumps({"graph": name, "n": g.n, "E": g.E, "loss": p, "kernels": "lossy" if p > 0 else "lossless",
                              "rounds_timed": [1, rounds - 1], "reps": reps, "us_per_round": round(us, 2),
                              "us_per_round_min": round(min(t[q]), 2), "us_per_round_max": round(max(t[q]), 2),
                              "pairs_per_round": round(ppr, 1), "first_lost_per_round": out[0],
                              "answers_lost_per_round": out[1], "complete_per_round": out[2],
                              "model_bytes_per_pair": round(per_pair, 1), "model_bytes_per_round": int(ppr * per_pair),
                              "roofline": round(ppr * per_pair / PEAK / (us * 1e-6), 5), "copy_GBs": copy_gbs}), flush=True)
    finally:
        for eng in engs:
            eng.close()


def columns_values(n, K):
    """(n, K): column 0 the scalar run's inputs, column 1 the COUNT indicator, then uniform streams."""
    cols = [fu.uniform_values(n, seed=0)]
    if K > 1:
        one = np.zeros(n)
        one[0] = 1.0
        cols.append(one)
    cols += [fu.uniform_values(n, seed=c) for c in range(2, K)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def big_columns(name, g, rounds, reps, copy_gbs, widths):
    """us per round of the scalar handle and of a K-column handle per K of `widths`, the handles
    alternating within each repetition."""
    per_pair_1 = model_bytes_per_pair(g, SEED)  # 8 (deg_i + deg_j) + 116
    engs = [fu.PairwiseSync(g, fu.uniform_values(g.n, seed=0), seed=SEED)]
    engs += [fu.PairwiseSyncBatch(g, columns_values(g.n, K), seed=SEED) for K in widths]
    try:
        for eng in engs:
            eng.run(rounds)  # warm
        t = [[] for _ in engs]
        pairs = 0
        for _ in range(reps):
            for q, eng in enumerate(engs):
                eng.reset()
                eng.run(1)
                eng.synchronize()
                first = eng.stats[0]
                t[q].append(eng.run_timed(rounds - 1) * 1e3 / (rounds - 1))
                pairs = eng.stats[0] - first
        ref = (engs[0].estimates(), engs[0].flows(), engs[0].cache())
        for eng in engs[1:]:
            state = (eng.estimates()[:, 0], eng.flows()[:, 0], eng.cache()[:, 0])
            if not all(same_bits(np.ascontiguousarray(a), b) for a, b in zip(state, ref)):
                raise SystemExit("bench_pair: column 0 of a K-column handle differs from the scalar handle")
        ppr = pairs / (rounds - 1)
        scalar_us = statistics.median(t[0])
        for q, (eng, K) in enumerate(zip(engs, [None] + list(widths))):
            us = statistics.median(t[q])
            k = K or 1
            per_pair = k * (per_pair_1 - 36) + 36
            line = {"graph": name, "n": g.n, "E": g.E, "handle": "scalar" if K is None else "columns", "columns": k,
                    "rounds_timed": [1, rounds - 1], "reps": reps, "us_per_round": round(us, 2),
                    "us_per_round_min": round(min(t[q]), 2), "us_per_round_max": round(max(t[q]), 2),
                    "pairs_per_round": round(ppr, 1), "model_bytes_per_pair": round(per_pair, 1),
                    "model_bytes_per_round": int(ppr * per_pair), "roofline": round(ppr * per_pair / PEAK / (us * 1e-6), 5),
                    "copy_GBs": copy_gbs}
            if K is not None:
                line.update({"k_scalar_us": round(k * scalar_us, 2), "ratio_over_k_scalar": round(us / (k * scalar_us), 4)})
            print(json.dumps(line), flush=True)
    finally:
        for eng in engs:
            eng.close()


def big_churn(name, g, rounds, reps, copy_gbs, frac):
    """us per round of a handle without a topology, one with everything alive and one with a
    fraction `frac` of the nodes dead, alternating within each repetition."""
    v = fu.uniform_values(g.n, seed=0)
    alive = ~(fu.uniform_values(g.n, seed=CHURN_SEED, lo=0.0, hi=1.0) < frac)  # not the values' stream (seed 0)
    kinds = ["no_topology", "all_alive", "dead"]
    engs = [fu.PairwiseSync(g, v, seed=SEED) for _ in kinds]
    try:
        engs[1].set_topology()
        engs[2].set_topology(alive=alive)
        for eng in engs:
            eng.run(rounds)  # warm
        t = [[] for _ in engs]
        pairs = [0] * len(engs)
        for _ in range(reps):
            for q, eng in enumerate(engs):
                eng.reset()
                eng.run(1)
                eng.synchronize()
                first = eng.stats[0]
                t[q].append(eng.run_timed(rounds - 1) * 1e3 / (rounds - 1))
                pairs[q] = eng.stats[0] - first
        ref = (engs[0].estimates(), engs[0].flows(), engs[0].cache())
        if not all(same_bits(a, b) for a, b in zip((engs[1].estimates(), engs[1].flows(), engs[1].cache()), ref)):
            raise SystemExit("bench_pair: the all-alive topology handle differs from the handle without a topology")
        base = statistics.median(t[0])
        for q, (eng, kind) in enumerate(zip(engs, kinds)):
            us = statistics.median(t[q])
            n_alive, n_live = eng.topology_stats
            print(json.dumps({"graph": name, "n": g.n, "E": g.E, "handle": kind, "churn": frac if kind == "dead" else 0.0,
                              "alive": n_alive, "live_slots": n_live, "rounds_timed": [1, rounds - 1], "reps": reps,
                              "us_per_round": round(us, 2), "us_per_round_min": round(min(t[q]), 2),
                              "us_per_round_max": round(max(t[q]), 2), "pairs_per_round": round(pairs[q] / (rounds - 1), 1),
                              "ratio_over_no_topology": round(us / base, 4), "copy_GBs": copy_gbs}), flush=True)
    finally:
        for eng in engs:
            eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-replay", action="store_true")
    ap.add_argument("--loss", type=float, nargs="+", default=None, metavar="P",
                    help="time the big graphs at p = 0 and at every P, in place of the A/B of the matching")
    ap.add_argument("--columns", type=int, nargs="+", default=None, metavar="K",
                    help="time the big graphs with a scalar handle and a K-column handle per K, in place of the A/B of the matching")
    ap.add_argument("--churn", type=float, default=None, metavar="F",
                    help="time the big graphs without a topology, with everything alive and with a fraction F dead")
    a = ap.parse_args()
    if a.churn is not None and (a.loss is not None or a.columns is not None or not 0.0 <= a.churn < 1.0):
        ap.error("--churn takes a fraction in [0, 1) and does not combine with --loss or --columns")
    if a.columns is not None and (a.loss is not None or not all(1 <= k <= 16 for k in a.columns)):
        ap.error("--columns takes widths in 1..16 and does not combine with --loss")
    if a.rounds < 2:
        ap.error("--rounds must be at least 2 (round 0 is not timed)")
    if not a.skip_replay:
        against_replay(a.rounds)
    copy_gbs = round(fu.copy_bandwidth(0), 1)
    if a.churn is not None:
        big_churn(f"er(n={a.n},m={4 * a.n},seed=1)", fu.Graph.erdos_renyi(a.n, 4 * a.n, seed=1), a.rounds, a.reps, copy_gbs, a.churn)
        big_churn(f"rr(n={a.n},d=8,seed=1)", fu.Graph.random_regular(a.n, 8, seed=1), a.rounds, a.reps, copy_gbs, a.churn)
        return
    if a.columns is not None:
        big_columns(f"er(n={a.n},m={4 * a.n},seed=1)", fu.Graph.erdos_renyi(a.n, 4 * a.n, seed=1), a.rounds, a.reps, copy_gbs, a.columns)
        big_columns(f"rr(n={a.n},d=8,seed=1)", fu.Graph.random_regular(a.n, 8, seed=1), a.rounds, a.reps, copy_gbs, a.columns)
        return
    if a.loss is not None:
        if not all(0.0 <= p <= 1.0 for p in a.loss):
            ap.error("--loss takes probabilities in [0, 1]")
        big_lossy(f"er(n={a.n},m={4 * a.n},seed=1)", fu.Graph.erdos_renyi(a.n, 4 * a.n, seed=1), a.rounds, a.reps, copy_gbs, a.loss)
        big_lossy(f"rr(n={a.n},d=8,seed=1)", fu.Graph.random_regular(a.n, 8, seed=1), a.rounds, a.reps, copy_gbs, a.loss)
        return
    big(f"er(n={a.n},m={4 * a.n},seed=1)", fu.Graph.erdos_renyi(a.n, 4 * a.n, seed=1), a.rounds, a.reps, copy_gbs)
    big(f"rr(n={a.n},d=8,seed=1)", fu.Graph.random_regular(a.n, 8, seed=1), a.rounds, a.reps, copy_gbs)


if __name__ == "__main__":
    main()
