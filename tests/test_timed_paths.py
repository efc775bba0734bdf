"""What the timed entry points compute: fu_run_collectall_timed, fu_batch_run_timed,
fu_lossy_run_timed and fu_pair_run_timed against the restatements the run() parity tests use
(coracle.ca_sync / ca_rounds, lossy_cases.oracle_lossy, pair_cases.oracle_pair), by bit pattern.
tools/bench_batch.py, bench_lossy.py and bench_pair.py time `reset(); run(1); run_timed(R - 1)`:
a timed call that picked another round phase, hash round or buffer than run() would make those
figures the timing of another computation.

One body per case over seven handles: CollectAll with the kernel forced to recon, stage and
pregather, CollectAllBatch at K = 3, CollectAllLossy at p = 0.25 and PairwiseSync with both
matchers. The collect-all engines run on parity_util._class_edge_graph(7) (every row class from
degree 0 to the block-per-row rows), the pairwise engine on pair_cases.class_graph(); the values
are the `sym` and `wide` families. Every returned time of a call with rounds > 0 is finite and
positive; no magnitude is asserted.

Last, fu_reset on a kernel-"auto" handle whose first autotune pass ran at a packed width."""
import functools
import math

import numpy as np
import pytest

import coracle
import fu
from lossy_cases import hashed, oracle_lossy
from pair_cases import class_graph, oracle_pair
from parity_util import CLASS_EDGE_DEGREES, FAMILIES, _class_edge_graph, assert_same_bits

pytestmark = pytest.mark.gpu

SEED = 11
LOSS = 0.25
CA_STOPS = (1, 2, 3, 4, 5, 7, 8, 9, 17, 20)


def _timed(eng, rounds):
    """run_timed(rounds) with the condition on every returned time."""
    ms = eng.run_timed(rounds)
    assert math.isfinite(ms), ms
    assert ms > 0.0 if rounds > 0 else ms >= 0.0, (rounds, ms)
    return ms


@functools.lru_cache(maxsize=None)
def _ca_graph():
    return _class_edge_graph(7)


@functools.lru_cache(maxsize=None)
def _ca_refs(family, seed):
    """(v, {r: (a, f)}) after r rounds from zero for every r of CA_STOPS, from the C oracle."""
    g = _ca_graph()
    v = FAMILIES[family](g.n, seed=seed)
    refs, done = {}, 0
    a = f = None
    for r in CA_STOPS:
        if a is None:
            a, f = coracle.ca_sync(*g.arrays(), v, r, nthreads=16)
        else:
            coracle.ca_rounds(*g.arrays(), v, r - done, a, f, nthreads=16)
        done = r
        refs[r] = (a.copy(), f.copy())
    return v, refs


@functools.lru_cache(maxsize=None)
def _lossy_ref(rounds):
    g = _ca_graph()
    a, f, _ = oracle_lossy(*g.arrays(), _ca_refs("sym", 3)[0], rounds, hashed(LOSS, SEED, g.E))
    return a, f


@functools.lru_cache(maxsize=None)
def _pair_values():
    return FAMILIES["sym"](class_graph().n, seed=3)


@functools.lru_cache(maxsize=None)
def _pair_ref(rounds):
    return oracle_pair(*class_graph().arrays(), _pair_values(), rounds, SEED)[:3]


def _pair_stats(g, seed_at, rounds):
    """(pairs, nodes that never fired) over rounds 0 .. rounds-1, from fu.pair_matching alone."""
    pairs, fired = 0, np.zeros(g.n, dtype=bool)
    for r in range(rounds):
        mate, initiator = fu.pair_matching(g, seed_at(r), r)
        pairs += int(np.count_nonzero(initiator))
        fired |= mate >= 0
    return pairs, int(g.n - np.count_nonzero(fired))


def _lossy_lost(E, rounds, down=None, masked_rounds=()):
    """Messages lost in rounds 1 .. rounds-1 at (LOSS, SEED), from fu.lossy_delivered alone; the
    slots of `down` count as lost in `masked_rounds`."""
    lost = 0
    for r in range(1, rounds):
        d = fu.lossy_delivered(SEED, r, 0, E, LOSS) != 0
        if r in masked_rounds:
            d &= np.asarray(down) == 0
        lost += int(np.count_nonzero(~d))
    return lost


# ------------------------------------------------------------------------------------
# the seven handles
# ------------------------------------------------------------------------------------
class _CollectAll:
    window = 20  # rounds of the benchmark's window

    def __init__(self, kernel):
        self.kernel = kernel
        self.id = f"collectall-{kernel}"

    def graph(self):
        return _ca_graph()

    def values(self):
        return _ca_refs("sym", 3)[0]

    def make(self):
        return fu.CollectAll(self.graph(), self.values(), kernel=self.kernel)

    def state(self, eng):
        return {"estimates": eng.estimates(), "flows": eng.flows()}

    def ref(self, r):
        a, f = _ca_refs("sym", 3)[1][r]
        return {"estimates": a, "flows": f}

    def targets(self):
        g = self.graph()
        return fu.component_means(g.rowptr, g.col, self.values())[0]

    def want_stats(self, rounds):
        return None


class _Batch(_CollectAll):
    id = "batch-K3"
    columns = (("sym", 3), ("wide", 3), ("sym", 5))

    def __init__(self):
        pass

    def values(self):
        return np.stack([_ca_refs(*c)[0] for c in self.columns], axis=1)

    def make(self):
        return fu.CollectAllBatch(self.graph(), self.values())

    def ref(self, r):
        return {"estimates": np.stack([_ca_refs(*c)[1][r][0] for c in self.columns], axis=1),
                "flows": np.stack([_ca_refs(*c)[1][r][1] for c in self.columns], axis=1)}

    def targets(self):
        g = self.graph()
        return np.stack([fu.component_means(g.rowptr, g.col, _ca_refs(*c)[0])[0] for c in self.columns], axis=1)


class _Lossy(_CollectAll):
    id = "lossy-p0.25"

    def __init__(self):
        pass

    def make(self):
        return fu.CollectAllLossy(self.graph(), self.values(), loss=LOSS, seed=SEED)

    def ref(self, r):
        a, f = _lossy_ref(r)
        return {"estimates": a, "flows": f}

    def want_stats(self, rounds):
        E = self.graph().E
        return E * (rounds - 1), _lossy_lost(E, rounds)


class _Pair(_CollectAll):
    window = 17

    def __init__(self, match):
        self.match = match
        self.id = f"pair-match{match}"

    def graph(self):
        return class_graph()

    def values(self):
        return _pair_values()

    def make(self):
        eng = fu.PairwiseSync(self.graph(), self.values(), seed=SEED)
        eng.set_option("match", self.match)
        return eng

    def state(self, eng):
        return {"estimates": eng.estimates(), "flows": eng.flows(), "cache": eng.cache()}

    def ref(self, r):
        last, f, c = _pair_ref(r)
        return {"estimates": last, "flows": f, "cache": c}

    def want_stats(self, rounds):
        return _pair_stats(self.graph(), lambda r: SEED, rounds)


CASES = [_CollectAll("recon"), _CollectAll("stage"), _CollectAll("pregather"), _Batch(), _Lossy(), _Pair(0), _Pair(1)]
every_engine = pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])


def _check(case, eng, r, what):
    assert eng.rounds_done == r, (case.id, what, eng.rounds_done, r)
    got, ref = case.state(eng), case.ref(r)
    for name in ref:
        assert_same_bits(got[name], ref[name], (case.id, what, "round", r, name))


def _want_err(case, r):
    """max_i |a_i - target_i| after r rounds, per column for the batch: the oracle's doubles."""
    return np.max(np.abs(case.ref(r)["estimates"] - case.targets()), axis=0)


# ------------------------------------------------------------------------------------
# 1. the first rounds, one timed call each
# ------------------------------------------------------------------------------------
@every_engine
def test_five_timed_calls_of_one_round(case):
    """From a fresh handle run_timed(1) five times: the calls begin at rounds 0, 1, 2, 3 and 4,
    so each must pick round 0, the rounds that compute the old flows instead of reading them
    (rounds 1 and 2 of the collect-all engines), and the steady state, on its own. Reading the
    flows after round 0 writes them to memory, which a round 1 that wrongly read them would then
    find: a second handle runs the first three calls with nothing read in between."""
    eng = case.make()
    for r in range(1, 6):
        _timed(eng, 1)
        _check(case, eng, r, "run_timed(1) x 5")
    eng.close()
    eng = case.make()
    for r in range(1, 4):
        _timed(eng, 1)
    _check(case, eng, 3, "run_timed(1) x 3, unread")
    eng.close()


def test_five_timed_calls_of_one_round_kernel_auto():
    """The same with kernel "auto" (no call is long enough for an autotune pass; which kernel
    runs is not asserted)."""
    case = _CollectAll("auto")
    eng = case.make()
    for r in range(1, 6):
        _timed(eng, 1)
        _check(case, eng, r, "run_timed(1) x 5")
    eng.close()


# ------------------------------------------------------------------------------------
# 2. the window the benchmark tools time
# ------------------------------------------------------------------------------------
@every_engine
def test_benchmark_window_twice(case):
    """reset(); run(1); synchronize(); run_timed(R - 1), as window_us does in tools/bench_batch.py,
    bench_lossy.py and bench_pair.py, twice on one handle: the second window starts from a reset
    of a handle that has run. R = 20 (the tools' default), 17 for the pairwise engine."""
    R = case.window
    eng = case.make()
    for window in range(2):
        eng.reset()
        eng.run(1)
        eng.synchronize()
        _timed(eng, R - 1)
        _check(case, eng, R, ("window", window))
    want = case.want_stats(R)
    if want is not None:
        assert eng.stats == want  # counted since the last reset
    eng.close()


# ------------------------------------------------------------------------------------
# 3. plain and timed calls mixed
# ------------------------------------------------------------------------------------
@every_engine
def test_plain_and_timed_calls_mixed(case):
    """run(3); run_timed(4); run(2, err_every=1); run_timed(0); run_timed(8): the oracle's bits
    after 3, 7, 9, 9 and 17 rounds, the two error entries, and for the lossy and pairwise engines
    the counters over the 17 rounds (the timed rounds feed their absolute round to the hash:
    messages offered and lost from fu.lossy_delivered, pairs and idle nodes from
    fu.pair_matching)."""
    eng = case.make()
    eng.set_targets(case.targets())
    eng.run(3)
    _check(case, eng, 3, "run(3)")
    _timed(eng, 4)
    _check(case, eng, 7, "run_timed(4)")
    trace = eng.run(2, err_every=1)
    assert_same_bits(trace, np.stack([_want_err(case, 8), _want_err(case, 9)]), (case.id, "error trace"))
    _check(case, eng, 9, "run(2, err_every=1)")
    _timed(eng, 0)
    _check(case, eng, 9, "run_timed(0)")
    _timed(eng, 8)
    _check(case, eng, 17, "run_timed(8)")
    want = case.want_stats(17)
    if want is not None:
        assert eng.stats == want
    eng.close()


# ------------------------------------------------------------------------------------
# 4. lossy: a link mask set ahead of timed rounds
# ------------------------------------------------------------------------------------
def test_lossy_link_mask_set_between_run_and_run_timed():
    """Every link of the degree-2049 centre is down (both directions) in rounds 3-7, all of them
    timed rounds, and up again in the timed rounds 8-11."""
    g = _ca_graph()
    v = _ca_refs("sym", 3)[0]
    c = CLASS_EDGE_DEGREES.index(2049)
    down = np.zeros(g.E, dtype=np.uint8)
    down[g.rowptr[c]:g.rowptr[c + 1]] = 1
    down[g.rev[g.rowptr[c]:g.rowptr[c + 1]]] = 1
    plain, masked = hashed(LOSS, SEED, g.E), hashed(LOSS, SEED, g.E, down)
    a, f, _ = oracle_lossy(*g.arrays(), v, 12, lambda r: masked(r) if 3 <= r <= 7 else plain(r))
    assert not np.array_equal(a, _lossy_ref(12)[0])  # the outage shows in the reference
    with fu.CollectAllLossy(g, v, loss=LOSS, seed=SEED) as eng:
        eng.run(3)
        eng.set_link_mask(down)
        _timed(eng, 5)
        eng.set_link_mask(None)
        _timed(eng, 4)
        assert eng.rounds_done == 12
        assert_same_bits(eng.estimates(), a, "outage in timed rounds 3-7: estimates")
        assert_same_bits(eng.flows(), f, "outage in timed rounds 3-7: flows")
        assert eng.stats == (g.E * 11, _lossy_lost(g.E, 12, down, range(3, 8)))


# ------------------------------------------------------------------------------------
# 5. pairwise: a seed set ahead of timed rounds
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("match", [0, 1])
def test_pair_seed_set_between_run_and_run_timed(match):
    """Seed 3 for rounds 0-5 (run), seed 0 for 6-11 and seed 9 for 12-16 (both run_timed): the
    round counter is absolute, so timed round 12 is element 12 of seed 9's stream."""
    g = class_graph()
    v = _pair_values()

    def seed(r):
        return 3 if r < 6 else 0 if r < 12 else 9

    ref = oracle_pair(*g.arrays(), v, 17, seed)
    assert not np.array_equal(ref[0], oracle_pair(*g.arrays(), v, 17, 3)[0])
    with fu.PairwiseSync(g, v, seed=3) as eng:
        eng.set_option("match", match)
        eng.run(6)
        eng.set_seed(0)
        _timed(eng, 6)
        eng.set_seed(9)
        _timed(eng, 5)
        assert eng.rounds_done == 17
        for name, got, want in (("last", eng.estimates(), ref[0]), ("flows", eng.flows(), ref[1]),
                                ("cache", eng.cache(), ref[2])):
            assert_same_bits(got, want, ("three seeds", match, name))
        assert eng.stats == _pair_stats(g, seed, 17)


# ------------------------------------------------------------------------------------
# 6. CollectAll: packing plans scheduled by timed rounds
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["recon", "stage", "pregather"])
def test_timed_rounds_schedule_packing_plans(kernel):
    """The input of test_value_domain.test_packing_window_straddles_signed_zero (ER(20000, 80000),
    mixed-sign subnormals within 50 ulps of zero: the first plan already packs to 8 bits) with
    pack_every 1, in steps of run_timed(8) to round 32: the timed loop schedules the plans, so
    the tables are 8 bits wide at every stop, and the bits are the oracle's."""
    g = fu.Graph.erdos_renyi(20_000, 80_000, seed=1)
    v = FAMILIES["subn"](g.n, seed=1)
    eng = fu.CollectAll(g, v, kernel=kernel)
    eng.set_option("pack_every", 1)
    a = f = None
    for r in (8, 16, 24, 32):
        if a is None:
            a, f = coracle.ca_sync(*g.arrays(), v, 8, nthreads=16)
        else:
            coracle.ca_rounds(*g.arrays(), v, 8, a, f, nthreads=16)
        _timed(eng, 8)
        assert eng.rounds_done == r
        assert eng.pack_widths() == (8, 8, 8), (kernel, r)
        assert_same_bits(eng.estimates(), a, (kernel, r, "estimates"))
        assert_same_bits(eng.flows(), f, (kernel, r, "flows"))
    eng.close()


# ------------------------------------------------------------------------------------
# 7. fu_reset of a handle whose first autotune pass ran at a packed width
# ------------------------------------------------------------------------------------
def test_reset_of_a_handle_first_tuned_at_a_packed_width():
    """The graph of test_gpu_parity.test_reset_drops_a_width_pass_left_pending, kernel "auto",
    pack_every 4. Calls of 16 rounds are too short for an autotune pass, so the pass stays
    pending while the tables pack; the first long call then runs it at a packed width, and no
    winner for the unpacked width exists. (fu_set_option refuses "kernel" once a round has run,
    so the pass cannot be armed in mid-run through the option.)

    fu_reset returns to the unpacked tables. The packed width's winner must not stay in use there
    as if tuned for it: the handle is pending again with the pass count unchanged, the next long
    call runs exactly one pass, at width 0, and the bits are the oracle's."""
    g = fu.Graph.erdos_renyi(200_000, 800_000, seed=13)
    v = fu.uniform_values(g.n, seed=13)
    eng = fu.CollectAll(g, v)
    eng.set_option("pack_every", 4)
    for _ in range(60):
        eng.run(16)
        eng.synchronize()
        if eng.pack_widths()[2] > 0:
            break
    assert eng.pack_widths()[2] > 0
    info = eng.info()
    assert info["autotune"] == "pending" and info["tune_passes"] == 0
    for _ in range(8):
        eng.run(64)
        eng.synchronize()
        if eng.info()["autotune"] == "done":
            break
    info = eng.info()
    assert info["autotune"] == "done" and info["tune_passes"] >= 1
    assert info["tuned_pack_width"] > 0 and 0 not in info["tune_winner_by_width"], info
    passes = info["tune_passes"]
    eng.reset()
    info = eng.info()
    assert (info["autotune"], info["tune_passes"], info["tuned_pack_width"], info["rounds"]) == ("pending", passes, 0, 0)
    eng.run(64)
    eng.synchronize()
    info = eng.info()
    assert (info["autotune"], info["tune_passes"], info["tuned_pack_width"]) == ("done", passes + 1, 0)
    assert 0 in info["tune_winner_by_width"], info
    a_ref, f_ref = coracle.ca_sync(*g.arrays(), v, 64, nthreads=16)
    assert_same_bits(eng.estimates(), a_ref, "estimates")
    assert_same_bits(eng.flows(), f_ref, "flows")
    # and with the unpacked winner cached, the next reset is the cached case
    eng.reset()
    info = eng.info()
    assert (info["autotune"], info["tune_passes"]) == ("done", passes + 1)
    eng.close()
