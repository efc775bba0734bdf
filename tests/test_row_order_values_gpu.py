"""Rows that are not in ascending id order (order_cases.py) with the inputs and the call
sequences that test_row_order_gpu.py left on ascending rows: the value families that show a
reordered sum in the high bits (`wide`), in where a chain overflows (`huge`) and in the sign of
zero (`subn`) on every engine; the packed table with the families that pack, escapes and signed
zeros beside the cluster; autotune passes, which hand the lagged flows, the transposes and the
width cache from one kernel to the next; the error reduction and the timed entry points; and
eight ranks on the in-process transport.

Every comparison is by bit pattern against coracle on the reordered graph, or against the
engine's own restatement (lossy_reference, churn_python, oracle_pair, oracle_pair_loss), never
against another GPU run. The (case, order, family) triples come from order_cases.FAMILY_TRIPLES;
test_order_case_inputs.py asserts on the CPU what each family can detect on each of them. Every
reference is computed once and shared read-only."""
import functools

import numpy as np
import pytest

import fu
import order_cases as oc
from churn_cases import churn_python
from err_cases import ERR_R, oracle_rounds
from pack_cases import OracleRun
from pair_cases import SEED, oracle_pair
from pair_loss_cases import CLASS_P, LOSS_SEED, hashed, oracle_pair_loss
from parity_util import CLASS_EDGE_DEGREES, FAMILIES, assert_same_bits, count_neg_zero, planted_D, planted_targets
from rev_columns_cases import LOSS_SEED as REV_LOSS_SEED
from rev_columns_cases import Step, drive_churn, link_mask, lossy_reference
from test_row_order_gpu import KERNELS, LOSSY_P, LOSSY_STOPS, MAX_K, PAIR_ROUNDS, REV_CASES, _churn_script

pytestmark = pytest.mark.gpu

FAMS = oc.ORDER_FAMILIES
LAYOUTS = ["given", "degree"]


def _triples(*names):
    return [t for t in oc.FAMILY_TRIPLES if t[0] in names and t[2] in FAMS]


def _run_to_stops(eng, name, how, family, what):
    """Estimates and flows at every stop of (case, family); reading the flows between stops
    finalises the lagged flows, as in test_row_classes_on_reordered_rows."""
    ref = oc.reference(name, how, None, family)
    for stop in sorted(ref):
        eng.run(stop - eng.info()["rounds"])
        assert_same_bits(eng.estimates(), ref[stop][0], what + ("estimates", stop))
        assert_same_bits(eng.flows(), ref[stop][1], what + ("flows", stop))


# ------------------------------------------------------------------------------------
# 2. value families on reordered rows: the main engine
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name,how,family", _triples("class_edge", "c16", "pack_er"))
def test_main_engine_value_families(name, how, family, kernel, layout):
    """Every row class (class_edge), kernel 4's 2-byte offsets (c16) and the ER of the packing
    cases, reordered: 36 decades, overflowing chains and signed zeros summed in the caller's row
    order by kernels 4, 8 and 9, through the degree layout's readback too."""
    with fu.CollectAll(oc.graph(name, how), oc.values(name, family), kernel=kernel, layout=layout) as eng:
        _run_to_stops(eng, name, how, family, (name, how, family, kernel, layout))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name,how,family,mega", [t + (m,) for t in _triples("rmat_small", "rmat_large")
                                                  for m in ((64, oc.MEGA_HUB) if t[0] == "rmat_small" else (oc.MEGA_HUB,))])
def test_mega_hubs_value_families(name, how, family, mega, kernel, layout):
    """R-MAT rows above a lowered mega_hub and heavy rows above hub_threshold 32: rmat_small at
    mega_hub 64 and 300 (heavy rows only at 300), rmat_large at 300."""
    g = oc.graph(name, how)
    with fu.CollectAll(g, oc.values(name, family), kernel=kernel, hub_threshold=32, layout=layout) as eng:
        eng.set_option("mega_hub", mega)
        assert eng.info()["mega_hubs"] == int((g.degrees > mega).sum())
        _run_to_stops(eng, name, how, family, (name, how, family, mega, kernel, layout))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kernel,option", [("recon", "wave_heavy"), ("pregather", "lag")])
@pytest.mark.parametrize("family", FAMS)
def test_value_families_with_the_other_summing_path(family, kernel, option, layout):
    """wave_heavy 0 and lag 0 change which launch sums a row: each family once with either."""
    with fu.CollectAll(oc.graph("class_edge", "random"), oc.values("class_edge", family), kernel=kernel,
                       layout=layout) as eng:
        eng.set_option(option, 0)
        _run_to_stops(eng, "class_edge", "random", family, (family, kernel, option, layout))


# ------------------------------------------------------------------------------------
# 2. the batched engine: one family per column
# ------------------------------------------------------------------------------------
BATCH_COLUMNS = ("wide", "huge", "subn", "uniform")
BATCH_STOPS = tuple(sorted(set(oc.STOPS["batch_boundary"]) | set(oc.stops("batch_boundary", "huge"))))


def _batch_column_values(c):
    family = BATCH_COLUMNS[c % 4]
    n = oc.base_graph("batch_boundary").n
    if family == "uniform":
        return fu.uniform_values(n, seed=oc.VALUE_SEED["batch_boundary"] + c // 4)
    return FAMILIES[family](n, seed=oc.VALUE_SEED["batch_boundary", family] + c // 4)


@functools.lru_cache(maxsize=None)
def _batch_column(how, c):
    import coracle

    g, v = oc.graph("batch_boundary", how), _batch_column_values(c)
    out, done, a, f = {}, 0, None, None
    for stop in BATCH_STOPS:
        if a is None:
            a, f = coracle.ca_sync(*g.arrays(), v, stop, nthreads=8)
        else:
            coracle.ca_rounds(*g.arrays(), v, stop - done, a, f, nthreads=8)
        done = stop
        out[stop] = (a.copy(), f.copy())
    return v, out


@pytest.mark.parametrize("K", [3, 16])
@pytest.mark.parametrize("how", oc.GPU_HOWS["batch_boundary"])
def test_batch_columns_of_different_families(how, K):
    """Column c carries wide, huge, subn or uniform values (c mod 4) over the reordered batch
    boundary graph. Each column equals an oracle run of its own, and a NaN of a huge column stays
    in its column: every other column is finite at every stop while the huge ones hold NaN."""
    cols = [_batch_column(how, c) for c in range(K)]
    V = np.ascontiguousarray(np.stack([v for v, _ in cols], axis=1))
    huge = [c for c in range(K) if BATCH_COLUMNS[c % 4] == "huge"]
    with fu.CollectAllBatch(oc.graph("batch_boundary", how), V) as eng:
        for stop in BATCH_STOPS:
            eng.run(stop - eng.rounds_done)
            a, f = eng.estimates(), eng.flows()
            for c, (_, ref) in enumerate(cols):
                assert_same_bits(np.ascontiguousarray(a[:, c]), ref[stop][0], (how, K, "column", c, "estimates", stop))
                assert_same_bits(np.ascontiguousarray(f[:, c]), ref[stop][1], (how, K, "column", c, "flows", stop))
                if c not in huge:
                    assert np.isfinite(a[:, c]).all() and np.isfinite(f[:, c]).all(), (how, K, c, stop)
        assert all(np.isnan(a[:, c]).any() for c in huge)


# ------------------------------------------------------------------------------------
# 2. the rev-gather round: lossy and churn
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rev_columns(name, family, K=MAX_K):
    n = oc.base_graph(name).n
    return np.ascontiguousarray(np.stack([FAMILIES[family](n, seed=oc.VALUE_SEED[name, family] + c) for c in range(K)],
                                         axis=1))


@functools.lru_cache(maxsize=None)
def _lossy_reference(name, how, family):
    g = oc.graph(name, how)
    down = link_mask(g, 0.1, 7)
    return down, lossy_reference(g, _rev_columns(name, family), LOSSY_STOPS, LOSSY_P, REV_LOSS_SEED, down)


@pytest.mark.parametrize("K", [1, MAX_K])
@pytest.mark.parametrize("family", FAMS)
@pytest.mark.parametrize("name,how", REV_CASES)
def test_lossy_columns_value_families(name, how, family, K):
    """p = 0.3 and the link mask of test_lossy_columns_on_reordered_rows: a lost slot keeps the
    node's own pair (the kOwn slot kind) in its place in the chain, beside +-inf under `huge`
    and -0.0 under `subn`."""
    down, ref = _lossy_reference(name, how, family)
    V = np.ascontiguousarray(_rev_columns(name, family)[:, :K])
    with fu.CollectAllLossyBatch(oc.graph(name, how), V, loss=LOSSY_P, seed=REV_LOSS_SEED) as eng:
        eng.set_link_mask(down)
        for stop in LOSSY_STOPS:
            eng.run(stop - eng.rounds_done)
            what = (name, how, family, K, stop)
            assert_same_bits(eng.estimates(), np.ascontiguousarray(ref[stop][0][:, :K]), what + ("estimates",))
            assert_same_bits(eng.flows(), np.ascontiguousarray(ref[stop][1][:, :K]), what + ("flows",))
        assert eng.stats[1] > 0


@functools.lru_cache(maxsize=None)
def _churn_column(name, how, family, c):
    g = oc.graph(name, how)
    return churn_python(*g.arrays(), _rev_columns(name, family)[:, c], _churn_script(g)).steps


def _churn_steps(name, how, family, K, script):
    per = [_churn_column(name, how, family, c) for c in range(K)]
    return [Step(np.stack([p[q].a for p in per], axis=1), np.stack([p[q].f for p in per], axis=1), per[0][q].state,
                 per[0][q].alive_nodes, per[0][q].live_slots) for q in range(len(script))]


@pytest.mark.parametrize("K", [1, MAX_K])
@pytest.mark.parametrize("family", FAMS)
@pytest.mark.parametrize("name,how", REV_CASES)
def test_churn_columns_value_families(name, how, family, K):
    """The mid-row slot of every heavy row DOWN (the kSkip slot kind inside a reordered chain),
    then FRESH, under each family, against the rule on Python floats column by column."""
    g = oc.graph(name, how)
    script = _churn_script(g)
    V = np.ascontiguousarray(_rev_columns(name, family)[:, :K])
    with fu.CollectAllChurnBatch(g, V) as eng:
        drive_churn(eng, script, _churn_steps(name, how, family, K, script), (name, how, family, K))


# ------------------------------------------------------------------------------------
# 2. the pair engine
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair_reference(name, how, family, p, rounds):
    g, v = oc.graph(name, how), oc.values(name, family)
    if p == 0.0:
        return oracle_pair(*g.arrays(), v, rounds, SEED)[:3]
    return oracle_pair_loss(*g.arrays(), v, rounds, SEED, hashed(p, LOSS_SEED, g.E))[:3]


def _check_pair(eng, name, how, family, p, r, what):
    ref = _pair_reference(name, how, family, p, r)
    assert_same_bits(eng.estimates(), ref[0], what + ("round", r, "last"))
    assert_same_bits(eng.flows(), ref[1], what + ("round", r, "flows"))
    assert_same_bits(eng.cache(), ref[2], what + ("round", r, "cache"))


@pytest.mark.parametrize("p", [0.0, CLASS_P])
@pytest.mark.parametrize("match", [0, 1])
@pytest.mark.parametrize("name,how,family", _triples("pair_class", "dense66"))
def test_pairs_value_families(name, how, family, match, p):
    """Both matchers, lossless and at p = 0.3: a fire sums the row's flows in row order (light
    lane groups and the heavy block's chunks) on each family."""
    with fu.PairwiseSync(oc.graph(name, how), oc.values(name, family), seed=SEED, loss=p,
                         loss_seed=LOSS_SEED if p else 0) as eng:
        eng.set_option("match", match)
        for r in PAIR_ROUNDS[name]:
            eng.run(r - eng.rounds_done)
            _check_pair(eng, name, how, family, p, r, (name, how, family, "match", match, "p", p))


# ------------------------------------------------------------------------------------
# 2. and 6. partitions on the in-process transport: worlds 2, 3 and 8
# ------------------------------------------------------------------------------------
CUT_KERNELS = [("cut_slivers", "recon"), ("cut_slivers", "stage"), ("cut_rmat", "recon"), ("cut_rmat", "stage"),
               ("cut_rmat", "pregather")]


def _open_cut(name, how, family, kernel, world):
    """(plans, handles) of the reordered cut at cut_bounds(name, world) with the case's options;
    a rank that has no layout for the kernel refuses it and runs kernel 4 (test_dist_cuts_gpu)."""
    from fu.dist import DistCollectAll, partition
    from test_dist_cuts_gpu import no_layout

    g, v, options = oc.graph(name, how), oc.values(name, family), oc.cut_options(name)
    bounds = oc.cut_bounds(name, world)
    plans = [partition(g.rowptr, g.col, g.rev, world, r, bounds=bounds) for r in range(world)]
    engs = []
    try:
        for p in plans:
            e = DistCollectAll(p, v[p.lo:p.hi], None)
            engs.append(e)
            for key, val in options.items():
                fu._lib.call("fu_set_option", e._h, key.encode(), val)
            why = no_layout(p, kernel, options)
            if why is None:
                fu._lib.call("fu_set_option", e._h, b"kernel", fu.engine.KERNELS[kernel])
            else:
                with pytest.raises(fu.FuError, match=why):
                    fu._lib.call("fu_set_option", e._h, b"kernel", fu.engine.KERNELS[kernel])
        assert kernel in [e.info()["kernel"] for e in engs]
    except BaseException:
        for e in engs:
            e.close()
        raise
    return plans, engs


def _check_cut(g, plans, engs, a_ref, f_ref, what):
    for p, e in zip(plans, engs):
        assert_same_bits(e.estimates(), np.ascontiguousarray(a_ref[p.lo:p.hi]), what + ("rank", p.rank, "estimates"))
        assert_same_bits(e.flows(), np.ascontiguousarray(f_ref[g.rowptr[p.lo]:g.rowptr[p.hi]]),
                         what + ("rank", p.rank, "flows"))


def _run_cut(name, how, family, kernel, world, after_reset=False):
    from fu.dist import run_local

    g = oc.graph(name, how)
    ref = oc.reference(name, how, None, family)
    plans, engs = _open_cut(name, how, family, kernel, world)
    try:
        for turn in range(2 if after_reset else 1):
            done = 0
            for stop in sorted(ref):
                run_local(engs, stop - done)
                done = stop
                _check_cut(g, plans, engs, *ref[stop], (name, family, kernel, world, "turn", turn, "stop", stop))
            for e in engs:
                e.reset()
    finally:
        for e in engs:
            e.close()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,how,family,kernel", [t + (k,) for t in _triples("cut_slivers", "cut_rmat")
                                                    for n, k in CUT_KERNELS if n == t[0]])
def test_partitions_value_families(name, how, family, kernel, world):
    """The two reordered cuts at uneven bounds, under every order and family of the table: the
    halo carries 36 decades, infinities and NaN, and signed zeros into the ghost slots, and every
    rank's slice equals the single-graph oracle's at the family's stops."""
    _run_cut(name, how, family, kernel, world)


@pytest.mark.parametrize("name,how,kernel,family",
                         [(n, h, k, "uniform") for n, k in CUT_KERNELS for h in oc.GPU_HOWS[n]]
                         + [(n, h, "recon", "wide") for n, h, f in _triples("cut_slivers", "cut_rmat") if f == "wide"])
def test_eight_ranks_on_reordered_rows(name, how, kernel, family):
    """Eight handles in one process at the cases' own bounds (slivers of 1, 2, 63, 64, 65 and 257
    rows; hub-only leading ranks), under both orders of each cut: stops 1, 2, 3, 4, 7 and 20, and
    again after a reset. Uniform values on every kernel, `wide` once per cut and order (kernel 4)."""
    _run_cut(name, how, family, kernel, 8, after_reset=True)


# ------------------------------------------------------------------------------------
# 3. the packed table with the families that pack
# ------------------------------------------------------------------------------------
def _packed_run(family, extras, kernel):
    from parity_util import PACK_WIDTHS

    g, v = oc.pack_graph(family, extras)
    refs = oc.pack_reference(family, extras)
    with fu.CollectAll(g, v, kernel=kernel) as eng:
        eng.set_option("pack_every", 4)
        seen = set()
        for r in oc.pack_stops(family, extras):
            eng.run(r - eng.info()["rounds"])
            seen.update(eng.pack_widths())
            assert_same_bits(eng.estimates(), refs[r][0], (family, extras, kernel, r, "estimates"))
            assert_same_bits(eng.flows(), refs[r][1], (family, extras, kernel, r, "flows"))
        assert PACK_WIDTHS[family] <= seen, (family, extras, kernel, seen)  # a run that never packed fails


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("family", oc.PACK_FAMILIES)
def test_packed_families_on_reordered_rows(family, kernel):
    """pack_er with shuffled rows, centred on negative values, on both signs and on the binade
    boundary at 1.0, with +-inf, NaN, -0.0, +-5e-324 and 1.7e308 in small components beside it:
    a gather of those takes the escape code and reads the double at the slot's own column. At
    the case's stops and with the table at 32, 16 and 8 bits (parity_util.PACK_STOPS; the
    widths are asserted, and test_pack_family_inputs_reach_every_width gives them from the
    plan's rule on the CPU)."""
    _packed_run(family, "nonfinite", kernel)


@pytest.mark.parametrize("kernel", KERNELS)
def test_packed_family_with_finite_extras(kernel):
    """The finite components (-0.0, +-5e-324, a triangle of 3, -7 and 1e-300) beside `neg`."""
    _packed_run("neg", "finite", kernel)


@pytest.mark.parametrize("kernel", KERNELS)
def test_packed_escapes_keep_the_sign_of_zero(kernel):
    """order_cases.SIGNED_ZERO_EXTRAS beside `neg`: components whose flows depend on the sign of
    the zero that the escape code's reader gathers, at every width and one and two rounds past
    the last stop. (A reader that returned a_prev[j] + 0.0 for an escape passed every other
    case of the suite; DESIGN 4.21, wrong variant b.)"""
    _packed_run("neg", "signed_zero", kernel)


@functools.lru_cache(maxsize=None)
def _straddle_refs():
    run = OracleRun(oc.graph("pack_er", "random"), oc.straddle_values(), nthreads=8)
    return {r: run.after(r) for r in oc.STRADDLE_STEPS}


@pytest.mark.parametrize("kernel", KERNELS + ["auto"])
def test_packing_window_straddles_signed_zero_on_reordered_rows(kernel):
    """test_packing_window_straddles_signed_zero on shuffled rows: the first plan packs to 8 bits
    with -0.0 and +0.0 inside the window, and the split-word flow store sees flips of the high
    word alone."""
    refs = _straddle_refs()
    with fu.CollectAll(oc.graph("pack_er", "random"), oc.straddle_values(), kernel=kernel) as eng:
        eng.set_option("pack_every", 2)
        for r in oc.STRADDLE_STEPS:
            a_ref, f_ref = refs[r]
            assert count_neg_zero(a_ref) > 0 and count_neg_zero(f_ref) > 0, r
            eng.run(r - eng.info()["rounds"])
            assert eng.pack_widths() == (8, 8, 8), (kernel, r)
            assert_same_bits(eng.estimates(), a_ref, (kernel, r, "estimates"))
            assert_same_bits(eng.flows(), f_ref, (kernel, r, "flows"))


# ------------------------------------------------------------------------------------
# 4. tuning passes
# ------------------------------------------------------------------------------------
KERNEL_OF_CANDIDATE = {"recon": 4, "recon_512": 4, "recon_1024": 4, "stage": 8, "pregather": 9}
AFTER_PASS = (0, 1, 2, 9)


STAND_IN_US = 1e20  # a partitioned pass reports 1e30 ms for a stand-in: kernel 4 ran its rounds


def _kernels_of_the_pass(info):
    """The kernels that ran rounds in the last pass: fu_get_info's time per round, 0 = not run,
    a stand-in's 1e30 ms not counted for the candidate it stood in for."""
    return {KERNEL_OF_CANDIDATE[c] for c, us in info["tune_us_per_round"].items() if 0 < us < STAND_IN_US}


def _check_after_pass(eng, oracle, what):
    """Right after a pass and 1, 2 and 9 rounds later; at least two kernels ran rounds in it."""
    assert len(_kernels_of_the_pass(eng.info())) >= 2, (what, eng.info())
    at = eng.info()["rounds"]
    for more in AFTER_PASS:
        eng.run(at + more - eng.info()["rounds"])
        a_ref, f_ref = oracle.after(at + more)
        assert_same_bits(eng.estimates(), a_ref, what + ("pass ended at", at, "+", more, "estimates"))
        assert_same_bits(eng.flows(), f_ref, what + ("pass ended at", at, "+", more, "flows"))


@pytest.mark.parametrize("before", [1, 3])
@pytest.mark.parametrize("how", oc.GPU_HOWS["rmat_large"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_tuning_pass_hands_over_on_reordered_rows(layout, how, before):
    """kernel "auto" on the reordered R-MAT with heavy rows and mega hubs: fu_tune after 1 or 3
    rounds runs kernels 4, 8 and 9 in turn on the running state (the lagged flows F[r & 1],
    kernel 9's transposes and buckets), and the state after the pass and 1, 2 and 9 rounds later
    is the oracle's. Under the degree layout the hand-over passes through the relabelling."""
    g, v = oc.graph("rmat_large", how), oc.values("rmat_large")
    oracle = OracleRun(g, v, nthreads=8)
    with fu.CollectAll(g, v, hub_threshold=32, layout=layout) as eng:
        eng.set_option("mega_hub", oc.MEGA_HUB)
        assert eng.info()["autotune"] == "pending" and eng.info()["mega_hubs"] > 0
        eng.run(before)
        assert_same_bits(eng.flows(), oracle.after(before)[1], (layout, how, before, "flows before the pass"))
        eng.tune()
        assert eng.info()["autotune"] == "done" and eng.info()["rounds"] > before
        _check_after_pass(eng, oracle, (layout, how, before))


def test_tuning_passes_and_the_width_cache_on_reordered_rows():
    """pack_er with shuffled rows, pack_every 4: one pass on the unpacked table, one after the
    table has reached 8 bits (test_autotune_width_cache_across_reset_bitwise's sequence, with the
    passes called), each followed by the oracle's bits; then fu_reset, which keeps both winners,
    and the first rounds again, unpacked, on the cached winner."""
    g, v = oc.graph("pack_er", "random"), oc.values("pack_er")
    oracle = OracleRun(g, v, nthreads=8)
    with fu.CollectAll(g, v) as eng:
        eng.set_option("pack_every", 4)
        eng.run(3)
        eng.tune()
        assert eng.info()["tuned_pack_width"] == 0
        _check_after_pass(eng, oracle, ("unpacked",))
        for _ in range(40):  # the host sees each plan's width once the stream has passed it
            eng.run(16)
            eng.synchronize()
            if eng.pack_widths() == (8, 8, 8):
                break
        assert eng.pack_widths() == (8, 8, 8), (eng.info()["rounds"], eng.pack_widths())
        eng.tune()
        info = eng.info()
        assert info["tuned_pack_width"] == 8 and {0, 8} <= set(info["tune_winner_by_width"]), info
        _check_after_pass(eng, oracle, ("8 bits",))
        passes = eng.info()["tune_passes"]
        eng.reset()
        again = OracleRun(g, v, nthreads=8)
        for r in (1, 2, 3, 9, 40):
            eng.run(r - eng.info()["rounds"])
            a_ref, f_ref = again.after(r)
            assert_same_bits(eng.estimates(), a_ref, ("after the reset", r, "estimates"))
            assert_same_bits(eng.flows(), f_ref, ("after the reset", r, "flows"))
        assert eng.info()["tune_passes"] == passes  # width 0's winner was cached


def test_partitioned_tuning_pass_on_a_reordered_cut():
    """The partitioned pass (FP::tune_steps with dist set: no candidate dropped, kernel 9 never a
    candidate) on cut_rmat with shuffled rows. A pass needs many rounds in one call and the
    in-process transport runs one at a time, so this is one RCCL rank, as in
    test_dist_autotune_never_runs_kernel_9; a pass across two ranks needs two GPUs."""
    from fu.dist import DistCollectAll, partition, unique_id

    name, how = "cut_rmat", oc.GPU_HOWS["cut_rmat"][0]
    g, v = oc.graph(name, how), oc.values(name)
    oracle = OracleRun(g, v, nthreads=8)
    d = DistCollectAll(partition(g.rowptr, g.col, g.rev, 1, 0), v, unique_id(), kernel="auto")
    try:
        for key, val in oc.cut_options(name).items():
            fu._lib.call("fu_set_option", d._h, key.encode(), val)
        d.run(2)
        assert d.info()["autotune"] == "pending"
        d.tune()
        info = d.info()
        assert info["autotune"] == "done" and info["tune_us_per_round"]["pregather"] == 0.0, info
        assert _kernels_of_the_pass(info) == {4, 8}, info
        at = info["rounds"]
        for more in AFTER_PASS:
            d.run(at + more - d.info()["rounds"])
            a_ref, f_ref = oracle.after(at + more)
            assert_same_bits(d.estimates(), a_ref, ("pass ended at", at, "+", more, "estimates"))
            assert_same_bits(d.flows(), f_ref, ("pass ended at", at, "+", more, "flows"))
    finally:
        d.close()


# ------------------------------------------------------------------------------------
# 5. the error reduction and the timed entry points
# ------------------------------------------------------------------------------------
PROBE_DEGREES = (0, 64, 255, 512, 1024, 4097, 12000)  # one centre per row class, the empty row included


@functools.lru_cache(maxsize=None)
def _err_case(family):
    g, v = oc.graph("class_edge", "random"), oc.values("class_edge", family)
    probes = [CLASS_EDGE_DEGREES.index(d) for d in PROBE_DEGREES] + [g.n - 1]
    return g, v, oracle_rounds(g.arrays(), v, ERR_R), probes


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kernel,family", [(k, "uniform") for k in KERNELS] + [("recon", "wide")])
def test_planted_error_trace_on_reordered_rows(kernel, family, layout):
    """max_i |a_i - target_i| per round with the argmax planted on one row of each class of the
    shuffled class-edge graph (parity_util.planted_targets): the device trace equals the
    oracle's by bit pattern, so each launch's rows contribute their own estimates; under the
    degree layout targets and estimates pass through the relabelling. Once on `wide`."""
    g, v, a_rounds, probes = _err_case(family)
    D = planted_D(a_rounds)
    with fu.CollectAll(g, v, kernel=kernel, layout=layout) as eng:
        for p in probes:
            t, want, runner_up = planted_targets(a_rounds, p, D)
            eng.reset()
            eng.set_targets(t)
            tr = eng.run(ERR_R, err_every=1)
            assert_same_bits(tr, want, (kernel, family, layout, f"probe {p}", f"without its row: {runner_up.tolist()}"))
        assert_same_bits(eng.estimates(), a_rounds[-1], (kernel, family, layout, "estimates"))


@pytest.mark.parametrize("bounds", [[0, 1, 7], [0, 3, 7]])
@pytest.mark.parametrize("how", oc.GPU_HOWS["rmat_large"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_marked_and_timed_rounds_on_reordered_rows(kernel, how, bounds):
    """fu_run_collectall_marked over rounds 0-6, then fu_run_collectall_timed for rounds 7-11,
    on the reordered R-MAT: the state of plain rounds after each."""
    ref = oc.reference("rmat_large", how, (7, 12))
    with fu.CollectAll(oc.graph("rmat_large", how), oc.values("rmat_large"), kernel=kernel, hub_threshold=32) as eng:
        eng.set_option("mega_hub", oc.MEGA_HUB)
        eng.run_marked(np.asarray(bounds, dtype=np.int32))
        eng.synchronize()
        assert all(eng.elapsed(k, k + 1) > 0.0 for k in range(len(bounds) - 1))
        assert_same_bits(eng.estimates(), ref[7][0], (kernel, how, bounds, "marked", "estimates"))
        assert_same_bits(eng.flows(), ref[7][1], (kernel, how, bounds, "marked", "flows"))
        assert eng.run_timed(5) > 0.0
        assert_same_bits(eng.estimates(), ref[12][0], (kernel, how, bounds, "timed", "estimates"))
        assert_same_bits(eng.flows(), ref[12][1], (kernel, how, bounds, "timed", "flows"))


@pytest.mark.parametrize("how", oc.GPU_HOWS["batch_boundary"])
def test_batch_timed_rounds_on_reordered_rows(how):
    """fu_batch_run_timed from each of the first rounds on: the columns of the family test."""
    K = 4
    cols = [_batch_column(how, c) for c in range(K)]
    V = np.ascontiguousarray(np.stack([v for v, _ in cols], axis=1))
    with fu.CollectAllBatch(oc.graph("batch_boundary", how), V) as eng:
        for stop in BATCH_STOPS:
            assert eng.run_timed(stop - eng.rounds_done) > 0.0
            a, f = eng.estimates(), eng.flows()
            for c, (_, ref) in enumerate(cols):
                assert_same_bits(np.ascontiguousarray(a[:, c]), ref[stop][0], (how, "column", c, "estimates", stop))
                assert_same_bits(np.ascontiguousarray(f[:, c]), ref[stop][1], (how, "column", c, "flows", stop))


@pytest.mark.parametrize("name,how", REV_CASES)
def test_lossy_and_churn_timed_rounds_on_reordered_rows(name, how):
    """fu_lossy_run_timed at p = 0.3 under the link mask, and fu_churn_run_timed through the DOWN
    and FRESH script, in place of the plain calls, on `wide` columns."""
    g = oc.graph(name, how)
    down, ref = _lossy_reference(name, how, "wide")
    V = _rev_columns(name, "wide")
    with fu.CollectAllLossyBatch(g, V, loss=LOSSY_P, seed=REV_LOSS_SEED) as eng:
        eng.set_link_mask(down)
        for stop in LOSSY_STOPS:
            assert eng.run_timed(stop - eng.rounds_done) > 0.0
            assert_same_bits(eng.estimates(), ref[stop][0], (name, how, "lossy", "estimates", stop))
            assert_same_bits(eng.flows(), ref[stop][1], (name, how, "lossy", "flows", stop))
    script = _churn_script(g)
    steps = _churn_steps(name, how, "wide", MAX_K, script)
    with fu.CollectAllChurnBatch(g, V) as eng:
        for q, s in enumerate(script):
            if s[0] == "run":
                assert eng.run_timed(s[1]) > 0.0
            else:
                eng.set_topology(s[1], s[2])
            assert_same_bits(eng.estimates(), steps[q].a, (name, how, "churn", "estimates", q))
            assert_same_bits(eng.flows(), steps[q].f, (name, how, "churn", "flows", q))
            assert np.array_equal(eng.slot_state(), steps[q].state), (name, how, "churn", "states", q)


@pytest.mark.parametrize("match", [0, 1])
@pytest.mark.parametrize("name,how", [(n, h) for n in ("pair_class", "dense66") for h in oc.GPU_HOWS[n]])
def test_pair_timed_rounds_on_reordered_rows(name, how, match):
    """fu_pair_run_timed at p = 0.3 on `wide` values, in place of the plain calls."""
    with fu.PairwiseSync(oc.graph(name, how), oc.values(name, "wide"), seed=SEED, loss=CLASS_P,
                         loss_seed=LOSS_SEED) as eng:
        eng.set_option("match", match)
        for r in PAIR_ROUNDS[name]:
            assert eng.run_timed(r - eng.rounds_done) > 0.0
            _check_pair(eng, name, how, "wide", CLASS_P, r, (name, how, "timed", "match", match))
