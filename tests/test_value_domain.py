"""GPU parity over the fp64 value domain. tests/test_gpu_parity.py varies kernels, row
classes, tile geometries, packing widths, lag and partitions, but draws nearly every value
from [0, 100): one sign, one order of magnitude, no zero, nothing non-finite. Here the value
families of parity_util.FAMILIES (negative, mixed sign, 36 decades, small integers, one
binade boundary, mixed-sign subnormals, overflow to +-inf and NaN) go through every path,
compared with the C oracle by bit pattern (parity_util.assert_same_bits): the signs of zeros
and infinities count, and a NaN must sit exactly where the oracle has one.

The references are computed once per family and shared by the cases; no case changes them.

These cases prove the kernels equal to the oracle. That the oracle, and so the kernels, equal the
reference's own Peer code on such values (signed zeros, subnormals, overflow order, NaN placement)
is pinned in test_value_domain_golden.py (oracles against tests/golden/vd_*.npz, no GPU) and
test_value_domain_golden_gpu.py (every engine against those files directly)."""
import functools

import numpy as np
import pytest

import coracle
import fu
from parity_util import (FAMILIES, FINITE_EXTRAS, NONFINITE_EXTRAS, PACK_STOPS, PACK_WIDTHS, _class_edge_graph,
                         assert_same_bits, count_neg_zero)

pytestmark = pytest.mark.gpu

KERNELS = ["recon", "stage", "pregather"]


# ------------------------------------------------------------------------------------
# 1. row classes
# ------------------------------------------------------------------------------------
CLASS_STOPS = (1, 3, 8, 17)  # total rounds: round 0 alone, the last computed old flows (fm), steady state


@functools.lru_cache(maxsize=None)
def _class_graph():
    return _class_edge_graph(7)


@functools.lru_cache(maxsize=None)
def _class_refs(family):
    g = _class_graph()
    v = FAMILIES[family](g.n, seed=3)
    return v, {r: coracle.ca_sync(*g.arrays(), v, r, nthreads=16) for r in CLASS_STOPS}


def _check_row_classes(family, kernel, opts, layout):
    g = _class_graph()
    v, refs = _class_refs(family)
    eng = fu.CollectAll(g, v, kernel=kernel, layout=layout)
    for key, val in opts.items():
        eng.set_option(key, val)
    done = 0
    for r in CLASS_STOPS:
        eng.run(r - done)
        done = r
        assert_same_bits(eng.estimates(), refs[r][0], (family, kernel, layout, r, "estimates"))
        assert_same_bits(eng.flows(), refs[r][1], (family, kernel, layout, r, "flows"))
    eng.close()


@pytest.mark.parametrize("layout", ["given", "degree"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_row_classes_value_families(family, kernel, layout):
    """Rows of every class (degrees 0 ... 12000, one star per class boundary) on every value
    family, after 1, 3, 8 and 17 rounds. `huge` is the order test: a chain that adds its
    elements in another order overflows at another element, and the inf and the NaN that
    follows land at other positions."""
    _check_row_classes(family, kernel, {}, layout)


@pytest.mark.parametrize("layout", ["given", "degree"])
@pytest.mark.parametrize("family", ["subn", "wide"])
def test_row_classes_value_families_pregather_two_pass(family, layout):
    """Kernel 9 with lag off (the two-pass heavy rows) on the two families that exercise the
    sign of zero and the high bits."""
    _check_row_classes(family, "pregather", {"lag": 0}, layout)


def test_row_class_inputs_reach_the_edges():
    """A condition on the inputs of the cases above, from the oracle alone: `subn` reaches
    -0.0 in estimates and flows, `huge` reaches both infinities and NaN."""
    _, refs = _class_refs("subn")
    assert count_neg_zero(refs[17][0]) > 0 and count_neg_zero(refs[17][1]) > 0
    _, refs = _class_refs("huge")
    f3, a17 = refs[3][1], refs[17][0]
    assert np.isposinf(f3).any() and np.isneginf(f3).any() and np.isnan(a17).any()


# ------------------------------------------------------------------------------------
# 2. packing with the window straddling +-0
# ------------------------------------------------------------------------------------
STRADDLE_STEPS = tuple(range(8, 65, 8))


@functools.lru_cache(maxsize=None)
def _straddle_refs():
    g = fu.Graph.erdos_renyi(20_000, 80_000, seed=1)
    v = FAMILIES["subn"](g.n, seed=1)
    refs = {}
    a, f = coracle.ca_sync(*g.arrays(), v, STRADDLE_STEPS[0], nthreads=16)
    for r in STRADDLE_STEPS:
        refs[r] = (a.copy(), f.copy())
        coracle.ca_rounds(*g.arrays(), v, 8, a, f, nthreads=16)
    return g, v, refs


@pytest.mark.parametrize("kernel", KERNELS + ["auto"])
def test_packing_window_straddles_signed_zero(kernel):
    """Mixed-sign subnormals within 50 ulps of zero: every key lies within 51 of the fold
    between -0.0 (key 0x7fff...f) and +0.0 (key 0x8000...0), so the first plan (round 2, from
    a_1) already packs to 8 bits with a window that holds both zeros, and the split-word flow
    store sees flips between +0.0 and -0.0, which change the high word only. On this graph
    and seed the oracle's output holds 2256 ... 4567 estimates and 284 ... 1150 flows equal
    to -0.0 at the eight stops. Bit-equal to the oracle and to the unpacked run at each."""
    g, v, refs = _straddle_refs()
    eng = fu.CollectAll(g, v, kernel=kernel)
    eng.set_option("pack_every", 2)
    off = fu.CollectAll(g, v, kernel=kernel)
    off.set_option("pack", 0)
    for r in STRADDLE_STEPS:
        a_ref, f_ref = refs[r]
        assert count_neg_zero(a_ref) > 0 and count_neg_zero(f_ref) > 0, r  # the inputs reach -0.0
        eng.run(8)
        off.run(8)
        assert eng.pack_widths() == (8, 8, 8), (kernel, r)
        assert off.pack_widths() == (0, 0, 0), (kernel, r)
        a, f = eng.estimates(), eng.flows()
        assert_same_bits(a, a_ref, (kernel, r, "estimates"))
        assert_same_bits(f, f_ref, (kernel, r, "flows"))
        assert_same_bits(off.estimates(), a, (kernel, r, "estimates, pack 0"))
        assert_same_bits(off.flows(), f, (kernel, r, "flows, pack 0"))
    eng.close()
    off.close()


# ------------------------------------------------------------------------------------
# 3. packing on other signs and binades, non-finite values behind the escape code
# ------------------------------------------------------------------------------------
GIANT_N, GIANT_SEED = 20_000, 17


def _giant_with_extras(values, extras):
    """ER(20000, 80000) carrying `values`, plus one small component (a pair or a triangle)
    per entry of `extras`, carrying that entry's values."""
    g = fu.Graph.erdos_renyi(GIANT_N, 4 * GIANT_N, seed=GIANT_SEED)
    src = np.repeat(np.arange(g.n), np.diff(g.rowptr))
    keep = src < g.col
    s, d, v, k = [src[keep]], [g.col[keep]], [values], GIANT_N
    for comp in extras:
        m = len(comp)
        s.append(k + np.arange(m - 1))  # a path ...
        d.append(k + np.arange(1, m))
        if m == 3:  # ... closed to a triangle
            s.append([k])
            d.append([k + 2])
        v.append(np.array(comp, dtype=np.float64))
        k += m
    return fu.Graph.from_edges(k, np.concatenate(s), np.concatenate(d)), np.concatenate(v)


@functools.lru_cache(maxsize=None)
def _pack_refs(family):
    g, v = _giant_with_extras(FAMILIES[family](GIANT_N, seed=GIANT_SEED), NONFINITE_EXTRAS)
    refs, done = {}, 0
    a = f = None
    for r in PACK_STOPS[family]:
        if a is None:
            a, f = coracle.ca_sync(*g.arrays(), v, r, nthreads=16)
        else:
            coracle.ca_rounds(*g.arrays(), v, r - done, a, f, nthreads=16)
        done = r
        refs[r] = (a.copy(), f.copy())
    return g, v, refs


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("family", sorted(PACK_STOPS))
def test_packing_signs_binades_and_nonfinite_escapes(family, kernel):
    """The packed table centred on negative values, on values of both signs, on a cluster
    that spans the binade boundary at 1.0 and on a mean near 2^46, while six small components
    hold +-inf, NaN, -0.0, +-5e-324 and 1.7e308 (whose sums overflow): every gather of those
    takes the escape branch with a non-finite or signed-zero double behind it. Bit-equal at
    two stops on the way and at the end; the widths are those the plan's rule gives on the
    oracle's estimates (PACK_STOPS above)."""
    g, v, refs = _pack_refs(family)
    a_end = refs[PACK_STOPS[family][-1]][0]
    # the inputs: the giant component stays finite; beside it NaN (every inf has met its
    # opposite by then) and a -0.0
    assert np.isfinite(a_end[:GIANT_N]).all()
    assert np.isnan(a_end[GIANT_N:]).sum() == 9 and count_neg_zero(a_end[GIANT_N:]) == 1
    eng = fu.CollectAll(g, v, kernel=kernel)
    eng.set_option("pack_every", 4)
    seen, done = set(), 0
    for r in PACK_STOPS[family]:
        eng.run(r - done)
        done = r
        seen.update(eng.pack_widths())
        assert_same_bits(eng.estimates(), refs[r][0], (family, kernel, r, "estimates"))
        assert_same_bits(eng.flows(), refs[r][1], (family, kernel, r, "flows"))
    assert PACK_WIDTHS[family] <= seen, (family, kernel, seen)
    eng.close()


# ------------------------------------------------------------------------------------
# 4. the convergence check
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_error_trace_wide_values(kernel):
    """max |a - target| from the device (fu_run_collectall with err_every 1) on 36 decades of
    values of both signs: the trace's last entry after 1, 3, 10, 40 and 200 rounds is the
    oracle's np.max(np.abs(a - target)) bit for bit (the difference and fabs are exact
    operations on equal operands; the maximum is taken over bit patterns)."""
    g, v = _giant_with_extras(FAMILIES["wide"](GIANT_N, seed=GIANT_SEED), FINITE_EXTRAS)
    tgt, _ = fu.component_means(g.rowptr, g.col, v)
    assert np.isfinite(tgt).all()
    eng = fu.CollectAll(g, v, kernel=kernel)
    eng.set_targets(tgt)
    a = f = None
    done = 0
    for r in (1, 3, 10, 40, 200):
        tr = eng.run(r - done, err_every=1)
        assert len(tr) == r - done
        if a is None:
            a, f = coracle.ca_sync(*g.arrays(), v, r, nthreads=16)
        else:
            coracle.ca_rounds(*g.arrays(), v, r - done, a, f, nthreads=16)
        done = r
        want = np.max(np.abs(a - tgt))
        assert np.isfinite(want) and want > 0.0
        assert_same_bits(np.array([tr[-1], eng.max_err()]), np.array([want, want]), (kernel, r))
    assert_same_bits(eng.estimates(), a, kernel)
    eng.close()


# ------------------------------------------------------------------------------------
# 5. partitions
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _part_refs(family):
    g = fu.Graph.erdos_renyi(6_000, 24_000, seed=23)
    v = FAMILIES[family](g.n, seed=23)
    return g, v, coracle.ca_sync(*g.arrays(), v, 40, nthreads=16)


@pytest.mark.parametrize("kernel", ["recon", "stage"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("family", ["subn", "wide"])
def test_partitions_value_families(family, world, kernel):
    """Two and three ranks on the in-process transport: the halo carries signed zeros and
    subnormals (`subn`) and 36 decades (`wide`) into the ghost slots; 40 rounds, every rank's
    slice against the oracle."""
    from fu.dist import DistCollectAll, partition, run_local

    g, v, (a_ref, f_ref) = _part_refs(family)
    plans = [partition(g.rowptr, g.col, g.rev, world, r) for r in range(world)]
    assert all(p.n_ghost_a > 0 for p in plans)
    engs = [DistCollectAll(p, v[p.lo:p.hi], None, kernel=kernel) for p in plans]
    run_local(engs, 40)
    for p, e in zip(plans, engs):
        assert_same_bits(e.estimates(), a_ref[p.lo:p.hi], (family, world, kernel, p.rank, "estimates"))
        assert_same_bits(e.flows(), f_ref[g.rowptr[p.lo]:g.rowptr[p.hi]], (family, world, kernel, p.rank, "flows"))
    for e in engs:
        e.close()


# ------------------------------------------------------------------------------------
# 6. tick replay
# ------------------------------------------------------------------------------------
REPLAY_TICKS, REPLAY_SNAPS = 80, (25, 55, 79)


def _nan_inf(n, seed):
    """Uniform values with one quiet NaN and one inf among them."""
    v = np.random.default_rng(seed).random(n)
    v[n // 3] = np.nan
    v[2 * n // 3] = np.inf
    return v


REPLAY_FAMILIES = {"subn": FAMILIES["subn"], "wide": FAMILIES["wide"], "neg": FAMILIES["neg"],
                   "nan_inf": _nan_inf}


@functools.lru_cache(maxsize=None)
def _replay_trace(mode):
    g = fu.Graph.random_regular(4096, 8, seed=1)
    return fu.Trace(g.rowptr, g.col, mode, REPLAY_TICKS, "rand:3")


@functools.lru_cache(maxsize=None)
def _replay_refs(mode, family):
    tr = _replay_trace(mode)
    a = tr.arrays()
    v = REPLAY_FAMILIES[family](tr.n, seed=9)
    return v, coracle.replay(a["rowptr"], v, a["tick_task_off"], a["tasks"], a["events"], a["out_ids"],
                             tr.n_msgs, list(REPLAY_SNAPS))


@pytest.mark.parametrize("persistent", [False, True, "noreg"])
@pytest.mark.parametrize("mode", ["collectall", "pairwise"])
@pytest.mark.parametrize("family", sorted(REPLAY_FAMILIES))
def test_replay_value_families(family, mode, persistent):
    """80 ticks of the tick-level replay (tie order rand:3) on RR-4096, the per-tick batches
    and both persistent kernels: last averages, flows, estimate caches and three snapshots
    against the C oracle's replay. `nan_inf`: a quiet NaN and an inf spread from two nodes
    (messages carry them; the receive negates the flow)."""
    tr = _replay_trace(mode)
    v, (l_ref, f_ref, e_ref, s_ref) = _replay_refs(mode, family)
    if family == "nan_inf":
        assert np.isnan(l_ref).any() and np.isfinite(l_ref).any()
    rep = fu.Replay(tr, v, persistent=bool(persistent), registers=persistent != "noreg")
    snaps = rep.run(REPLAY_TICKS, snapshot_ticks=list(REPLAY_SNAPS))
    last, flows, est = rep.state()
    rep.close()
    what = (family, mode, persistent)
    assert_same_bits(last, l_ref, what + ("last",))
    assert_same_bits(flows, f_ref, what + ("flows",))
    assert_same_bits(est, e_ref, what + ("est",))
    for t in REPLAY_SNAPS:
        assert_same_bits(snaps[t], s_ref[t], what + ("snapshot", t))
