"""The device error reduction, max_i |a_i - target_i|, per row class, kernel, layout, launch
path and partition, bit for bit against values worked out from the C oracle alone.

The scalar engine has no error kernel of its own for rounds >= 1: every round launch carries
a CHECK branch (csrc/fu_ca_recon.h, fu_ca_stage.h, fu_ca_pregather.h: light tiles, heavy rows
per wave and per block, the mega-hub chain block, kernel 8's staged tiles, kernel 9's k_heavy_multi and k_isolated, the
PART boundary / interior launches of partitioned handles), each reducing its own rows into
one slot. With component means as targets nothing controls which row holds the maximum, so
a launch that drops its rows, or one that adds something it should not, goes unseen.

Planted targets (parity_util.planted_targets) control it: the targets are the oracle's last
estimates a_{R-1} except at one probe row p, where D is added, so at every round p alone
holds the maximum, the expected entry is np.max(np.abs(a_r - t)) on oracle data, and a
dropped contribution would show the runner-up instead (named in every failure message). One
more run per case plants nothing: its trace is max |a_r - a_{R-1}| and ends in +0.0, which
anything counted that should not be would raise. The conditions on the inputs (p alone at
the maximum at every round, D a power of two >= 4 max |a_r - a_{R-1}|) are checked on the
CPU in tests/test_parity_util.py.

R = 6 rounds: round 0 (k_max_err behind k_round0), rounds 1 and 2 (fm, the launches that
read no flows), generic rounds, both parities of kernel 9's lag. err_every > 0 keeps the
autotuner off, and every case pins its kernel.

Nothing was cut from the probes the cases were designed with; on the class-edge graph the
background has no row of degree 0, so the last rows of the degree order stand in for them
(err_cases.err_class_case). The inputs of every case are built in tests/err_cases.py."""
import ctypes

import numpy as np
import pytest

import fu
from err_cases import (ERR_BATCH_KS, ERR_DIST_HUB, ERR_DIST_MEGA, ERR_DIST_R, ERR_GRID, ERR_R, ERR_REDUCER_R, ERR_RMAT_HUB,
                       ERR_RMAT_MEGA, ISO_TAILS, err_batch_case, err_batch_nonfinite_rows, err_batch_trace_probes,
                       err_churn_reducer_case, err_class_case, err_dist_case, err_isolated_case, err_rccl_case,
                       err_rmat_case, err_scalar_reducer_case, with_decoys)
from parity_util import CLASS_EDGE_DEGREES, assert_same_bits, planted_D, planted_targets

pytestmark = pytest.mark.gpu

POS_ZERO = np.uint64(0)


def _is_pos_zero(x):
    return np.ascontiguousarray(x, dtype=np.float64).reshape(-1).view(np.uint64)[-1] == POS_ZERO


def _zero_trace(a_rounds):
    """The trace with nothing planted: max |a_r - a_{R-1}|, +0.0 at the last round."""
    return np.max(np.abs(a_rounds - a_rounds[-1]), axis=1)


def _check_probes(eng, a_rounds, probes, what):
    """The no-probe run, then one run per probe: reset, targets, R rounds with the check on
    every round, the whole trace against the oracle's."""
    rounds = len(a_rounds)
    D = planted_D(a_rounds)
    eng.reset()
    eng.set_targets(a_rounds[-1])
    tr = eng.run(rounds, err_every=1)
    assert_same_bits(tr, _zero_trace(a_rounds), what + ("no probe",))
    assert _is_pos_zero(tr), (what, "no probe: the last entry must be +0.0", tr[-1])
    assert_same_bits(eng.estimates(), a_rounds[-1], what + ("estimates",))
    for p in probes:
        t, want, runner_up = planted_targets(a_rounds, p, D)
        eng.reset()
        eng.set_targets(t)
        tr = eng.run(rounds, err_every=1)
        assert_same_bits(tr, want, what + (f"probe {p}", f"without its row: {runner_up.tolist()}"))


# ------------------------------------------------------------------------------------
# 1. row classes x kernel x layout (the fused check)
# ------------------------------------------------------------------------------------
CLASS_KERNELS = [("recon", {}), ("recon", {"wave_heavy": 0}), ("stage", {}), ("pregather", {}),
                 ("pregather", {"lag": 0}), ("pregather", {"multi_mid": 0}), ("pregather", {"iso_rows": 0}),
                 ("pregather", {"tr_nt": 0, "lag": 0}), ("pregather", {"multi_short": 0}),
                 ("pregather", {"multi_short": 1, "multi_heavy": 0})]


@pytest.mark.parametrize("layout", ["given", "degree"])
@pytest.mark.parametrize("kernel,opts", CLASS_KERNELS)
def test_row_classes_planted_trace(kernel, opts, layout):
    """Every first and last degree of every row class as the argmax (the 28 star centres, the
    empty row among them), node n-1, background rows and the rows the degree layout moves
    farthest, on test_row_class_boundaries_bitwise's kernels and options. Under layout
    "degree" the targets go in by caller id while the rows are relabelled on the device: a
    target that reaches the wrong row (invisible with component means on a connected
    component, where all targets are equal) changes every entry."""
    g, v, a_rounds, probes = err_class_case()
    eng = fu.CollectAll(g, v, kernel=kernel, layout=layout)
    for key, val in opts.items():
        eng.set_option(key, val)
    _check_probes(eng, a_rounds, probes, (kernel, tuple(opts.items()), layout))
    eng.close()


# ------------------------------------------------------------------------------------
# 2. isolated runs and what follows them (kernel 9, k_isolated)
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", ISO_TAILS)
@pytest.mark.parametrize("opts", [{}, {"iso_rows": 0}, {"lag": 0}])
def test_isolated_rows_planted_trace(tail, opts):
    """An isolated row's estimate is its value, and so is its component mean: only a planted
    target gives it an error, so only here can k_isolated's check decide an entry. The
    first, a middle and the last row of the isolated run, the heavy row and the mega hub
    beside it, and node 0."""
    g, v, a_rounds, probes = err_isolated_case(tail)
    eng = fu.CollectAll(g, v, kernel="pregather", layout="given")
    for key, val in opts.items():
        eng.set_option(key, val)
    _check_probes(eng, a_rounds, probes, (tail, tuple(opts.items())))
    eng.close()


@pytest.mark.parametrize("opts", [{}, {"iso_rows": 0}])
def test_isolated_rows_planted_trace_degree_layout(opts):
    """The same graph under layout "degree": the relabelling moves the 700 empty rows to the
    end of the device numbering whatever the tail, so k_isolated computes them and checks
    them against targets that came in by caller id (with iso_rows 0: light tiles)."""
    g, v, a_rounds, probes = err_isolated_case("heavy_hub")
    eng = fu.CollectAll(g, v, kernel="pregather", layout="degree")
    for key, val in opts.items():
        eng.set_option(key, val)
    _check_probes(eng, a_rounds, probes, ("degree", tuple(opts.items())))
    eng.close()


# ------------------------------------------------------------------------------------
# 3. tile geometry and thresholds (kernel 4)
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fork_heavy", [0, 1])
@pytest.mark.parametrize("wave_heavy", [0, 1])
@pytest.mark.parametrize("tile", [512, 1024, 2048])
def test_kernel4_geometries_planted_trace(tile, wave_heavy, fork_heavy):
    """R-MAT with hub_threshold 32 and mega_hub 300: mega hubs (k_hub_stage + chain block),
    heavy rows per wave or per block, light tiles of every geometry; with fork_heavy the heavy
    tiles run on the side stream and raise the same slot."""
    g, v, a_rounds, probes = err_rmat_case()
    eng = fu.CollectAll(g, v, kernel="recon", hub_threshold=ERR_RMAT_HUB)
    for key, val in (("mega_hub", ERR_RMAT_MEGA), ("tile_edges", tile), ("wave_heavy", wave_heavy),
                     ("fork_heavy", fork_heavy)):
        eng.set_option(key, val)
    assert eng.info()["mega_hubs"] >= 3
    _check_probes(eng, a_rounds, probes, (tile, wave_heavy, fork_heavy))
    eng.close()


# ------------------------------------------------------------------------------------
# 4. partitions
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,world,kernel", [("er", 2, "recon"), ("er", 2, "stage"), ("er", 3, "recon"),
                                               ("er", 3, "stage"), ("rmat", 2, "recon"), ("rmat", 2, "pregather"),
                                               ("rgg", 2, "recon"), ("rgg", 2, "stage"), ("rgg", 2, "pregather"),
                                               ("rgg", 3, "recon"), ("rgg", 3, "stage"), ("rgg", 3, "pregather")])
def test_partitions_planted_trace_local_transport(kind, world, kernel):
    """Partitioned handles with ghost slots (in-process transport), driven round by round with
    the check on: every rank plants one of its own rows (first, last, a row with a ghost
    column, its longest row, a mega hub at the cut) with its own D, and its entry is the
    maximum over its local rows only (the caller combines the ranks on this transport). The
    no-probe run is the one that a read of `target` at a ghost slot would raise.

    Boundary or interior is decided per light tile. ER and R-MAT have no locality: every
    light tile of every rank reads a ghost, and the interior launch (the second light launch
    of kernel 4 / 9's PART tiles and of launch_k8) has no tile. The random geometric cases
    are slabs: each rank has boundary and interior tiles in every geometry, and its
    "interior" row lies in an interior one (err_cases.err_dist_case; checked on the CPU by
    test_partition_probes_are_of_the_kind_they_name)."""
    from fu.dist import DistCollectAll

    g, v, a_rounds, plans, probes, D, _ = err_dist_case(kind, world)
    engs = [DistCollectAll(p, v[p.lo:p.hi], None, kernel=kernel) for p in plans]
    if kind == "rmat":
        for e in engs:
            for key, val in (("hub_threshold", ERR_DIST_HUB), ("mega_hub", ERR_DIST_MEGA)):
                fu._lib.call("fu_set_option", e._h, key.encode(), val)
        assert all(e.info()["mega_hubs"] > 0 for e in engs)
    assert all(e.info()["kernel"] == kernel for e in engs)
    arr = (ctypes.c_void_p * world)(*[e._h.value for e in engs])

    def traces(targets):
        for e, t in zip(engs, targets):
            e.reset()
            e.set_targets(t)
        out = np.empty((ERR_DIST_R, world))
        for r in range(ERR_DIST_R):
            for q, e in enumerate(engs):
                out[r, q] = e.run(1, err_every=1)[0]
            fu._lib.call("fu_dist_exchange_local", arr, world)
        return out

    local = [a_rounds[:, p.lo:p.hi] for p in plans]
    got = traces([a[-1] for a in local])
    for p, e in zip(plans, engs):
        what = (kind, world, kernel, "rank", p.rank, "no probe")
        assert_same_bits(np.ascontiguousarray(got[:, p.rank]), _zero_trace(local[p.rank]), what)
        assert _is_pos_zero(got[:, p.rank]), what
        assert_same_bits(e.estimates(), local[p.rank][-1], what + ("estimates",))
    for rows in probes:
        planted = [planted_targets(local[q], rows[q], D[q]) for q in range(world)]
        got = traces([t for t, _, _ in planted])
        for q in range(world):
            assert_same_bits(np.ascontiguousarray(got[:, q]), planted[q][1],
                             (kind, world, kernel, "rank", q, f"probe {rows[q]}",
                              f"without its row: {planted[q][2].tolist()}"))
    for e in engs:
        e.close()


def test_rccl_single_rank_planted_trace_and_max_err():
    """The all-reduce path (RCCL communicator at world size 1, the only size one GPU runs):
    the planted trace over R = 6 and fu_max_err with a planted target, by bits. The runs take
    milliseconds; the process's first RCCL communicator takes ~6 s to create, which the first
    test of a session that makes one pays (this one, when the whole suite runs)."""
    from fu.dist import DistCollectAll, partition, unique_id

    g, v, a_rounds, probes = err_rccl_case()
    plan = partition(g.rowptr, g.col, g.rev, 1, 0)
    d = DistCollectAll(plan, v, unique_id(), kernel="recon")

    def max_err():
        out = ctypes.c_double()
        fu._lib.call("fu_max_err", d._h, ctypes.byref(out))
        return np.array([out.value])

    _check_probes(d, a_rounds, probes, ("rccl",))  # leaves the state at a_{R-1}
    D = planted_D(a_rounds)
    d.set_targets(a_rounds[-1])
    assert _is_pos_zero(max_err())
    for p in probes:
        t, want, _ = planted_targets(a_rounds, p, D)
        d.set_targets(t)
        assert_same_bits(max_err(), want[-1:], ("rccl max_err", p))
    d.close()


# ------------------------------------------------------------------------------------
# 5. the stand-alone reducers: grids of min(1024, ...) blocks that stride over the rest
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["given", "degree"])
def test_fu_max_err_stride_loop(layout):
    """k_max_err on n = 300,000 > 1024 x 256: the argmax at the first and last thread of
    block 0, the first of block 1, either side of the first stride's end and at n-1. Three
    rounds run once; each probe only sets targets and reduces."""
    g, v, a_rounds, probes, new_of_old = err_scalar_reducer_case()
    if layout == "degree":  # by caller id, and at the caller ids that sit at these device indices
        old_of_new = np.argsort(new_of_old)
        probes = list(dict.fromkeys(probes + [int(old_of_new[q]) for q in probes]))
    eng = fu.CollectAll(g, v, kernel="recon", layout=layout)
    eng.run(ERR_REDUCER_R)
    assert_same_bits(eng.estimates(), a_rounds[-1], (layout, "estimates"))
    eng.set_targets(a_rounds[-1])
    assert _is_pos_zero(eng.max_err()), (layout, "no probe")
    D = planted_D(a_rounds)
    for p in probes:
        t, want, _ = planted_targets(a_rounds, p, D)
        eng.set_targets(t)
        assert_same_bits(np.array([eng.max_err()]), want[-1:], (layout, f"probe {p}"))
    eng.close()


def test_kc_max_err_stride_loop_skips_the_dead():
    """kc_max_err, the churn engine's reduction over the alive nodes, on n = 300,000 > 1024 x 256
    with a tenth of the nodes dead: the argmax at the probes of test_fu_max_err_stride_loop, one
    at a time, while a dead node of block 0, one of the last block of the first stride and one
    of the second stride each sit 2^20 D off their targets. The whole trace and max_err, by bits;
    then a NaN target on an alive node of the second stride, and NaN and inf on the dead."""
    g, v, alive, a_rounds, probes, decoys = err_churn_reducer_case()
    last, D = a_rounds[-1], planted_D(a_rounds)
    eng = fu.CollectAllChurn(g, v)
    eng.set_topology(alive, None)
    assert eng.stats[0] == int(alive.sum())
    eng.set_targets(with_decoys(last, last, decoys, D))
    tr = eng.run(ERR_REDUCER_R, err_every=1)
    assert_same_bits(tr, _zero_trace(a_rounds), "no probe, the decoys only")
    assert _is_pos_zero(tr) and _is_pos_zero(eng.max_err())
    assert_same_bits(eng.estimates(), last, "estimates")
    for p in probes:
        t, want, runner_up = planted_targets(a_rounds, p, D)
        eng.reset()
        eng.set_targets(with_decoys(t, last, decoys, D))
        tr = eng.run(ERR_REDUCER_R, err_every=1)
        assert_same_bits(tr, want, (f"probe {p}", f"without its row: {runner_up.tolist()}"))
        assert_same_bits(np.array([eng.max_err()]), want[-1:], (f"probe {p}", "max_err"))
    t, want, _ = planted_targets(a_rounds, probes[0], D)
    for bad in (np.nan, np.inf):
        for q in decoys:
            tq = with_decoys(t, last, decoys, D)
            tq[q] = bad
            eng.set_targets(tq)
            assert_same_bits(np.array([eng.max_err()]), want[-1:], (bad, "on the dead node", q))
    tq = with_decoys(t, last, decoys, D)
    tq[probes[4]] = np.nan
    assert probes[4] == ERR_GRID * 256 and alive[probes[4]]
    eng.set_targets(tq)
    assert_same_bits(np.array([eng.max_err()]), np.array([np.nan]), "NaN on an alive node of the second stride")
    eng.reset()
    eng.set_targets(tq)
    assert_same_bits(eng.run(ERR_REDUCER_R, err_every=1), np.full(ERR_REDUCER_R, np.nan), "NaN trace")
    eng.close()


def _stack_last(a_rounds):
    return np.stack([a[-1] for a in a_rounds], axis=1)


@pytest.mark.parametrize("K", ERR_BATCH_KS)
def test_kb_max_err_stride_loop_and_columns(K):
    """kb_max_err past one full grid, at K = 16 (tb = 256), 7 (tb = 252) and 3 (tb = 255: the
    threads from tb on stay idle, and a stride that is no multiple of K would mix columns):
    the planted column's entry is exact, every other column's is +0.0."""
    g, vs, a_rounds, probes, D = err_batch_case(K)
    last = _stack_last(a_rounds)
    eng = fu.CollectAllBatch(g, np.stack(vs, axis=1))
    eng.run(ERR_REDUCER_R)
    assert_same_bits(eng.estimates(), last, (K, "estimates"))
    eng.set_targets(last)
    assert_same_bits(eng.max_err(), np.zeros(K), (K, "no probe"))
    for i, c in probes:
        t, want, _ = planted_targets(a_rounds[c], i, D[c])
        T = last.copy()
        T[:, c] = t
        exp = np.zeros(K)
        exp[c] = want[-1]
        eng.set_targets(T)
        assert_same_bits(eng.max_err(), exp, (K, f"node {i}, column {c}"))
    eng.close()


def test_batch_planted_trace_one_probe_per_column():
    """run(R, err_every=1) at K = 7 with a probe in every column, each with its own D:
    (rounds / err_every) K slots, round-major (more than the K slots a handle starts with),
    each column against its own oracle run."""
    K = 7
    g, vs, a_rounds, _, D = err_batch_case(K)
    planted = [planted_targets(a_rounds[c], p, D[c]) for c, p in enumerate(err_batch_trace_probes(K, g.n))]
    eng = fu.CollectAllBatch(g, np.stack(vs, axis=1))
    eng.set_targets(_stack_last(a_rounds))
    tr = eng.run(ERR_REDUCER_R, err_every=1)
    assert tr.shape == (ERR_REDUCER_R, K)
    assert_same_bits(tr, np.stack([_zero_trace(a) for a in a_rounds], axis=1), "no probe")
    assert_same_bits(tr[-1], np.zeros(K), "no probe, last row")
    eng.reset()
    eng.set_targets(np.stack([t for t, _, _ in planted], axis=1))
    tr = eng.run(ERR_REDUCER_R, err_every=1)
    assert_same_bits(tr, np.stack([w for _, w, _ in planted], axis=1),
                     ("planted", "without the rows:", [r.tolist() for _, _, r in planted]))
    eng.close()


# ------------------------------------------------------------------------------------
# 6. NaN and inf as the planted value
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nonfinite_planted_target_scalar(bad):
    """t[p] = NaN at the mega hub and at the empty row: every entry is NaN (a NaN's pattern,
    sign cleared, is above +inf's in the uint64 order); t[p] = inf: +inf bits."""
    g, v, a_rounds, _ = err_class_case()
    hub, empty = len(CLASS_EDGE_DEGREES) - 1, 0
    assert g.degrees[hub] > 8192 and g.degrees[empty] == 0
    eng = fu.CollectAll(g, v, kernel="recon", layout="given")
    for p in (hub, empty):
        t = a_rounds[-1].copy()
        t[p] = bad
        want = np.max(np.abs(a_rounds - t), axis=1)
        assert_same_bits(want, np.full(ERR_R, bad))
        eng.reset()
        eng.set_targets(t)
        assert_same_bits(eng.run(ERR_R, err_every=1), want, (bad, p, "trace"))
        assert_same_bits(np.array([eng.max_err()]), want[-1:], (bad, p, "max_err"))
    eng.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nonfinite_planted_target_batched(bad):
    """The same at K = 7, at the longest row and at an empty row: NaN (or +inf) in the planted
    column only, the other columns' entries untouched."""
    K = 7
    g, hub, empty = err_batch_nonfinite_rows()
    _, vs, a_rounds, _, _ = err_batch_case(K)
    last = _stack_last(a_rounds)
    zero = np.stack([_zero_trace(a) for a in a_rounds], axis=1)
    eng = fu.CollectAllBatch(g, np.stack(vs, axis=1))
    for p, c in ((hub, 2), (empty, 5)):
        T = last.copy()
        T[p, c] = bad
        want = zero.copy()
        want[:, c] = bad
        eng.reset()
        eng.set_targets(T)
        assert_same_bits(eng.run(ERR_REDUCER_R, err_every=1), want, (bad, p, c, "trace"))
        assert_same_bits(eng.max_err(), want[-1], (bad, p, c, "max_err"))
    eng.close()
