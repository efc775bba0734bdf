"""Tick replay parity on irregular graphs. The other replay tests run on random regular graphs
of degree <= 8 (and three fixtures of <= 12 nodes), the shapes the three kernels
(k_replay_tick, k_replay_persist, k_replay_persist_reg) were tuned on. Here: union degrees
9 ... 16 (the register kernel's 16-register instantiations), degree 17 and hubs (the fallback
to the generic persistent kernel), rows of different lengths side by side, isolated nodes,
asymmetric declarations, faults in collect-all mode, the value families, resumed runs, a
generic persistent launch of 1, 2 and 5 blocks (each thread owns several nodes), degenerate
graphs, and a trace of more than 2^20 ticks.

Every expected value comes from coracle.replay on the trace's own arrays, every comparison
goes through parity_util.assert_same_bits (last averages, flows, estimate caches, every
snapshot), and Replay.info() tells which persistent kernel a handle runs, so a silent
fallback fails the case that claims the register kernel.

The state at a cut of a resumed run is the oracle's replay of the trace's prefix: the same
arrays with tick_task_off cut after the segment's last tick (a shorter trace is a prefix of
the longer one: test_inputs_shorter_trace_is_a_prefix).

The unmarked tests at the end are conditions on the inputs, computed from the trace arrays
and the oracle alone: they run without a GPU, so a change to a generator cannot hollow a
case out unnoticed."""
import functools

import numpy as np
import pytest

import coracle
import fu
from fu import _lib as L
from parity_util import FAMILIES, assert_same_bits, count_neg_zero

gpu = pytest.mark.gpu

MODES = ["collectall", "pairwise"]
REPLAY_MODES = [False, True, "noreg"]  # per-tick launches, persistent (registers), persistent generic
TICKS, ORDER = 300, "rand:3"
FAULTS = "drop=0.1,delay=4:0.1,seed=3"
SNAPS = (100, 200, 299)
# value families: the non-finite values are still spreading at 70 ... 120; 120 is the last
# tick of the first segment, so the state (flows included) is compared while infinities exist
FAMILY_CUT, FAMILY_SNAPS = 121, (70, 90, 120, 299)
# resumed runs: (tick_end, snapshot ticks); the second run(57) has zero length
RESUME = ((57, (30, 56)), (57, ()), (58, (57,)), (200, (58, 120, 199)), (300, (200, 299)))
PATH_TICKS = (1 << 20) + 64


def _nan_inf(n, seed):
    """Uniform values with one quiet NaN and one inf among them."""
    v = np.random.default_rng(seed).random(n)
    v[n // 3] = np.nan
    v[2 * n // 3] = np.inf
    return v


VALUES = {"uniform": lambda n, seed: fu.uniform_values(n, seed=0), "huge": FAMILIES["huge"],
          "subn": FAMILIES["subn"], "wide": FAMILIES["wide"], "nan_inf": _nan_inf}


# ------------------------------------------------------------------------------------
# inputs: declared neighbour lists, traces and oracle results, each built once
# ------------------------------------------------------------------------------------
def _csr(rows):
    rp = np.zeros(len(rows) + 1, dtype=np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows).astype(np.int32) if rp[-1] else np.zeros(0, dtype=np.int32)
    return rp, col


def _asym(g, seed=5, frac=0.3):
    """g's neighbour lists with the declaration i -> j (i < j) removed for a random `frac` of
    the undirected edges (j still declares i: a dynamic addition at i when j's first message
    arrives), and each row's declared order shuffled."""
    rng = np.random.default_rng(seed)
    src = np.repeat(np.arange(g.n), np.diff(g.rowptr))
    col = np.asarray(g.col)
    up = np.flatnonzero(src < col)
    keep = np.ones(len(col), dtype=bool)
    keep[up[rng.random(len(up)) < frac]] = False
    return _csr([rng.permutation(col[g.rowptr[i]:g.rowptr[i + 1]][keep[g.rowptr[i]:g.rowptr[i + 1]]])
                 for i in range(g.n)])


@functools.lru_cache(maxsize=None)
def _decl(name):
    """(rowptr, col) of the declared neighbour lists."""
    if name == "er16":
        g = fu.Graph.erdos_renyi(3001, 9000, seed=4)
    elif name == "er16_asym":
        return _asym(fu.Graph.erdos_renyi(3001, 9000, seed=4))
    elif name in ("rr8", "rr9", "rr16", "rr17"):
        d = int(name[2:])
        g = fu.Graph.random_regular(1002 if d == 17 else 1000, d, seed=2)
    elif name == "rmat11":
        g = fu.Graph.rmat(11, 8, seed=4)
    elif name == "path4":
        return np.array([0, 1, 3, 5, 6], dtype=np.int64), np.array([1, 0, 2, 1, 3, 2], dtype=np.int32)
    elif name == "noedge5":
        return _csr([[]] * 5)
    elif name == "single":
        return _csr([[]])
    elif name == "edge2":
        return _csr([[1], [0]])
    else:
        raise KeyError(name)
    return np.asarray(g.rowptr, dtype=np.int64), np.asarray(g.col, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _trace(name, mode, faults=None, ticks=TICKS, order=ORDER):
    rp, col = _decl(name)
    return fu.Trace(rp, col, mode, ticks, order, faults=faults)


@functools.lru_cache(maxsize=None)
def _values(key, family):
    v = VALUES[family](_trace(*key).n, 9)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _ref(key, family, end, snaps):
    """The oracle's replay of ticks [0, end) of trace `key`: (last, flows, est, {tick: snapshot})."""
    tr = _trace(*key)
    a = tr.arrays()
    assert 0 <= end <= tr.ticks and all(0 <= t < end for t in snaps)
    return coracle.replay(a["rowptr"], _values(key, family), a["tick_task_off"][:end + 1], a["tasks"],
                          a["events"], a["out_ids"], tr.n_msgs, list(snaps))


def _unique_messages(a):
    """Messages sent over the trace: k per collect-all fire, one per pairwise fire."""
    ev = a["events"]
    return int(ev[ev[:, 0] == 1, 1].sum()) + int((ev[:, 0] == 2).sum())


def _open(key, family, persistent, blocks=None):
    rep = fu.Replay(_trace(*key), _values(key, family), persistent=bool(persistent),
                    registers=persistent != "noreg")
    if blocks is not None:
        rep.set_option("persistent_blocks", blocks)
    return rep


def _check_info(rep, key, persistent, reg):
    """info() against the trace: reg = the row registers the case claims (0: generic kernel)."""
    tr = _trace(*key)
    a = tr.arrays()
    info = rep.info()
    assert info[0] == int(bool(persistent))
    assert info[3] == int(tr.mode == "collectall" and tr.n_events > 0)
    assert info[6] == int(np.diff(a["rowptr"]).max(initial=0))
    if persistent:
        assert info[5] == _unique_messages(a)
        assert info[4] >= 1
    want = reg if persistent is True else 0
    assert (info[1], info[2]) == (int(want > 0), want), (key, persistent, info)
    return info


def _run_segments(rep, key, family, segments, what, states=True):
    """Run the segments [(tick_end, snapshot ticks)]: every snapshot, and the state after every
    segment, against the oracle's replay of [0, tick_end). states=False: one reference, the
    whole run; every snapshot and the state after the last segment."""
    seen = ()
    every = tuple(t for _, st in segments for t in st)
    for k, (end, st) in enumerate(segments):
        got = rep.run(end, snapshot_ticks=list(st))
        assert sorted(got) == sorted(st)
        seen += tuple(st)
        assert rep.info()[7] == end
        final = k == len(segments) - 1
        l_ref, f_ref, e_ref, s_ref = _ref(key, family, end, seen) if states else _ref(key, family, segments[-1][0], every)
        for t in st:
            assert_same_bits(got[t], s_ref[t], what + ("snapshot", t))
        if states or final:
            last, flows, est = rep.state()
            assert_same_bits(last, l_ref, what + (end, "last"))
            assert_same_bits(flows, f_ref, what + (end, "flows"))
            assert_same_bits(est, e_ref, what + (end, "est"))


def _check(key, family, persistent, reg, segments=((TICKS, SNAPS),), blocks=None):
    rep = _open(key, family, persistent, blocks)
    try:
        info = _check_info(rep, key, persistent, reg)
        if blocks is not None:
            assert info[4] == blocks
        _run_segments(rep, key, family, segments, (key, family, persistent, blocks))
    finally:
        rep.close()


# ------------------------------------------------------------------------------------
# 1. selection boundaries of the register kernel: degree <= 8, 9 ... 16, 17
# ------------------------------------------------------------------------------------
REG = {"rr8": 8, "rr9": 16, "rr16": 16, "er16": 16, "er16_asym": 16, "rr17": 0, "rmat11": 0}


@gpu
@pytest.mark.parametrize("persistent", REPLAY_MODES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["rr9", "rr16", "rr17", "er16"])
def test_selection_boundaries(name, mode, persistent):
    """Degrees 9 and 16 (16 row registers, the slot and k fields of the packed events above 8),
    17 (the generic kernel) and er16 (degrees 0 ... 16 side by side in a wave, every k at a
    collect-all fire). info() must show the kernel the case is about."""
    _check((name, mode), "uniform", persistent, REG[name])


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_degree_8_keeps_8_row_registers(mode):
    _check(("rr8", mode), "uniform", True, 8)


# ------------------------------------------------------------------------------------
# 2. hubs
# ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("persistent", REPLAY_MODES)
@pytest.mark.parametrize("mode", MODES)
def test_hubs(mode, persistent):
    """rmat11: a 593-element left-to-right chain in a fire, 334 nodes above degree 16 beside
    497 isolated ones; both persistent settings run the generic kernel."""
    _check(("rmat11", mode), "uniform", persistent, 0)


# ------------------------------------------------------------------------------------
# 3. asymmetric declarations and faults
# ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("persistent", REPLAY_MODES)
@pytest.mark.parametrize("mode", MODES)
def test_asymmetric_declarations(mode, persistent):
    """Dynamic neighbour additions: k < degree at a fire, slots in arrival order."""
    _check(("er16_asym", mode), "uniform", persistent, 16)


@gpu
@pytest.mark.parametrize("persistent", REPLAY_MODES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["er16_asym", "rmat11"])
def test_faults(name, mode, persistent):
    """Dropped and delayed messages, in collect-all mode too."""
    _check((name, mode, FAULTS), "uniform", persistent, REG[name])


# ------------------------------------------------------------------------------------
# 4. value families
# ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("persistent", REPLAY_MODES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["er16", "rmat11"])
@pytest.mark.parametrize("family", ["huge", "subn", "wide", "nan_inf"])
def test_value_families(family, name, mode, persistent):
    """`huge`: the order of a chain decides where the first inf and the first NaN appear;
    `wide`: a reassociated sum shows in the high bits; `subn`: the sign of zero. Two segments,
    so that flows and estimate caches are compared at tick 120 as well, before NaN has taken
    nearly every node."""
    _check((name, mode), family, persistent, REG[name],
           segments=((FAMILY_CUT, FAMILY_SNAPS[:3]), (TICKS, FAMILY_SNAPS[3:])))


# ------------------------------------------------------------------------------------
# 5. resumed runs
# ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("persistent", REPLAY_MODES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["er16", "rmat11"])
def test_resumed_runs(name, mode, persistent):
    """To tick 57, a zero-length run, to 58, 200 and 300, with snapshots at the last tick of a
    segment and the first of the next: the cursor write-back, the ring rebuild and the
    snapshot cursor at a cut. The state after every segment equals the oracle's replay of
    the trace's prefix."""
    _check((name, mode), "uniform", persistent, REG[name], segments=RESUME)


# ------------------------------------------------------------------------------------
# 6. few threads, many nodes: the node-stride loop of k_replay_persist
# ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("blocks", [1, 2, 5])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["rmat11", "er16"])
def test_few_blocks_many_nodes(name, mode, blocks):
    """With one block each of the 256 threads owns 8 (rmat11) or 11-12 (er16) nodes, polls each
    once per pass and moves on."""
    _check((name, mode), "uniform", "noreg", 0, blocks=blocks)


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_one_block_with_faults_resumed(mode):
    _check(("rmat11", mode, FAULTS), "uniform", "noreg", 0, segments=RESUME, blocks=1)


@gpu
def test_persistent_blocks_option():
    key = ("rr9", "pairwise")
    rep = _open(key, "uniform", True)
    try:
        free = rep.info()[4]
        assert free >= 1
        with pytest.raises(fu.FuError) as e:
            rep.set_option("persistent_blocks", -1)
        assert e.value.code == -1  # FU_ERR_ARG
        rep.set_option("persistent_blocks", 1 << 40)  # never above the occupancy-derived grid
        assert rep.info()[4] == free
        rep.set_option("persistent_blocks", 0)
        assert rep.info()[4] == free
        rep.set_option("persistent_blocks", 3)
        info = rep.info()
        assert info[4] == 3 and (info[1], info[2]) == (1, 16)  # no effect on the register kernel
        rep.run(60)
        with pytest.raises(fu.FuError) as e:
            rep.set_option("persistent_blocks", 1)
        assert e.value.code == -4  # FU_ERR_STATE
        assert rep.info()[4] == 3
        _run_segments(rep, key, "uniform", ((TICKS, SNAPS),), (key, "after option errors"))
    finally:
        rep.close()


@gpu
def test_device_out_of_range_then_a_good_create():
    """device == device_count is refused by name, leaves nothing behind, and device 0 still opens."""
    key = ("rr9", "pairwise")
    with pytest.raises(fu.FuError) as e:
        fu.Replay(_trace(*key), _values(key, "uniform"), device=fu.device_count())
    assert e.value.code == -1 and "fu_replay_create: device out of range" in str(e.value)
    rep = _open(key, "uniform", False)
    try:
        _run_segments(rep, key, "uniform", ((TICKS, SNAPS),), (key, "after a refused create"))
    finally:
        rep.close()


# ------------------------------------------------------------------------------------
# 7. degenerate shapes
# ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("persistent", REPLAY_MODES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["noedge5", "single", "edge2"])
def test_degenerate_shapes(name, mode, persistent):
    """No edges, one node, one edge: empty event and message arrays, fires with k = 0, and a
    snapshot of a node that never averaged reads 0.0 (as the oracle's does)."""
    _check((name, mode, None, 120), "uniform", persistent, 8, segments=((120, (40, 60, 119)),))


# ------------------------------------------------------------------------------------
# 8. past 2^20 ticks
# ------------------------------------------------------------------------------------
@gpu
def test_past_2pow20_ticks_falls_back_to_the_generic_kernel():
    """The register kernel's 8-byte events hold 20 tick bits, so a trace of 2^20 + 64 ticks
    runs the generic kernel. In segments of 2^16 ticks (a launch stays far from the kernels'
    bound of 2^22 passes), snapshots in the first, a middle and the last segment."""
    key = ("path4", "pairwise", None, PATH_TICKS, "fwd")
    rep = _open(key, "uniform", True)
    try:
        _check_info(rep, key, True, 0)
        cuts = list(range(1 << 16, PATH_TICKS, 1 << 16)) + [PATH_TICKS]
        snaps = {cuts[0]: (1000, (1 << 16) - 1), cuts[8]: (1 << 19,), 1 << 20: ((1 << 20) - 1,),
                 PATH_TICKS: (1 << 20, PATH_TICKS - 1)}
        _run_segments(rep, key, "uniform", [(c, snaps.get(c, ())) for c in cuts], (key,), states=False)
    finally:
        rep.close()


@gpu
def test_path_at_4096_ticks_uses_the_register_kernel():
    _check(("path4", "pairwise", None, 4096, "fwd"), "uniform", True, 8, segments=((4096, (1000, 4095)),))


# ------------------------------------------------------------------------------------
# input conditions (no GPU): the reference alone must meet each
# ------------------------------------------------------------------------------------
def _union_degrees(key):
    return np.diff(_trace(*key).arrays()["rowptr"])


@pytest.mark.parametrize("mode", MODES)
def test_inputs_degree_facts(mode):
    d = _union_degrees(("er16", mode))
    assert len(d) == 3001 and len(d) % 64 != 0
    assert d.min() == 0 and d.max() == 16 and set(range(17)) <= set(d.tolist())
    assert int(((d >= 9) & (d <= 16)).sum()) == 471
    d = _union_degrees(("er16_asym", mode))
    assert d.max() == 16 and d.min() == 0
    for name, deg, n in (("rr8", 8, 1000), ("rr9", 9, 1000), ("rr16", 16, 1000), ("rr17", 17, 1002)):
        d = _union_degrees((name, mode))
        assert len(d) == n and (d == deg).all()
    d = _union_degrees(("rmat11", mode))
    assert len(d) == 2048 and d.max() == 593 and d.min() == 0
    assert int((d > 16).sum()) == 334 and int(((d >= 9) & (d <= 16)).sum()) == 248
    # one block of 256 threads: 8 nodes per thread on rmat11, 11 or 12 on er16
    assert 2048 // 256 == 8 and (3001 // 256, -(-3001 // 256)) == (11, 12)


def test_inputs_every_k_at_a_collect_all_fire():
    ev = _trace("er16", "collectall").arrays()["events"]
    assert set(ev[ev[:, 0] == 1, 1].tolist()) == set(range(17))
    ev = _trace("er16", "pairwise").arrays()["events"]
    assert set(ev[ev[:, 0] == 2, 2].tolist()) == set(range(1, 17))  # k of the pairwise fires
    assert set(ev[ev[:, 0] == 2, 1].tolist()) == set(range(16))     # and their slots


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,faults", [("er16", None), ("er16_asym", None), ("er16_asym", FAULTS),
                                         ("rr8", None), ("rr9", None), ("rr16", None), ("rr17", None),
                                         ("rmat11", None), ("rmat11", FAULTS)])
def test_inputs_every_connected_node_fires(name, faults, mode):
    tr = _trace(name, mode, faults)
    a = tr.arrays()
    connected = np.diff(a["rowptr"]) > 0
    assert connected.any() and a["fires"][connected].min() >= 5
    if faults:
        assert tr.dropped > 0 and tr.delayed > 0
    else:
        assert tr.dropped == 0 and tr.delayed == 0
    if name == "er16_asym":
        assert tr.dynamic_additions > 2000
    else:
        assert tr.dynamic_additions == 0


@pytest.mark.parametrize("mode", MODES)
def test_inputs_asymmetric_fires_before_a_row_is_complete(mode):
    """k < union degree at a fire (the neighbour is added when its first message arrives)."""
    a = _trace("er16_asym", mode).arrays()
    deg = np.diff(a["rowptr"])
    tasks, ev = a["tasks"], a["events"]
    # the tasks' event ranges tile the event array in order, so this is each event's node
    assert tasks[0, 1] == 0 and tasks[-1, 2] == len(ev) and np.array_equal(tasks[1:, 1], tasks[:-1, 2])
    node = np.repeat(tasks[:, 0], tasks[:, 2] - tasks[:, 1])
    fire = ev[:, 0] == (1 if mode == "collectall" else 2)
    k = ev[fire, 1 if mode == "collectall" else 2]
    assert int((k < deg[node[fire]]).sum()) > 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["er16", "rmat11"])
def test_inputs_value_families_reach_the_edges(name, mode):
    key = (name, mode)
    l, f, _, _ = _ref(key, "subn", TICKS, FAMILY_SNAPS)
    assert count_neg_zero(l) > 0 and count_neg_zero(f) > 0
    l, f, e, _ = _ref(key, "wide", TICKS, FAMILY_SNAPS)
    assert np.isfinite(l).all() and np.isfinite(f).all() and np.isfinite(e).all()
    # huge: NaN and an infinity in the flows at the cut, a snapshot with finite values and NaN
    l, f, _, s = _ref(key, "huge", FAMILY_CUT, FAMILY_SNAPS[:3])
    assert np.isnan(f).any() and np.isinf(f).any() and np.isfinite(f).any()
    assert any(np.isnan(s[t]).any() and np.isfinite(s[t]).any() for t in FAMILY_SNAPS[:3])
    assert np.isnan(s[120]).any() and np.isfinite(s[120]).any()  # the compared state is mixed too
    l, _, _, s = _ref(key, "nan_inf", FAMILY_CUT, FAMILY_SNAPS[:3])
    assert np.isnan(s[120]).any() and np.isfinite(s[120]).any()
    n_nan = [int(np.isnan(s[t]).sum()) for t in FAMILY_SNAPS[:3]]
    assert n_nan[0] < n_nan[1] < n_nan[2]  # still spreading


def test_inputs_huge_takes_nearly_every_node():
    l, _, _, _ = _ref(("er16", "collectall"), "huge", TICKS, FAMILY_SNAPS)
    assert int(np.isnan(l).sum()) == 2994  # all but the 7 isolated nodes


@pytest.mark.parametrize("mode", MODES)
def test_inputs_degenerate_shapes(mode):
    tr = _trace("noedge5", mode, None, 120)
    ev = tr.arrays()["events"]
    if mode == "pairwise":
        assert tr.n_events == 0 and tr.n_msgs == 0 and tr.n_tasks == 0
    else:
        assert tr.n_events > 0 and (ev[:, 0] == 1).all() and (ev[:, 1] == 0).all() and tr.n_msgs == 0
    l, _, _, s = _ref(("noedge5", mode, None, 120), "uniform", 120, (40, 60, 119))
    assert not s[40].any()  # nothing happens before the first timeout: never averaged reads 0.0
    assert _trace("single", mode, None, 120).n == 1
    tr = _trace("edge2", mode, None, 120)
    assert tr.n_union_edges == 2 and tr.n_msgs > 0
    assert _trace("rr16", mode, None, 40).n_events == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["er16", "rmat11"])
def test_inputs_shorter_trace_is_a_prefix(name, mode):
    """The trace of the first 200 ticks is the 300-tick trace cut after tick 199, so the
    oracle's replay of the long trace's prefix is the reference run stopped there."""
    long, short = _trace(name, mode).arrays(), _trace(name, mode, None, 200).arrays()
    assert np.array_equal(short["rowptr"], long["rowptr"]) and np.array_equal(short["col"], long["col"])
    assert np.array_equal(short["tick_task_off"], long["tick_task_off"][:201])
    nt = len(short["tasks"])
    assert nt == long["tick_task_off"][200] and np.array_equal(short["tasks"], long["tasks"][:nt])
    ne = len(short["events"])
    assert 0 < ne < len(long["events"])
    assert np.array_equal(short["events"], long["events"][:ne])
    assert np.array_equal(short["out_ids"], long["out_ids"][:len(short["out_ids"])])


def test_inputs_path_trace_has_events_past_2pow20():
    tr = _trace("path4", "pairwise", None, PATH_TICKS, "fwd")
    a = tr.arrays()
    assert tr.ticks >= (1 << 20) and a["tick_task_off"][-1] > a["tick_task_off"][1 << 20]
    assert np.diff(a["rowptr"]).max() == 2
    assert _unique_messages(a) < (1 << 27)  # not the register kernel's other limit


def test_get_info_null_handle_is_an_argument_error():
    info = np.zeros(8, dtype=np.int64)
    assert L.lib.fu_replay_get_info(None, L.ptr(info)) == -1  # FU_ERR_ARG
    assert "fu_replay_get_info" in L.last_error()
