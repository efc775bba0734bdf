"""The conditions that make test_row_order_gpu.py mean something, all on the CPU
(order_cases.py): the reordered graphs reach the engines as written, the native reverse index
and the validation of a caller's one take the unsorted branch and agree with the oracle's, the
results are sensitive to the row order on every named row (so an engine that sums in ascending
id order fails on every row class), the fast oracle is itself pinned to the Python one off
ascending rows, and the host-side pieces that see rows (the pair matching, fu.dist.partition,
fu_graph_relabel) keep the caller's order."""
import numpy as np
import pytest

import coracle
import fu
import oracle
import order_cases as oc
from lossy_cases import M64, splitmix_at_py
from pair_cases import SEED as PAIR_SEED
from pair_cases import matching_py

CASES = sorted(oc.GRAPHS)
CASE_HOWS = [(name, how) for name in CASES for how in oc.GPU_HOWS[name]]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------
# the rows reach the library as written
# ------------------------------------------------------------------------------------
def test_reorder_rows_on_a_row_by_hand():
    rp = np.array([0, 5, 6, 7, 8, 9, 10], dtype=np.int64)
    col = np.array([1, 2, 3, 4, 5, 0, 0, 0, 0, 0], dtype=np.int32)
    want = {"descending": [5, 4, 3, 2, 1], "rotated": [4, 5, 1, 2, 3], "zigzag": [1, 5, 2, 4, 3]}
    for how, row in want.items():
        got = oc.reorder_cols(rp, col, how)
        assert got[:5].tolist() == row and got[5:].tolist() == [0] * 5, how
        assert oc.reorder_cols(rp, got, how).tolist() == got.tolist()  # from any order of the same rows
    got = oc.reorder_cols(rp, col, "random", seed=1)
    assert sorted(got[:5].tolist()) == [1, 2, 3, 4, 5] and got[:5].tolist() != [1, 2, 3, 4, 5]
    assert np.array_equal(got, oc.reorder_cols(rp, col, "random", seed=1))
    assert not np.array_equal(got, oc.reorder_cols(rp, col, "random", seed=2))


@pytest.mark.parametrize("how", oc.HOWS)
@pytest.mark.parametrize("name", CASES)
def test_from_csr_keeps_the_rows_and_rev_is_the_oracles(name, how):
    """fu_graph_from_csr returns col unchanged, the rows are the base graph's as sets, no row of
    three or more slots is ascending (how = "random": nearly none), and the native reverse index
    (the `perm` branch of build_rev) is oracle.build_rev's."""
    base = oc.base_graph(name)
    assert oc.is_ascending(base.rowptr, base.col).all()
    want = oc.reorder_cols(base.rowptr, base.col, how, oc.REORDER_SEED)
    g = oc.reorder_rows(base, how, oc.REORDER_SEED)
    assert np.array_equal(g.rowptr, base.rowptr) and g.col.dtype == np.int32
    assert np.array_equal(g.col, want)
    assert np.array_equal(oc.sorted_cols(g.rowptr, g.col), base.col)
    asc = oc.is_ascending(g.rowptr, g.col)
    d3 = base.degrees >= 3
    if how == "random":
        assert asc[d3].mean() < 0.2  # 1 / 6 of the rows of three slots, fewer of the longer ones
        assert not asc[base.degrees >= 12].any()
    else:
        assert not asc[d3].any()
    rev = oracle.build_rev(g.rowptr, g.col)
    assert np.array_equal(g.rev, rev)
    k = np.arange(g.E)
    assert np.array_equal(g.rev[g.rev], k)
    m = oc.slot_map(g, base)
    assert np.array_equal(base.col[m], g.col) and np.array_equal(m[g.rev], base.rev[m])


@pytest.mark.parametrize("name,how", [("tile_limit", "random"), ("chunk_edge", "zigzag"), ("pair_class", "random")])
def test_callers_rev_passes_the_create_checks(name, how):
    """fu_lossy_create, fu_churn_create and fu_pair_create with the caller's rev on a reordered
    graph: the pairing check passes (on a host without a GPU the call ends at the device probe),
    and a rev taken from the ascending graph is refused."""
    g = oc.graph(name, how)
    rp, col, rev = g.arrays()
    v = oc.values(name)
    stale = oc.base_graph(name).rev
    assert not np.array_equal(stale, rev)
    for cls in (fu.CollectAllLossy, fu.CollectAllChurn, fu.PairwiseSync):
        try:
            cls(rowptr=rp, col=col, rev=rev, values=v).close()
        except fu.FuError as e:
            assert fu.device_count() == 0 and "no HIP device" in str(e), (cls.__name__, e)
        with pytest.raises(fu.FuError, match="rev is not the reverse-edge pairing") as ei:
            cls(rowptr=rp, col=col, rev=stale, values=v)
        assert ei.value.code == -5


# ------------------------------------------------------------------------------------
# sensitivity: the order of a row shows in its bits
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,how", CASE_HOWS)
def test_results_depend_on_the_row_order(name, how):
    """The C oracle on the reordered graph against the C oracle on the ascending one, slot for
    slot, at the stops the GPU tests compare: on every named row of three or more slots
    (order_cases.named_rows: every class-edge centre among them) the estimate differs in bits at
    one of the stops and so does the flow of at least one slot. The GPU tests compare at every
    stop, so an engine that summed such a row in ascending id order would fail on it. (At a
    single stop a long row's estimate often keeps its bits: the quotient by d + 1 rounds the
    sums' last bits away. Hence "at one of the stops", and the seeds in order_cases.) Rows of 0,
    1 and 2 slots cannot differ in their own sums and are exempt, by degree; no other row is."""
    deg = oc.base_graph(name).degrees
    rows = oc.named_rows(name)
    assert any(deg[i] >= 3 for i in rows)
    da, df = oc.differing_rows(name, how)
    for i, why in rows.items():
        if int(deg[i]) in oc.EXEMPT_DEGREES:
            continue
        assert da[i], (name, how, why, "estimate")
        assert df[i], (name, how, why, "flows")
    # round 0 is a = v / (d + 1) for either order; from round 1 on the sums are over several
    # terms, and every later stop tells the two orders apart somewhere
    got, asc = oc.reference(name, how), oc.reference(name, None)
    for stop in oc.STOPS[name]:
        same = np.array_equal(_bits(got[stop][0]), _bits(asc[stop][0]))
        assert same == (stop == 1), (name, how, stop)


def _named(name):
    deg = oc.base_graph(name).degrees
    return [i for i in oc.named_rows(name) if int(deg[i]) not in oc.EXEMPT_DEGREES]


@pytest.mark.parametrize("name,how,family", oc.FAMILY_TRIPLES)
def test_family_results_depend_on_the_row_order(name, how, family):
    """The same condition for the value families of order_cases.GPU_FAMILIES, for exactly the
    (case, order, family) triples test_row_order_values_gpu.py runs, at the family's stops and
    judged as assert_same_bits judges (NaN against NaN is no difference).

    wide, neg, sym, binade: every named row of three or more slots differs in its estimate and
    in at least one flow, as for uniform values.

    subn: no condition on differences can hold. The values are integers times 2^-1074 below 50
    in magnitude, so every sum and difference of the rule is exact (no row reaches 2^52 of
    them) and only the quotient by d + 1 rounds: the bits do not depend on the order of any
    row, which is asserted here so that nobody reads a subn pass as evidence about order. What
    subn brings to reordered rows is signed zeros through every gather and store: the oracle
    holds -0.0 in the estimate or a flow of at least one named row.

    huge: "every named row" cannot hold either. A row whose chain overflows in both orders ends
    in the same infinity, or in NaN once both infinities met, whatever the order (10 of the 12
    cases have such named rows at every seed from 3 to 12). The family exists for the other
    rows, where the order decides whether and where the chain overflows: at least one named
    row differs in its estimate or a flow, and at least one row of three or more slots of the
    graph is of another class (finite, +inf, -inf, NaN) than on ascending rows; the class
    condition on the named rows is test_huge_changes_the_class_of_a_named_row."""
    rows = _named(name)
    da, df = oc.differing_rows(name, how, family)
    if family == "subn":
        assert not da.any() and not df.any(), (name, how, "subn sums are exact")
        nz = oc.neg_zero_rows(name, how)
        assert any(nz[i] for i in rows), (name, how, "no named row reaches -0.0")
    elif family == "huge":
        assert any(da[i] or df[i] for i in rows), (name, how, "no named row differs")
        cc = oc.class_changing_rows(name, how)
        assert cc[oc.base_graph(name).degrees >= 3].any(), (name, how, "no row changes class")
        ref = oc.reference(name, how, None, family)
        last = oc.stops(name, family)[-1]
        assert np.isnan(ref[last][0]).any() and np.isinf(ref[3][1]).any()  # the chains do overflow
    else:
        for i in rows:
            assert da[i], (name, how, family, oc.named_rows(name)[i], "estimate")
            assert df[i], (name, how, family, oc.named_rows(name)[i], "flows")


@pytest.mark.parametrize("name", CASES)
def test_huge_changes_the_class_of_a_named_row(name):
    """Over the named rows of the case at least one is finite, +inf, -inf or NaN under a
    reordered oracle where the ascending one is of another class, at one of the early stops: an
    engine that summed that row in ascending order would put an infinity or a NaN where the
    reference has none. Two cases have no such seed from 3 to 12 (order_cases.HUGE_BITWISE_ONLY);
    for them the test states that, so that a change of their named rows or seeds revisits it."""
    rows = _named(name)
    hit = [how for how in oc.GPU_HOWS[name] if any(oc.class_changing_rows(name, how)[i] for i in rows)]
    assert bool(hit) == (name not in oc.HUGE_BITWISE_ONLY), (name, hit)
    assert len(oc.HUGE_BITWISE_ONLY) <= 2


def test_family_table_and_stops():
    """The table both sides parametrize from: wide, huge and subn on every case, the packing
    families on pack_er only; huge stops at rounds 1, 2, 3 and the case's last stop, every other
    family at the case's stops; the uniform seeds are the ones fixed before."""
    assert set(oc.GPU_FAMILIES) == set(oc.GRAPHS) == set(oc.GPU_HOWS)
    for name, fams in oc.GPU_FAMILIES.items():
        assert fams[:3] == ("wide", "huge", "subn")
        assert fams[3:] == (("neg", "sym", "binade") if name == "pack_er" else ())
        assert oc.stops(name, "huge")[:3] == (1, 2, 3) and oc.stops(name, "huge")[-1] == oc.STOPS[name][-1]
        assert len(oc.stops(name, "huge")) <= 4
        for family in fams:
            assert 3 <= oc.VALUE_SEED[name, family] <= 12
            if family != "huge":
                assert oc.stops(name, family) == oc.STOPS[name]
    assert len(oc.FAMILY_TRIPLES) == len(set(oc.FAMILY_TRIPLES)) == 72
    assert {n: oc.VALUE_SEED[n] for n in oc.GRAPHS} == {**{n: 3 for n in oc.GRAPHS}, "batch_boundary": 4,
                                                        "rmat_large": 5, "tile_limit": 6, "pack_er": 4}


def test_pack_family_inputs_reach_every_width():
    """The inputs of test_packed_families_on_reordered_rows, from the oracle and the plan's rule
    restated (pack_cases.plan_of) alone: on the reordered pack_er graph with the non-finite
    components beside it, the plan from the oracle's estimates gives 32, 16 and 8 bits at the
    three stops of parity_util.PACK_STOPS, for each packing family; the components end in
    NaN and -0.0 (the doubles behind the escape code); and the straddle input packs to 8 bits
    from the first plan."""
    from pack_cases import plan_of, plan_sample
    from parity_util import count_neg_zero
    from parity_util import PACK_STOPS

    for family in oc.PACK_FAMILIES:
        g, v = oc.pack_graph(family)
        sample = plan_sample(g.col)
        refs = oc.pack_reference(family)
        n0 = oc.base_graph("pack_er").n
        for stop, width in zip(PACK_STOPS[family], (32, 16, 8)):
            for r in (stop - oc.PACK_SETTLED, stop):  # pack_every 4: a plan from this span is in use at the stop
                assert plan_of(refs[r][0], sample)[0] == width, (family, r)
        a_end = refs[PACK_STOPS[family][-1]][0]
        assert np.isfinite(a_end[:n0]).all()
        assert np.isnan(a_end[n0:]).sum() == 9 and count_neg_zero(a_end[n0:]) == 1
    g, v = oc.graph("pack_er", "random"), oc.straddle_values()
    a, _ = coracle.ca_sync(*g.arrays(), v, 2)
    assert plan_of(a, plan_sample(g.col))[0] == 8


def _rule_on_python_floats(adj, v, rounds, drop_zero_sign):
    """[(estimates, flows in row order)] after 1 .. rounds rounds of the collect-all rule on a
    small graph (round 0 receives nothing; from round 1 on fr = -f_ji, er = a_j, S = 0.0 + fr..,
    T = 0.0 + er.., a = ((v - S) + T) / (d + 1), f_ij = (fr + a) - er). drop_zero_sign: a gathered
    estimate that is a zero arrives as +0.0."""
    n = len(v)
    f = {(i, j): 0.0 for i in range(n) for j in adj[i]}
    a, out = [0.0] * n, []
    for r in range(rounds):
        na, nf = [0.0] * n, {}
        for i in range(n):
            S = T = 0.0
            got = []
            for j in adj[i]:
                fr, er = (-f[j, i] if r else 0.0), a[j]
                if drop_zero_sign and er == 0.0:
                    er = er + 0.0
                got.append((j, fr, er))
                S, T = S + fr, T + er
            na[i] = ((v[i] - S) + T) / (len(adj[i]) + 1)
            for j, fr, er in got:
                nf[i, j] = (fr + na[i]) - er
        a, f = na, nf
        out.append((np.array(a), np.array([f[i, j] for i in range(n) for j in adj[i]])))
    return out


def test_signed_zero_extras_show_the_sign_of_a_gathered_zero():
    """The components of order_cases.SIGNED_ZERO_EXTRAS, alone: the rule on Python floats equals
    the C oracle on them, and a gather that drops the sign of a zero gives other bits at every
    packing stop of the `neg` case or one or two rounds after the last (the stops of
    test_packed_escapes_keep_the_sign_of_zero), so a packed reader that loses the sign behind
    its escape code fails there."""
    from parity_util import PACK_STOPS

    stops = oc.pack_stops("neg", "signed_zero")
    assert stops[-3:] == (PACK_STOPS["neg"][-1], PACK_STOPS["neg"][-1] + 1, PACK_STOPS["neg"][-1] + 2)
    for comp in oc.SIGNED_ZERO_EXTRAS:
        adj = [[1], [0]] if len(comp) == 2 else [[2, 1], [0, 2], [1, 0]]  # with_components' rows
        rp = np.cumsum([0] + [len(x) for x in adj]).astype(np.int64)
        g = fu.Graph.from_csr(rp, np.concatenate(adj).astype(np.int32))
        right = _rule_on_python_floats(adj, comp, stops[-1], False)
        wrong = _rule_on_python_floats(adj, comp, stops[-1], True)
        differ = []
        for r in stops:
            a, f = coracle.ca_sync(*g.arrays(), np.array(comp), r)
            assert np.array_equal(_bits(a), _bits(right[r - 1][0])) and np.array_equal(_bits(f), _bits(right[r - 1][1])), (comp, r)
            differ.append(not np.array_equal(_bits(f), _bits(wrong[r - 1][1])))
        assert any(differ[len(oc.STOPS["pack_er"]):len(oc.STOPS["pack_er"]) + 3]), (comp, differ)  # at a packing stop
        assert any(differ[-3:]), (comp, differ)


@pytest.mark.parametrize("name,how", [("rmat_small", "random"), ("rmat_small", "descending"), ("tile_limit", "zigzag"),
                                      ("pair_class", "random"), ("batch_boundary", "rotated")])
def test_python_oracle_equals_c_oracle_off_ascending_rows(name, how):
    """oracle.py (numpy float64 chains in row order, the restatement of the Python floats) and
    coracle agree bit for bit on reordered rows: the fast oracle that the GPU tests compare with
    is itself pinned where rows are not ascending."""
    g, v = oc.graph(name, how), oc.values(name)
    rounds = 9
    snaps = oracle.ca_sync(g.rowptr, g.col, v, rounds, rev=g.rev, snapshot_rounds=[1, 2, rounds - 1])
    for r, (a, f) in snaps.items():
        a_c, f_c = coracle.ca_sync(*g.arrays(), v, r + 1)
        assert np.array_equal(_bits(a), _bits(a_c)) and np.array_equal(_bits(f), _bits(f_c)), (name, how, r)


# ------------------------------------------------------------------------------------
# c16: the narrow blocks do not move
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", oc.GPU_HOWS["c16"])
def test_c16_blocks_stay_narrow_or_wide(how):
    """Whether a 1024-slot block is narrow depends on the columns it holds and on its first row,
    not on their order inside a row; a row that straddles two blocks could still move a far
    column across the boundary. On this graph it does not: the reordered graph has the narrow
    and wide blocks of the ascending one, narrow ones before and after a wide one inside the
    RGG part, and 2-byte offsets that go both up and down inside a row and reach both halves of
    the window."""
    base, g = oc.base_graph("c16"), oc.graph("c16", how)
    narrow0, base0 = oc.c16_blocks(base.rowptr, base.col)
    narrow, base1 = oc.c16_blocks(g.rowptr, g.col)
    assert np.array_equal(narrow, narrow0) and np.array_equal(base1, base0)
    wide = np.flatnonzero(~narrow)
    # the blocks that hold an end of a long-range link are the wide ones, each beside a narrow one
    ends = sorted({int(base.rowptr[i]) // oc.C16_BLOCK for link in oc.C16_FAR for i in link})
    assert set(wide.tolist()) <= set(ends + [b + 1 for b in ends]) and len(wide) >= len(oc.C16_FAR)
    assert narrow.sum() > 400
    for b in wide:
        assert narrow[max(b - 1, 0)] or narrow[min(b + 1, len(narrow) - 1)]
    src = np.repeat(np.arange(g.n), g.degrees)
    off = g.col.astype(np.int64) - np.repeat(base1, oc.C16_BLOCK)[:g.E]
    in_narrow = np.repeat(narrow, oc.C16_BLOCK)[:g.E]
    assert off[in_narrow].min() < -100 and off[in_narrow].max() > 100
    step = np.diff(g.col.astype(np.int64))
    inside = (src[1:] == src[:-1]) & in_narrow[1:]
    assert (step[inside] > 0).any() and (step[inside] < 0).any()


# ------------------------------------------------------------------------------------
# the pair matching takes its slot from the caller's row
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,how", [(n, h) for n in ("pair_class", "dense66") for h in oc.GPU_HOWS[n]])
def test_pair_matching_on_reordered_rows(name, how):
    """fu_pair_matching against the rule on Python ints: proposer i (the same nodes as on the
    ascending graph: h_i does not see the rows) picks j = col[rowptr[i] + p_i] of the caller's
    row, so the matching differs from the ascending graph's; mate is symmetric."""
    g, base = oc.graph(name, how), oc.base_graph(name)
    differ = 0
    for r in range(4):
        mate, ini = fu.pair_matching(g, PAIR_SEED, r)
        want_mate, want_ini = matching_py(g.rowptr, g.col, PAIR_SEED, r)
        assert mate.tolist() == want_mate and ini.tolist() == want_ini, (name, how, r)
        on = np.flatnonzero(mate >= 0)
        assert len(on) and np.array_equal(mate[mate[on]], on)
        assert np.array_equal(ini[on] + ini[mate[on]], np.ones(len(on)))
        key = splitmix_at_py(PAIR_SEED & M64, r)
        for i in np.flatnonzero(ini)[:200]:
            h = splitmix_at_py(key, int(i))
            assert h & 1 and mate[i] == g.col[g.rowptr[i] + (h >> 1) % int(g.degrees[i])]
        mate0, ini0 = fu.pair_matching(base, PAIR_SEED, r)
        differ += int((mate0 != mate).sum())
    assert differ > g.n // 10


# ------------------------------------------------------------------------------------
# fu.dist.partition and the halo plan
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("name,how", [(n, h) for n in ("cut_slivers", "cut_rmat") for h in oc.GPU_HOWS[n]])
def test_partition_keeps_the_row_order(name, how, world):
    """Every rank's local rows are the caller's rows with ghost ids substituted (col) and ghost
    flow slots substituted (rev), in the caller's order; sender and receiver agree on the halo."""
    from dist_cases import check_plan_symmetry
    from fu.dist import partition

    g = oc.graph(name, how)
    bounds = oc.cut_bounds(name, world)
    plans = [partition(g.rowptr, g.col, g.rev, world, r, bounds=bounds) for r in range(world)]
    check_plan_symmetry(g.rowptr, plans)
    assert sum(p.n_ghost_a for p in plans) > 0
    for p in plans:
        e0, e1 = int(g.rowptr[p.lo]), int(g.rowptr[p.hi])
        assert np.array_equal(p.rowptr, g.rowptr[p.lo:p.hi + 1] - e0)
        c = p.col.astype(np.int64)
        gid = np.where(c < p.n_local, c + p.lo, p.ghost_a_gid[np.maximum(c - p.n_local, 0)] if p.n_ghost_a else c + p.lo)
        assert np.array_equal(gid, g.col[e0:e1]), (name, how, world, p.rank)
        r = p.rev.astype(np.int64)
        gidx = np.where(r < p.e_local, r + e0, p.ghost_f_gidx[np.maximum(r - p.e_local, 0)] if p.n_ghost_f else r + e0)
        assert np.array_equal(gidx, g.rev[e0:e1]), (name, how, world, p.rank)
        if how != "random":  # the local ids are monotone in the global ones inside a rank's own range only
            continue
        assert not oc.is_ascending(p.rowptr, p.col)[np.diff(p.rowptr) >= 12].any()


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("name", ["cut_slivers", "cut_rmat"])
def test_partitioned_rounds_on_reordered_rows_match_oracle(name, world):
    """The CPU model of the partitioned rounds (test_dist_gloo: gloo ranks that exchange the
    halo as fu_dist.hip does, estimates-only) on the reordered cut cases reproduces the
    single-graph Python oracle bit for bit."""
    from test_dist_gloo import _run_and_compare

    g = oc.graph(name, oc.GPU_HOWS[name][0])
    _run_and_compare(g, np.array(oc.values(name)), world, "recon", 8, bounds=oc.cut_bounds(name, world))


# ------------------------------------------------------------------------------------
# fu_graph_relabel
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,how", [("rmat_small", "random"), ("class_edge", "zigzag"), ("chunk_edge", "rotated")])
def test_degree_relabel_keeps_unsorted_rows(name, how):
    """fu_graph_relabel order 1 on a reordered graph: rows move as blocks, the order inside a row
    is kept (the new ids are then in no order at all), rev follows, and the rounds on the
    relabelled graph are the caller's, bit for bit."""
    from test_relabel import _check_relabelled

    g, v = oc.graph(name, how), oc.values(name)
    h, perm = g.relabel("degree")
    _check_relabelled(g, h, perm)
    assert np.all(np.diff(h.degrees) <= 0)
    v2 = np.empty_like(v)
    v2[perm] = v
    a, f = coracle.ca_sync(*g.arrays(), v, 6)
    a2, f2 = coracle.ca_sync(*h.arrays(), v2, 6)
    assert np.array_equal(_bits(a2[perm]), _bits(a))
    f_back = np.concatenate([f2[h.rowptr[perm[i]]:h.rowptr[perm[i] + 1]] for i in range(g.n)])
    assert np.array_equal(_bits(f_back), _bits(f))
