"""Every engine on rows whose neighbours are not in ascending id order (order_cases.py), bit for
bit against the C oracle on the same reordered graph, or against the engine's own restatement
where the C oracle has no such mode. On ascending rows, slice order (kernel 8), bucket order
(kernel 9), chunk order (heavy rows, chains, mega hubs, the batch, rev-gather and pair engines) and
ascending id order all coincide with row order; here they do not, and test_order_case_inputs.py
shows on the CPU that the reference bits of every named row differ from the ascending order's.
Every reference is computed once per case and shared read-only."""
import functools

import numpy as np
import pytest

import coracle
import fu
import order_cases as oc
from churn_cases import churn_python, cut, heavy_rows
from pair_cases import CLASS_ROUNDS, SEED, oracle_pair, pair_count, roles
from pair_loss_cases import CLASS_P, LOSS_SEED, fired_nodes, hashed, loss_counts, oracle_pair_loss
from parity_util import assert_same_bits
from rev_columns_cases import LOSS_SEED as REV_LOSS_SEED
from rev_columns_cases import Step, drive_churn, link_mask, lossy_reference

pytestmark = pytest.mark.gpu

KERNELS = ["recon", "stage", "pregather"]


def _run_to_stops(eng, name, how, what, stops=None, ref=None):
    ref = ref or oc.reference(name, how, stops)
    for stop in sorted(ref):
        eng.run(stop - eng.info()["rounds"])
        assert_same_bits(eng.estimates(), ref[stop][0], what + ("estimates", stop))
        assert_same_bits(eng.flows(), ref[stop][1], what + ("flows", stop))


# ------------------------------------------------------------------------------------
# the main engine on every row class
# ------------------------------------------------------------------------------------
OPTION_ROWS = [("recon", "wave_heavy"), ("recon", "fork_heavy"), ("pregather", "lag"), ("pregather", "multi_heavy"),
               ("pregather", "multi_mid"), ("pregather", "multi_short"), ("pregather", "mid_heavy")]


@pytest.mark.parametrize("how", oc.GPU_HOWS["class_edge"])
@pytest.mark.parametrize("layout", ["given", "degree"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_row_classes_on_reordered_rows(kernel, layout, how):
    """Star centres of every row class's first and last degree, 0 to 12000, their rows shuffled
    or zigzag: light tiles, heavy rows, multi-row chains, the register launch and the mega
    hubs sum in the caller's row order; read back after 1, 3, 8 and 17 rounds (the lagged flows
    finalised in between), and through the degree layout's readback."""
    g = oc.graph("class_edge", how)
    with fu.CollectAll(g, oc.values("class_edge"), kernel=kernel, layout=layout) as eng:
        _run_to_stops(eng, "class_edge", how, (kernel, layout, how))


@pytest.mark.parametrize("layout", ["given", "degree"])
@pytest.mark.parametrize("kernel,option", OPTION_ROWS)
def test_row_classes_with_the_other_summing_path(kernel, option, layout):
    """The options that change which launch sums a row, each switched off, on shuffled rows."""
    g = oc.graph("class_edge", "random")
    with fu.CollectAll(g, oc.values("class_edge"), kernel=kernel, layout=layout) as eng:
        eng.set_option(option, 0)
        _run_to_stops(eng, "class_edge", "random", (kernel, option, layout))


# ------------------------------------------------------------------------------------
# mega hubs
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,opt", [("recon", ("tile_edges", 512)), ("recon", ("tile_edges", 1024)),
                                        ("recon", ("tile_edges", 2048)), ("pregather", ("tr_bpx", 0)),
                                        ("pregather", ("tr_bpx", 3))])
@pytest.mark.parametrize("mega", [64, oc.MEGA_HUB])
@pytest.mark.parametrize("name,how", [(n, h) for n in ("rmat_small", "rmat_large") for h in oc.GPU_HOWS[n]])
def test_mega_hubs_on_reordered_rows(name, how, mega, kernel, opt):
    """R-MAT rows above a lowered mega_hub (k_hub_stage, the chain block, k_hub_flows) and heavy
    rows above hub_threshold 32, reordered: kernel 4 at every tile size, kernel 9 with one
    transpose block per bucket and with three per XCD."""
    g = oc.graph(name, how)
    with fu.CollectAll(g, oc.values(name), kernel=kernel, hub_threshold=32) as eng:
        eng.set_option("mega_hub", mega)
        eng.set_option(*opt)
        hubs = int((g.degrees > mega).sum())
        assert eng.info()["mega_hubs"] == hubs
        if (name, mega) != ("rmat_small", oc.MEGA_HUB):  # its longest row has 221 slots: heavy rows only there
            assert hubs > 0
        _run_to_stops(eng, name, how, (name, how, mega, kernel, opt))


# ------------------------------------------------------------------------------------
# kernel 4's 2-byte column offsets
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [2048, 1024, 512])
@pytest.mark.parametrize("how", oc.GPU_HOWS["c16"])
def test_c16_on_reordered_rows(how, tile):
    """The c16 graph rotated (the smallest id mid-row) and zigzag (offsets alternate between the
    two halves of the 32K window), c16 on and off. Which blocks stay narrow: all those of the
    ascending graph, the blocks that hold an end of one of the three long-range links being the
    wide ones (test_c16_blocks_stay_narrow_or_wide restates FP::build_blocks on the CPU;
    fu_get_info reports no tile counts, so the split cannot be read from the handle)."""
    g = oc.graph("c16", how)
    for c16 in (1, 0):
        with fu.CollectAll(g, oc.values("c16"), kernel="recon") as eng:
            eng.set_option("tile_edges", tile)
            eng.set_option("c16", c16)
            _run_to_stops(eng, "c16", how, (how, tile, "c16", c16))


# ------------------------------------------------------------------------------------
# packed gathers
# ------------------------------------------------------------------------------------
PACK_STEP, PACK_LIMIT, PACK_BEYOND = 20, 600, (3, 10)
_pack_ref = {}


def _pack_reference(rounds):
    """(a, f) of the reordered ER after `rounds` rounds, continued from the longest run so far."""
    g, v = oc.graph("pack_er", "random"), oc.values("pack_er")
    if rounds not in _pack_ref:
        before = [r for r in _pack_ref if r < rounds]
        if before:
            a, f = (x.copy() for x in _pack_ref[max(before)])
            coracle.ca_rounds(*g.arrays(), v, rounds - max(before), a, f, nthreads=8)
        else:
            a, f = coracle.ca_sync(*g.arrays(), v, rounds, nthreads=8)
        _pack_ref[rounds] = (a, f)
    return _pack_ref[rounds]


@pytest.mark.parametrize("kernel,layout", [("recon", -1), ("pregather", -1)] + [("stage", q) for q in range(4)])
def test_packed_gathers_on_reordered_rows(kernel, layout):
    """Reordered ER with a packing plan every 4 rounds, run until the estimate table is 8 bits
    wide: compared right after the switch and 3 and 10 rounds beyond it, every kernel, kernel 8
    with each slice layout forced."""
    g, v = oc.graph("pack_er", "random"), oc.values("pack_er")
    with fu.CollectAll(g, v, kernel=kernel) as eng:
        eng.set_option("pack_every", 4)
        if layout >= 0:
            eng.set_option("stage_layout", layout)
        done = 0
        while eng.pack_widths()[2] != 8 and done < PACK_LIMIT:
            eng.run(PACK_STEP)
            done += PACK_STEP
        assert eng.pack_widths()[2] == 8, (done, eng.pack_widths())
        for more in (0,) + PACK_BEYOND:
            eng.run(done + more - eng.info()["rounds"])
            a_ref, f_ref = _pack_reference(done + more)
            assert_same_bits(eng.estimates(), a_ref, (kernel, layout, done + more))
            assert_same_bits(eng.flows(), f_ref, (kernel, layout, done + more))
        assert 8 in eng.pack_widths()


# ------------------------------------------------------------------------------------
# fu_create on raw arrays
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", oc.GPU_HOWS["rmat_large"])
def test_raw_create_with_and_without_the_callers_rev(how):
    """fu_create with the caller's rev and with rev = NULL (the library builds it through the
    unsorted branch of build_rev): the same bits, and the oracle's."""
    g, v = oc.graph("rmat_large", how), oc.values("rmat_large")
    rp, col, rev = g.arrays()
    ref = oc.reference("rmat_large", how)
    got = []
    for r in (rev, None):
        with fu.CollectAll(rowptr=rp, col=col, rev=r, values=v, kernel="recon", hub_threshold=32) as eng:
            eng.set_option("mega_hub", oc.MEGA_HUB)
            _run_to_stops(eng, "rmat_large", how, (how, "rev" if r is not None else "no rev"), ref=ref)
            got.append((eng.estimates(), eng.flows()))
    assert_same_bits(got[0][0], got[1][0])
    assert_same_bits(got[0][1], got[1][1])


# ------------------------------------------------------------------------------------
# the batched engine
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _column_reference(name, how, seed):
    g = oc.graph(name, how)
    v = fu.uniform_values(g.n, seed=seed)
    out, done, a, f = {}, 0, None, None
    for stop in oc.STOPS[name]:
        if a is None:
            a, f = coracle.ca_sync(*g.arrays(), v, stop, nthreads=8)
        else:
            coracle.ca_rounds(*g.arrays(), v, stop - done, a, f, nthreads=8)
        done = stop
        out[stop] = (a.copy(), f.copy())
    return v, out


@pytest.mark.parametrize("K", [1, 3, 8, 16])
@pytest.mark.parametrize("how", oc.GPU_HOWS["batch_boundary"])
def test_batch_columns_on_reordered_rows(how, K):
    """K columns over the reordered batch boundary graph (rows on both sides of every chunk of
    2048 // K slots): each column against an oracle run of its own."""
    name = "batch_boundary"
    g = oc.graph(name, how)
    cols = [_column_reference(name, how, oc.VALUE_SEED[name] + c) for c in range(K)]
    V = np.ascontiguousarray(np.stack([v for v, _ in cols], axis=1))
    with fu.CollectAllBatch(g, V) as eng:
        for stop in oc.STOPS[name]:
            eng.run(stop - eng.rounds_done)
            a, f = eng.estimates(), eng.flows()
            for c, (_, ref) in enumerate(cols):
                assert_same_bits(np.ascontiguousarray(a[:, c]), ref[stop][0], (how, K, "column", c, "estimates", stop))
                assert_same_bits(np.ascontiguousarray(f[:, c]), ref[stop][1], (how, K, "column", c, "flows", stop))


# ------------------------------------------------------------------------------------
# the rev-gather round: lossy and churn
# ------------------------------------------------------------------------------------
REV_CASES = [(n, h) for n in ("tile_limit", "chunk_edge") for h in oc.GPU_HOWS[n]]
LOSSY_P, LOSSY_STOPS = 0.3, (2, 6)
MAX_K = 5


def _rev_columns(name, K):
    g = oc.base_graph(name)
    return np.ascontiguousarray(np.stack([fu.uniform_values(g.n, seed=oc.VALUE_SEED[name] + c) for c in range(K)],
                                         axis=1))


@functools.lru_cache(maxsize=None)
def _lossy_reference(name, how):
    g = oc.graph(name, how)
    down = link_mask(g, 0.1, 7)
    return down, lossy_reference(g, _rev_columns(name, MAX_K), LOSSY_STOPS, LOSSY_P, REV_LOSS_SEED, down)


@pytest.mark.parametrize("K", [1, MAX_K])
@pytest.mark.parametrize("name,how", REV_CASES)
def test_lossy_columns_on_reordered_rows(name, how, K):
    """p = 0.3 and a link mask on the reordered tile and chunk graphs: a lost slot keeps the
    node's own pair in its place in the chain, a delivered one gathers through the rev of the
    reordered rows; column c against the C oracle's replay of column c."""
    g = oc.graph(name, how)
    down, ref = _lossy_reference(name, how)
    with fu.CollectAllLossyBatch(g, _rev_columns(name, K), loss=LOSSY_P, seed=REV_LOSS_SEED) as eng:
        eng.set_link_mask(down)
        for stop in LOSSY_STOPS:
            eng.run(stop - eng.rounds_done)
            assert_same_bits(eng.estimates(), np.ascontiguousarray(ref[stop][0][:, :K]), (name, how, K, "estimates", stop))
            assert_same_bits(eng.flows(), np.ascontiguousarray(ref[stop][1][:, :K]), (name, how, K, "flows", stop))
        assert eng.stats[1] > 0


def _churn_script(g):
    """run(2); the mid-row slot of every heavy row down; run(2); everything up again; run(2)."""
    mid = np.array([g.rowptr[h] + (g.rowptr[h + 1] - g.rowptr[h]) // 2 for h in heavy_rows(g)], dtype=np.int64)
    assert len(mid)
    up = cut(g, np.ones(g.E, dtype=np.uint8), mid)
    return [("run", 2), ("topology", None, up), ("run", 2), ("topology", None, None), ("run", 2)]


@functools.lru_cache(maxsize=None)
def _churn_column(name, how, c):
    g = oc.graph(name, how)
    v = fu.uniform_values(g.n, seed=oc.VALUE_SEED[name] + c)
    return churn_python(*g.arrays(), v, _churn_script(g)).steps


@pytest.mark.parametrize("K", [1, MAX_K])
@pytest.mark.parametrize("name,how", REV_CASES)
def test_churn_columns_on_reordered_rows(name, how, K):
    """One topology change takes the mid-row slot of every heavy row down (the DOWN slot skipped
    inside a reordered chain, mid-chunk), the next brings it back (FRESH): estimates, flows, slot
    states and stats after every step against the rule on Python floats, column by column."""
    g = oc.graph(name, how)
    script = _churn_script(g)
    per = [_churn_column(name, how, c) for c in range(K)]
    steps = [Step(np.stack([p[q].a for p in per], axis=1), np.stack([p[q].f for p in per], axis=1), per[0][q].state,
                  per[0][q].alive_nodes, per[0][q].live_slots) for q in range(len(script))]
    with fu.CollectAllChurnBatch(g, _rev_columns(name, K)) as eng:
        drive_churn(eng, script, steps, (name, how, K))


# ------------------------------------------------------------------------------------
# the pair engine
# ------------------------------------------------------------------------------------
PAIR_ROUNDS = {"pair_class": (1, 2, 7, CLASS_ROUNDS), "dense66": (1, 2, 3)}


@functools.lru_cache(maxsize=None)
def _pair_reference(name, how, p, rounds):
    g = oc.graph(name, how)
    if p == 0.0:
        return oracle_pair(*g.arrays(), oc.values(name), rounds, SEED)[:3]
    return oracle_pair_loss(*g.arrays(), oc.values(name), rounds, SEED, hashed(p, LOSS_SEED, g.E))[:3]


@pytest.mark.parametrize("p", [0.0, CLASS_P])
@pytest.mark.parametrize("match", [0, 1])
@pytest.mark.parametrize("name,how", [(n, h) for n in ("pair_class", "dense66") for h in oc.GPU_HOWS[n]])
def test_pairs_on_reordered_rows(name, how, match, p):
    """The proposer's slot p_i picks j = col[rowptr[i] + p_i] of the caller's row and the answer
    lands on t = rev[..] - rowptr[j]; a fire sums the row's flows in row order (light lane groups
    and the heavy block's chunks of 1024 slots). Both matchers, lossless and at p = 0.3: last
    averages, flows, caches, stats and loss stats."""
    g, v = oc.graph(name, how), oc.values(name)
    arrays = g.arrays()
    lost = hashed(p, LOSS_SEED, g.E)
    with fu.PairwiseSync(g, v, seed=SEED, loss=p, loss_seed=LOSS_SEED if p else 0) as eng:
        eng.set_option("match", match)
        for r in PAIR_ROUNDS[name]:
            eng.run(r - eng.rounds_done)
            ref = _pair_reference(name, how, p, r)
            what = (name, how, "match", match, "p", p, "round", r)
            assert_same_bits(eng.estimates(), ref[0], what + ("last",))
            assert_same_bits(eng.flows(), ref[1], what + ("flows",))
            assert_same_bits(eng.cache(), ref[2], what + ("cache",))
        pairs = pair_count(*arrays, SEED, r)
        if p:
            m1, m2, full = loss_counts(*arrays, SEED, r, lost)
            assert eng.loss_stats == (m1, m2, full) and m1 + m2 + full == pairs and m1 and m2
            assert eng.stats == (pairs, g.n - len(fired_nodes(*arrays, SEED, r, lost)))
        else:
            ini, lis = roles(*arrays, SEED, r)
            assert eng.stats == (pairs, g.n - len(ini | lis)) and eng.loss_stats == (0, 0, pairs)


# ------------------------------------------------------------------------------------
# partitions on the in-process transport
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,kernel", [("cut_slivers", "recon"), ("cut_slivers", "stage"), ("cut_rmat", "recon"),
                                         ("cut_rmat", "stage"), ("cut_rmat", "pregather")])
def test_partitions_on_reordered_rows(name, kernel, world):
    """The two reordered cut cases at uneven bounds: every rank's rows keep the caller's order
    with ghost ids in place, and every rank's estimates and flows equal the single-graph
    oracle's slice at every stop. A rank that has no layout for the kernel asked for (the
    hub-only rank of the R-MAT cut has no light tile for kernel 8) refuses it and runs kernel
    4, as in test_dist_cuts_gpu."""
    from fu.dist import DistCollectAll, partition, run_local
    from test_dist_cuts_gpu import no_layout

    how = oc.GPU_HOWS[name][0]
    g, v, options = oc.graph(name, how), oc.values(name), oc.cut_options(name)
    bounds = oc.cut_bounds(name, world)
    plans = [partition(g.rowptr, g.col, g.rev, world, r, bounds=bounds) for r in range(world)]
    ref = oc.reference(name, how)
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
        done = 0
        for stop in oc.STOPS[name]:
            run_local(engs, stop - done)
            done = stop
            for p, e in zip(plans, engs):
                assert_same_bits(e.estimates(), np.ascontiguousarray(ref[stop][0][p.lo:p.hi]),
                                 (name, kernel, world, "rank", p.rank, "estimates", stop))
                assert_same_bits(e.flows(), np.ascontiguousarray(ref[stop][1][g.rowptr[p.lo]:g.rowptr[p.hi]]),
                                 (name, kernel, world, "rank", p.rank, "flows", stop))
    finally:
        for e in engs:
            e.close()
