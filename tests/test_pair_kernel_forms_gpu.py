"""Two shapes of the pair engine's kernels (csrc/fu_pair.hip) beside test_pair_columns_gpu.py's:
kp_exchange_cols at widths where the lanes of a group disagree on having a second column, and
kp_heavy<Args, false> at K = 1 and at those widths, on the chunk edges of each. Every column
holds the bits of its own reference (pair_columns_cases.ref_column, ref_column_loss: the C
oracle's replay of that column alone), on last averages, flows and caches; the counters against
the helpers' counts. The conditions that make the cases meaningful are asserted in
test_pair_kernel_forms_case_inputs.py."""
import pytest

import fu
from pair_cases import SEED, pair_count, rr256_d8
from pair_columns_cases import BOUNDARY_ROUNDS, columns, ref_column, ref_column_loss
from pair_kernel_forms_cases import HEAVY_FORM_WIDTHS, HEAVY_LOSS_SEED, HEAVY_SEED, MIXED_WIDTHS, heavy_graph
from pair_loss_cases import CLASS_P, LOSS_SEED, fired_nodes, hashed, link_mask, loss_counts
from parity_util import assert_same_bits

pytestmark = pytest.mark.gpu


def _check(eng, refs, what):
    """refs[c] = (last, f, c) of column c."""
    est, fl, ca = eng.estimates(), eng.flows(), eng.cache()
    K = len(refs)
    assert est.shape == (eng.n, K) and fl.shape == (eng.E, K) and ca.shape == (eng.E, K), what
    for c, ref in enumerate(refs):
        assert_same_bits(est[:, c], ref[0], what + ("column", c, "last"))
        assert_same_bits(fl[:, c], ref[1], what + ("column", c, "flows"))
        assert_same_bits(ca[:, c], ref[2], what + ("column", c, "cache"))


def _refs(g, V, rounds, seed, lost=None, tag=None):
    if lost is None:
        return [ref_column(g, V[:, c], rounds, seed) for c in range(V.shape[1])]
    return [ref_column_loss(g, V[:, c], rounds, seed, lost, tag) for c in range(V.shape[1])]


def _check_counts(eng, g, seed, rounds, lost, what):
    """stats and loss_stats against the host's count of the outcomes; lost = None: no loss."""
    if lost is None:
        pairs = pair_count(*g.arrays(), seed, rounds)
        assert eng.stats[0] == pairs and eng.loss_stats == (0, 0, pairs), what
        return
    m1, m2, full = loss_counts(*g.arrays(), seed, rounds, lost)
    assert eng.loss_stats == (m1, m2, full), what
    assert eng.stats == (m1 + m2 + full, g.n - len(fired_nodes(*g.arrays(), seed, rounds, lost))), what


# ------------------------------------------------------------------------------------
# 1. a group whose lanes disagree on having a second column
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lossy", [False, True])
@pytest.mark.parametrize("K", MIXED_WIDTHS)
def test_mixed_widths_on_light_pairs(K, lossy):
    """test_pair_columns_gpu.test_every_width_on_light_pairs at K = 9 and 15, and the same run at
    p = 0.3 under a link mask."""
    g = rr256_d8()
    V = columns(g.n, K)
    down = link_mask(g)
    lost = hashed(CLASS_P, LOSS_SEED, g.E, down) if lossy else None
    kw = dict(seed=SEED, loss=CLASS_P, loss_seed=LOSS_SEED, link_mask=down) if lossy else dict(seed=SEED)
    with fu.PairwiseSyncBatch(g, V, **kw) as eng, fu.PairwiseSync(g, V[:, 0].copy(), **kw) as one:
        assert eng.K == K
        for r in (1, 5, 40):
            eng.run(r - eng.rounds_done)
            _check(eng, _refs(g, V, r, SEED, lost, "p+mask"), ("K", K, "lossy", lossy, "round", r))
        _check_counts(eng, g, SEED, 40, lost, (K, lossy))
        one.run(40)
        assert eng.stats == one.stats and eng.loss_stats == one.loss_stats
        assert eng.rounds_done == 40


# ------------------------------------------------------------------------------------
# 2. the K-column heavy kernel at one column and at the mixed widths
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lossy", [False, True])
@pytest.mark.parametrize("match", [0, 1])
@pytest.mark.parametrize("K", HEAVY_FORM_WIDTHS)
def test_heavy_form_at_its_chunk_edges(K, match, lossy):
    """Centres of 64, 65, cs, cs + 1 and 2 cs + 1 slots, cs = 2048 / K. At K = 1 a scalar handle
    of the same seeds runs beside it: kp_heavy<Args, true>, whose chunk of 1024 slots has its
    edges elsewhere in the same rows."""
    g = heavy_graph(K)
    V = columns(g.n, K)
    seed, loss_seed = HEAVY_SEED[K], HEAVY_LOSS_SEED[K]
    lost = hashed(CLASS_P, loss_seed, g.E) if lossy else None
    kw = dict(seed=seed, loss=CLASS_P, loss_seed=loss_seed) if lossy else dict(seed=seed)
    what = ("K", K, "match", match, "lossy", lossy)
    refs = _refs(g, V, BOUNDARY_ROUNDS, seed, lost, "p")
    with fu.PairwiseSyncBatch(g, V, **kw) as eng:
        eng.set_option("match", match)
        eng.run(BOUNDARY_ROUNDS)
        _check(eng, refs, what)
        _check_counts(eng, g, seed, BOUNDARY_ROUNDS, lost, what)
        if K == 1:
            with fu.PairwiseSync(g, V[:, 0].copy(), **kw) as one:
                one.set_option("match", match)
                one.run(BOUNDARY_ROUNDS)
                assert_same_bits(one.estimates(), refs[0][0], what + ("scalar", "last"))
                assert_same_bits(one.flows(), refs[0][1], what + ("scalar", "flows"))
                assert_same_bits(one.cache(), refs[0][2], what + ("scalar", "cache"))
                assert one.stats == eng.stats and one.loss_stats == eng.loss_stats
