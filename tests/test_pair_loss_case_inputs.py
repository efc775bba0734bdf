"""Conditions on the yardstick of tests/test_pair_loss_gpu.py, without the engine: the two
restatements of the lossy pairwise round (pair_loss_cases) agree bit for bit, both equal the
reference's recording (tests/golden/rule_pair_lossy_hub_mix.npz), and the inputs of the GPU cases
make every kernel path meet every outcome."""
import os

import numpy as np
import pytest

import fu
import vd_cases
from pair_cases import (CLASS_DEGREES, CLASS_ROUNDS, LAST_SLOT_ROUNDS, LAST_SLOT_SEED, SEED, Recorded, class_graph, dense66,
                        rr256_d8)
from pair_loss_cases import (CLASS_P, COMPLETE, CONV_P, CONV_ROUNDS, LOSS_SEED, M1_LOST, M2_LOST, MASK_CLEARED_AT, VD_ROUNDS,
                             census, fired_nodes, hashed, link_mask, load_recording, loss_counts, oracle_pair_loss, outcomes,
                             pair_loss_python)
from parity_util import assert_same_bits, count_neg_zero

GOLDEN_FILE = os.path.join(os.path.dirname(__file__), "golden", "rule_pair_lossy_hub_mix.npz")


@pytest.mark.parametrize("p", [0.1, 0.5, 1.0])
def test_python_floats_equal_the_oracle_trace(p):
    g = rr256_d8()
    v = fu.uniform_values(g.n, seed=0)
    lost = hashed(p, LOSS_SEED, g.E)
    py = pair_loss_python(*g.arrays(), v, 60, SEED, lost)
    c = oracle_pair_loss(*g.arrays(), v, 60, SEED, lost)
    for a, b, what in zip(py, c, ("last", "flows", "cache")):
        assert_same_bits(a, b, (p, what))
    m1, m2, full = loss_counts(*g.arrays(), SEED, 60, lost)
    if p == 1.0:
        assert m2 == full == 0 and m1 > 0
        ini = {i for pairs in outcomes(*g.arrays(), SEED, 60, lost) for i, *_ in pairs}
        assert fired_nodes(*g.arrays(), SEED, 60, lost) == ini and 0 < len(ini) <= g.n
    else:
        assert min(m1, m2, full) > 50
        # a lost answer leaves the link's two flows not negating each other somewhere
        assert np.count_nonzero(py[1][g.rev] + py[1]) > 0


def test_no_loss_is_the_lossless_helper():
    from pair_cases import oracle_pair

    g = rr256_d8()
    v = fu.uniform_values(g.n, seed=0)
    a = oracle_pair_loss(*g.arrays(), v, 40, SEED, hashed(0.0, LOSS_SEED, g.E, np.zeros(g.E, dtype=np.uint8)))
    b = oracle_pair(*g.arrays(), v, 40, SEED)
    for x, y in zip(a[:3], b[:3]):
        assert_same_bits(x, y, "p = 0")


def test_both_restatements_equal_the_recording():
    """hub_mix at the recorded matching, p = 0.25, loss seed 3 and a mask over about 5 % of the
    links: what the reference's own avg_and_send / on_receive left after 5, 20 and 40 rounds with
    the lost messages dropped. The recorded `lost` bits are the engine's decision restated.

    Within the 40 rounds node 0 (degree 2101) meets, as initiator, 2 pairs with m1 lost, 2 with
    m2 lost and 7 complete, as listener 7 / 5 / 10; node 1 (degree 130) as initiator 2 / 3 / 1,
    as listener 7 / 3 / 15. All pairs: 2363 / 1536 / 4504."""
    d = load_recording()
    assert os.path.getsize(GOLDEN_FILE) <= 452_000
    assert tuple(int(x) for x in d.python.split(".")[:2]) < (3, 12)
    assert d.stops == [5, 20, 40] and d.p == 0.25 and d.lost.shape == (40, d.E)
    assert 0.03 < d.down.mean() < 0.07 and np.array_equal(d.down, d.down[d.rev])
    for r in (0, 1, 39):
        assert np.array_equal(d.lost[r], hashed(d.p, d.loss_seed, d.E, d.down)(r)), r
        mate, ini = fu.pair_matching((d.rowptr, d.col), d.seed, r)
        assert np.array_equal(mate, d.mate[r]) and np.array_equal(ini, d.initiator[r])
    rec = Recorded(d.mate, d.initiator)
    oc = outcomes(d.rowptr, d.col, d.rev, rec, 40, lambda r: d.lost[r])
    cnt = {(h, role): [0, 0, 0] for h in (0, 1) for role in "IL"}
    for pairs in oc:
        for i, _, j, _, o in pairs:
            if i in (0, 1):
                cnt[(i, "I")][o] += 1
            if j in (0, 1):
                cnt[(j, "L")][o] += 1
    assert cnt == {(0, "I"): [2, 2, 7], (0, "L"): [7, 5, 10], (1, "I"): [2, 3, 1], (1, "L"): [7, 3, 15]}
    assert all(min(c) >= 1 for c in cnt.values())
    assert loss_counts(d.rowptr, d.col, d.rev, rec, 40, lambda r: d.lost[r]) == (2363, 1536, 4504)
    for q, stop in enumerate(d.stops):
        want = (d.last_avg[q], d.flows[q], d.estimates[q])
        py = pair_loss_python(d.rowptr, d.col, d.rev, d.values, stop, rec, lambda r: d.lost[r])
        c = oracle_pair_loss(d.rowptr, d.col, d.rev, d.values, stop, rec, lambda r: d.lost[r])
        for a, b, w, what in zip(py, c, want, ("last", "flows", "cache")):
            assert_same_bits(a, w, ("python floats", stop, what))
            assert_same_bits(b, w, ("oracle trace", stop, what))


def _all_three(c, what):
    assert min(c) >= 1, (what, c)


def test_degree_boundary_inputs_meet_every_outcome_on_every_path():
    """class_graph() at SEED, p = 0.3, loss seed 5, 40 rounds: pairs with the heavy row on the
    initiator's side 13 / 11 / 14 (m1 lost / m2 lost / complete), on the listener's side
    26 / 19 / 58, light pairs 4930 / 3517 / 8245."""
    g = class_graph()
    c = census(g, outcomes(*g.arrays(), SEED, CLASS_ROUNDS, hashed(CLASS_P, LOSS_SEED, g.E)))
    assert c == {"heavy_i": [13, 11, 14], "heavy_j": [26, 19, 58], "light": [4930, 3517, 8245]}
    for k, v in c.items():
        _all_three(v, k)


def test_last_slot_run_delivers_m1_into_the_second_chunk():
    """At LAST_SLOT_SEED the centre of degree 1025 listens on slot 1024 in round 4; at loss seed 5
    its m1 arrives (so -F1 stands alone in the row's second chunk) and the answer is lost."""
    g = class_graph()
    c1025 = CLASS_DEGREES.index(1025)
    oc = outcomes(*g.arrays(), LAST_SLOT_SEED, LAST_SLOT_ROUNDS, hashed(CLASS_P, LOSS_SEED, g.E))
    hit = [(t, o) for i, s, j, t, o in oc[LAST_SLOT_ROUNDS - 2] if j == c1025]
    assert hit == [(1024, M2_LOST)]


def test_dense66_inputs():
    """More than 1024 heavy pairs in each of 3 rounds, with every outcome among them."""
    g = dense66()
    for pairs in outcomes(*g.arrays(), SEED, 3, hashed(CLASS_P, LOSS_SEED, g.E)):
        assert len(pairs) > 1024
        _all_three([sum(1 for x in pairs if x[4] == o) for o in (M1_LOST, M2_LOST, COMPLETE)], "dense66")


def test_mask_alone_inputs():
    """The mask of the mask-alone case is down in both directions on some links and in one
    direction on others, and forces every outcome on the heavy and on the light path while it is
    set; once cleared every exchange is complete."""
    g = class_graph()
    down = link_mask(g)
    both = (down != 0) & (down[g.rev] != 0)
    one = (down != 0) & (down[g.rev] == 0)
    assert both.sum() > 100 and one.sum() > 100
    lost = hashed(0.0, 0, g.E, lambda r: down if r < MASK_CLEARED_AT else None)
    oc = outcomes(*g.arrays(), SEED, CLASS_ROUNDS, lost)
    c = census(g, oc[:MASK_CLEARED_AT])
    assert c == {"heavy_i": [6, 2, 12], "heavy_j": [13, 4, 32], "light": [2407, 804, 5086]}
    for k, v in c.items():
        _all_three(v, k)
    after = census(g, oc[MASK_CLEARED_AT:])
    assert all(v[0] == v[1] == 0 for v in after.values()) and after["light"][2] > 0


@pytest.mark.parametrize("family", vd_cases.RULE_FAMILIES)
def test_value_domain_inputs_reach_the_edges(family):
    """hub_mix with the `subn` / `special` inputs at p = 0.3, 16 rounds: the Python floats reach
    -0.0 (subn) and NaN (special: 4 each in last averages, flows and caches; the infinite inputs
    have turned into NaN or have not fired by then) while most entries stay finite, and more than
    100 first messages are lost on the way."""
    d, g = vd_cases.rule("pair", family)
    lost = hashed(CLASS_P, LOSS_SEED, g.E)
    last, f, c = pair_loss_python(g.rowptr, g.col, g.rev, d.values, VD_ROUNDS, g.seed, lost)
    if family == "subn":
        assert count_neg_zero(last) + count_neg_zero(f) + count_neg_zero(c) > 0
    else:
        assert np.isnan(last).any() and np.isnan(f).any() and np.isnan(c).any()
        assert np.isinf(d.values).any() and np.isfinite(last).sum() > len(last) // 2
    assert loss_counts(g.rowptr, g.col, g.rev, g.seed, VD_ROUNDS, lost)[0] > 100


def test_the_reference_converges_under_loss():
    """rr256_d8, p = 0.1: after CONV_ROUNDS = 1500 rounds the reference's own error is below 1e-6
    of its error before round 0 (3.0e-13 of it on these inputs)."""
    g = rr256_d8()
    v = fu.uniform_values(g.n, seed=0)
    tgt, _ = fu.component_means(g.rowptr, g.col, v)
    _, _, _, sn = oracle_pair_loss(*g.arrays(), v, CONV_ROUNDS, SEED, hashed(CONV_P, LOSS_SEED, g.E), snaps=(CONV_ROUNDS - 1,))
    e0 = float(np.max(np.abs(np.zeros(g.n) - tgt)))
    e1 = float(np.max(np.abs(sn[CONV_ROUNDS - 1] - tgt)))
    print("error before round 0:", e0, "after", CONV_ROUNDS, "rounds:", e1)
    assert e1 < 1e-6 * e0
