"""The inputs of test_pair_kernel_forms_gpu.py held to the conditions that make them meaningful, on
the host alone (pair_cases' and pair_loss_cases' restatements: no GPU)."""
import pytest

from pair_cases import SEED, roles, rr256_d8
from pair_columns_cases import BOUNDARY_ROUNDS, LIGHT_WIDTHS, HEAVY_WIDTHS, boundary_degrees, chunk_slots
from pair_kernel_forms_cases import HEAVY_FORM_WIDTHS, HEAVY_LEAVES, HEAVY_LOSS_SEED, HEAVY_SEED, MIXED_WIDTHS, heavy_graph
from pair_loss_cases import CLASS_P, LOSS_SEED, census, hashed, link_mask, outcomes

GROUP = 8  # csrc/fu_pair.hip kGroup: lane l of a pair's group carries columns l and l + 8


def _lanes(K):
    """(lanes of a group with two columns, lanes with exactly one) at width K."""
    two = sum(1 for l in range(GROUP) if l + GROUP < K)
    return two, min(K, GROUP) - two


def test_the_mixed_widths_are_the_ones_the_light_widths_leave_out():
    assert all(0 in _lanes(K) for K in LIGHT_WIDTHS)  # all of one kind
    assert [_lanes(K) for K in MIXED_WIDTHS] == [(1, 7), (7, 1)]
    assert not set(HEAVY_FORM_WIDTHS) & set(HEAVY_WIDTHS)


def test_each_outcome_on_the_light_graph_under_loss_and_mask():
    g = rr256_d8()
    down = link_mask(g)
    assert 0 < int(down.sum()) < g.E
    oc = outcomes(*g.arrays(), SEED, 40, hashed(CLASS_P, LOSS_SEED, g.E, down))
    cen = census(g, oc)
    assert all(x > 0 for x in cen["light"]) and not any(cen["heavy_i"] + cen["heavy_j"]), cen


@pytest.mark.parametrize("K", HEAVY_FORM_WIDTHS)
def test_heavy_graph_centres_sit_on_the_chunk_edges(K):
    cs = chunk_slots(K)
    assert cs == 2048 // K and boundary_degrees(K) == [64, 65, cs, cs + 1, 2 * cs + 1]
    assert 2 * cs + 1 <= HEAVY_LEAVES[K]  # a centre's leaves are distinct
    g = heavy_graph(K)
    assert [int(d) for d in g.degrees[:5]] == boundary_degrees(K) and g.n == 5 + HEAVY_LEAVES[K]
    assert int(g.degrees[5:].max()) <= 64  # the leaves stay in the lane groups
    assert not (g.col[g.rowptr[0]:g.rowptr[5]] < 5).any()  # no centre touches a centre
    if K == 1:  # the scalar handle's chunk of 1024 slots has its edges elsewhere in these rows
        assert [int(d) % 1024 for d in g.degrees[2:5]] == [0, 1, 1] and [int(d) // 1024 for d in g.degrees[2:5]] == [2, 2, 4]


@pytest.mark.parametrize("K", HEAVY_FORM_WIDTHS)
def test_every_heavy_graph_centre_initiates_and_listens(K):
    g = heavy_graph(K)
    ini, lis = roles(*g.arrays(), HEAVY_SEED[K], BOUNDARY_ROUNDS)
    assert set(range(5)) <= ini and set(range(5)) <= lis


@pytest.mark.parametrize("K", HEAVY_FORM_WIDTHS)
def test_each_outcome_on_a_heavy_pair_in_both_roles(K):
    g = heavy_graph(K)
    oc = outcomes(*g.arrays(), HEAVY_SEED[K], BOUNDARY_ROUNDS, hashed(CLASS_P, HEAVY_LOSS_SEED[K], g.E))
    cen = census(g, oc)
    assert all(x > 0 for x in cen["light"] + cen["heavy_i"] + cen["heavy_j"]), cen
