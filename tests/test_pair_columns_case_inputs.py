"""The inputs of test_pair_columns_gpu.py held to the conditions that make them meaningful, on
the host alone (fu.pair_matching and pair_cases.matching_py: no GPU)."""
import numpy as np
import pytest

import fu
from lossy_cases import M64, splitmix_at_py
from pair_columns_cases import (BOUNDARY_ROUNDS, BOUNDARY_SEED, COLS_CHUNK, HEAVY_WIDTHS, LIGHT_WIDTHS, PARTIAL_CHUNK_RUNS,
                                boundary_degrees, boundary_graph, chunk_slots, columns, partial_chunk_centres)
from pair_cases import matching_py, roles
from pair_loss_cases import CLASS_P, LOSS_SEED, census, hashed, outcomes


def test_widths_and_chunks():
    assert LIGHT_WIDTHS == (1, 2, 3, 5, 8, 16) and HEAVY_WIDTHS == (2, 3, 16)
    assert [chunk_slots(K) for K in HEAVY_WIDTHS] == [1024, 682, 128] and COLS_CHUNK == 2048
    for K in HEAVY_WIDTHS:
        cs = chunk_slots(K)
        assert cs * K <= COLS_CHUNK < (cs + 1) * K
        degs = boundary_degrees(K)
        assert degs == [64, 65, cs, cs + 1, 2 * cs + 1] and len(set(degs)) == 5
        g = boundary_graph(K)
        assert [int(d) for d in g.degrees[:5]] == degs
        assert int(g.degrees[5:].max()) <= 64  # the leaves stay in the lane groups
        assert not (g.col[g.rowptr[0]:g.rowptr[5]] < 5).any()  # no centre touches a centre


def test_columns_differ_in_scale():
    v = columns(256, 16)
    assert v.shape == (256, 16) and v.flags["C_CONTIGUOUS"]
    top = np.abs(v).max(axis=0)
    assert (top[2:] > 4.0 * top[1:-1]).all()  # every column dwarfs the one before it
    assert len({v[:, c].tobytes() for c in range(16)}) == 16
    assert np.array_equal(columns(256, 5), v[:, :5])  # width K is the first K columns


@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_every_boundary_centre_initiates_and_listens(K):
    g = boundary_graph(K)
    ini, lis = roles(*g.arrays(), BOUNDARY_SEED[K], BOUNDARY_ROUNDS)
    assert set(range(5)) <= ini and set(range(5)) <= lis
    # the host restatement in C agrees with the one on Python ints
    for r in (0, BOUNDARY_ROUNDS - 1):
        mate, init = fu.pair_matching(g, BOUNDARY_SEED[K], r)
        m2, i2 = matching_py(g.rowptr, g.col, BOUNDARY_SEED[K], r)
        assert mate.tolist() == m2 and init.tolist() == i2


def _centre_slot(g, seed, r, c):
    """The slot of centre c's own row on which its pair of round r stands, or None."""
    mate, init = fu.pair_matching(g, seed, r)
    if mate[c] < 0:
        return None
    b, d = int(g.rowptr[c]), int(g.degrees[c])
    if init[c]:
        return (splitmix_at_py(splitmix_at_py(seed & M64, r), c) >> 1) % d
    (s,) = np.flatnonzero(g.col[b:b + d] == mate[c])
    return int(s)


@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_a_pair_stands_in_the_final_partial_chunk(K):
    g = boundary_graph(K)
    first = partial_chunk_centres(K)
    runs = PARTIAL_CHUNK_RUNS[K]
    assert sorted(c for c, _, _ in runs) == sorted(first)
    for c, seed, rounds in runs:
        d = int(g.degrees[c])
        assert d % chunk_slots(K) == 1  # one above a chunk edge: the final chunk holds one slot
        s = _centre_slot(g, seed, rounds - 1, c)
        assert s is not None and first[c] <= s < d, (K, c, s)


@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_each_outcome_on_a_heavy_and_on_a_light_pair(K):
    g = boundary_graph(K)
    oc = outcomes(*g.arrays(), BOUNDARY_SEED[K], BOUNDARY_ROUNDS, hashed(CLASS_P, LOSS_SEED, g.E))
    cen = census(g, oc)
    assert all(x > 0 for x in cen["light"]), cen
    assert all(a + b > 0 for a, b in zip(cen["heavy_i"], cen["heavy_j"])), cen
