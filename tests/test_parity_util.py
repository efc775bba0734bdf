"""The bit-pattern comparison itself (tests/parity_util.py), and the two oracles against each
other over the value families of tests/test_value_domain.py: the fixtures pin both oracles on
ordinary values only, and the GPU tests trust the C oracle on all of them."""
import math

import numpy as np
import pytest

import coracle
import oracle
from err_cases import (ERR_BATCH_KS, ERR_CHURN_DECOY, ERR_DIST_CASES, ERR_GRID, ERR_RMAT_HUB, ERR_RMAT_MEGA,
                       LIGHT_TILE_GEOMETRIES, PLANTED_CASES, dist_thresholds, err_batch_case, err_batch_nonfinite_rows,
                       err_churn_reducer_case, err_class_case, err_dist_case, err_isolated_case, err_rmat_case,
                       light_tiles, planted_conditions, rows_with_ghosts, with_decoys)
from parity_util import (CLASS_EDGE_DEGREES, FAMILIES, assert_same_bits, count_neg_zero, planted_D,
                         planted_targets)

QNAN_POS = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
QNAN_NEG = np.array([0xFFF8000000000000], dtype=np.uint64).view(np.float64)[0]


@pytest.mark.parametrize("got,ref", [
    ([1.0, -0.0], [1.0, 0.0]),                       # zero sign
    ([1.0, 2.0], [np.nextafter(1.0, 2.0), 2.0]),     # one ulp
    ([5e-324], [1e-323]),                            # one ulp among the subnormals
    ([np.nan, 2.0], [1.0, 2.0]),                     # NaN against a number
    ([1.0, 2.0], [1.0, np.nan]),                     # a number against NaN
    ([np.inf], [-np.inf]),                           # inf sign
    ([np.nan], [np.inf]),
    ([1.0, 2.0], [1.0, 2.0, 3.0]),                   # shape
    ([[1.0, 2.0]], [1.0, 2.0]),
])
def test_assert_same_bits_rejects(got, ref):
    with pytest.raises(AssertionError):
        assert_same_bits(np.array(got, dtype=np.float64), np.array(ref, dtype=np.float64))


def test_assert_same_bits_rejects_other_dtypes():
    with pytest.raises(AssertionError, match="float64"):
        assert_same_bits(np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32))
    with pytest.raises(AssertionError, match="float64"):
        assert_same_bits(np.zeros(3), np.zeros(3, dtype=np.int64))


def test_assert_same_bits_accepts():
    assert np.isnan(QNAN_POS) and np.isnan(QNAN_NEG)
    assert_same_bits(np.array([QNAN_POS, 1.0]), np.array([QNAN_NEG, 1.0]))  # NaN sign: not compared
    x = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -2.5e-320, np.inf, -np.inf, np.nan, 1.0])
    assert_same_bits(x, x.copy())
    assert_same_bits(x.reshape(2, 5), x.copy().reshape(2, 5))
    assert_same_bits(x[::2], x[::2].copy())  # strided views
    assert_same_bits(np.empty(0), np.empty(0))
    assert count_neg_zero(x) == 1


def test_assert_same_bits_report():
    """The message carries the number of mismatches, the first index and both patterns."""
    got = np.array([1.0, -0.0, 3.0, -0.0])
    ref = np.array([1.0, 0.0, 3.0, 0.0])
    with pytest.raises(AssertionError) as e:
        assert_same_bits(got, ref, what=("flows", 7))
    msg = str(e.value)
    assert "2 of 4 differ" in msg and "first at 1" in msg and "('flows', 7)" in msg
    assert "0x8000000000000000" in msg and "0x0000000000000000" in msg


def _star_graph():
    """About 300 nodes: a random background, a 40-leaf star whose centre is node 0, and node 1
    with no edge at all; rows in ascending neighbour order."""
    rng = np.random.default_rng(11)
    n = 300
    e = rng.integers(2, n, size=(450, 2))
    e = e[e[:, 0] != e[:, 1]]
    leaves = rng.choice(np.arange(2, n), size=40, replace=False)
    pairs = np.concatenate([e, np.stack([np.zeros(40, dtype=np.int64), leaves], axis=1)])
    pairs = np.unique(np.concatenate([pairs, pairs[:, ::-1]]), axis=0)  # symmetric, sorted by (src, dst)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, pairs[:, 0] + 1, 1)
    rowptr = np.cumsum(rowptr)
    deg = np.diff(rowptr)
    assert deg[0] == 40 and deg[1] == 0
    return rowptr, pairs[:, 1].astype(np.int32)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_c_oracle_matches_numpy_oracle_on_value_families(family):
    """coracle.ca_sync (what the GPU tests compare against) and oracle.ca_sync (the numpy
    restatement) agree after 1, 2, 5 and 40 rounds on every value family: signed zeros,
    subnormals, overflow to +-inf and the NaNs that follow, at the same positions."""
    rowptr, col = _star_graph()
    rev = oracle.build_rev(rowptr, col)
    v = FAMILIES[family](len(rowptr) - 1, seed=5)
    with np.errstate(all="ignore"):  # `huge` overflows by construction
        snaps = oracle.ca_sync(rowptr, col, v, 40, rev=rev, snapshot_rounds=[0, 1, 4, 39])
    for rounds in (1, 2, 5, 40):
        a, f = coracle.ca_sync(rowptr, col, rev, v, rounds, nthreads=2)
        assert_same_bits(a, snaps[rounds - 1][0], (family, rounds, "estimates"))
        assert_same_bits(f, snaps[rounds - 1][1], (family, rounds, "flows"))
    if family == "subn":
        assert count_neg_zero(snaps[39][0]) > 0  # the inputs do reach -0.0
    if family == "huge":
        assert np.isnan(snaps[39][0]).any() and np.isinf(snaps[4][1]).any()


# ------------------------------------------------------------------------------------
# planted targets (parity_util.planted_targets): the helper itself, and the uniqueness
# condition on the inputs of every case of tests/test_err_paths.py, from the oracle alone
# ------------------------------------------------------------------------------------
def test_planted_targets_hand_made():
    """Five nodes, three rounds, probe 3, D = 8: every entry worked out by hand (all values
    are small dyadic numbers, so every subtraction is exact)."""
    a = np.array([[0.0, 4.0, -2.0, 1.0, 8.0],
                  [1.0, 3.0, -1.0, 2.5, 6.0],
                  [1.5, 2.5, -0.5, 3.0, 5.0]])
    assert planted_D(a) == 16.0  # 4 x |8 - 5| = 12 -> 16
    assert planted_D(a, shift=2) == 64.0
    assert planted_D(np.array([[2.0, 0.0], [0.0, 0.0]])) == 8.0  # a power of two stays: 4 x 2
    t, want, runner_up = planted_targets(a, 3, 8.0)
    assert_same_bits(t, np.array([1.5, 2.5, -0.5, 11.0, 5.0]))
    assert_same_bits(want, np.array([10.0, 8.5, 8.0]))       # |1 - 11|, |2.5 - 11|, |3 - 11|
    assert_same_bits(runner_up, np.array([3.0, 1.0, 0.0]))   # node 4: |8 - 5|, |6 - 5|; +0.0 at the end
    for r in range(3):
        assert want[r] == np.max(np.abs(a[r] - t))


def test_planted_targets_raises_when_D_is_too_small():
    a = np.array([[0.0, 4.0, -2.0, 1.0, 8.0],
                  [1.5, 2.5, -0.5, 3.0, 5.0]])
    with pytest.raises(AssertionError, match="runner-up"):
        planted_targets(a, 3, 0.5)   # round 0: |1 - 3.5| = 2.5 against node 4's |8 - 5| = 3
    with pytest.raises(AssertionError, match="runner-up"):
        planted_targets(a, 3, 1.0)   # a tie, |1 - 4| = 3: the maximum must be at the probe only
    with pytest.raises(AssertionError, match="runner-up"):
        planted_targets(a, 3, 0.0)   # no probe at all: the last round's 0 is not below 0
    _, want, runner_up = planted_targets(a, 3, 2.0)
    assert_same_bits(want, np.array([4.0, 2.0]))
    assert_same_bits(runner_up, np.array([3.0, 0.0]))


@pytest.mark.parametrize("case", PLANTED_CASES)
def test_planted_inputs_have_a_unique_maximum(case):
    """For every (oracle rounds, probe, D) that tests/test_err_paths.py plants, the probe alone
    holds the maximum at every round (planted_targets asserts it), D is a power of two of at
    least 4 max |a_r - a_{R-1}| over the rows it is planted among (that the probes planted
    at once, ranks and columns, have distinct D is checked below)."""
    conds = planted_conditions(case)
    assert len(conds) > 0
    for a, p, D in conds:
        assert math.frexp(D)[0] == 0.5 and D >= 4.0 * np.max(np.abs(a - a[-1])), (case, p, D)
        _, want, runner_up = planted_targets(a, p, D)
        assert np.all(runner_up < want) and runner_up[-1] == 0.0
        assert abs(want[-1] - D) <= D * 2.0 ** -40  # D itself, up to the rounding of a + D


def test_churn_reducer_decoys_are_dead_where_named():
    """kc_max_err's case: the probes are alive, the three decoys dead, one in block 0, one in
    the last block of the first stride (1024 blocks of 256) and one in the second stride; about a
    tenth of the nodes are dead and stay at 0.0; D exceeds every honest error, and the decoys'
    2^20 D would be the maximum if a dead node entered it."""
    g, v, alive, a, probes, decoys = err_churn_reducer_case()
    stride = ERR_GRID * 256
    assert g.n > stride and probes == [0, 255, 256, stride - 1, stride, g.n - 1]
    assert alive[probes].all() and not alive[decoys].any()
    assert 0 <= decoys[0] < 256 and stride - 256 <= decoys[1] < stride <= decoys[2] < g.n
    assert 0.08 < 1.0 - alive.mean() < 0.12
    assert not a[:, alive == 0].any() and (a[-1][alive != 0] != 0.0).all()
    D = planted_D(a)
    assert D > 2.0 * np.max(np.abs(a - a[-1]))
    for p in probes:
        t, want, _ = planted_targets(a, p, D)
        td = with_decoys(t, a[-1], decoys, D)
        assert np.array_equal(np.flatnonzero(td != t), decoys)
        assert np.all(np.abs(a[:, decoys] - td[decoys]) == ERR_CHURN_DECOY * D) and np.all(want < ERR_CHURN_DECOY * D)
        assert_same_bits(np.max(np.abs(a - td)[:, alive != 0], axis=1), want)


def test_planted_cases_cover_what_they_name():
    """Conditions on the graphs behind the probes: the row classes the probes are meant to
    sit in exist where the cases look for them."""
    g, _, _, probes = err_class_case()
    deg = g.degrees
    assert set(range(len(CLASS_EDGE_DEGREES))) <= set(probes) and g.n - 1 in probes
    assert not (deg[len(CLASS_EDGE_DEGREES):] == 0).any()  # centre 0 is the only empty row, so
    last = np.argsort(-deg, kind="stable")[-5:]            # the degree layout's last five rows
    assert set(int(x) for x in last) <= set(probes) and 0 in last  # stand in for the degree-0 rows
    assert len(probes) >= 28 + 2 + 12 + 2
    g, _, _, probes = err_rmat_case()
    deg = g.degrees
    assert all(deg[p] > ERR_RMAT_MEGA for p in probes[:3])
    assert all(ERR_RMAT_HUB < deg[p] <= ERR_RMAT_MEGA for p in probes[3:6])
    assert probes[6] == g.n - 1 and len(probes) >= 14
    g, _, _, probes = err_isolated_case("heavy_hub")
    last = np.argsort(-g.degrees, kind="stable")[-700:]  # the degree layout ends in the 700 empty rows
    assert not g.degrees[last].any() and set(probes[:3]) <= set(int(x) for x in last)
    for K in ERR_BATCH_KS:
        g, _, _, probes, D = err_batch_case(K)
        assert len(set(D)) == K and len(set(probes)) == 7
        assert len({c for _, c in probes}) > 1  # more than one column is planted
    g, hub, iso = err_batch_nonfinite_rows()
    assert g.degrees[iso] == 0 and g.degrees[hub] == g.max_deg > 16


@pytest.mark.parametrize("kind,world", ERR_DIST_CASES)
def test_partition_probes_are_of_the_kind_they_name(kind, world):
    """The rows that the partition cases plant, per rank: each is what its name says, at least
    5 of them are distinct rows, and every rank's D differs. Tile membership, with the light
    tiles cut as the engine cuts them, for every geometry a light launch can have: "ghost"
    always lies in a boundary tile; on the random geometric graph every rank has boundary and
    interior tiles and "interior" lies in an interior one (the partitioned round's second
    light launch); on ER and R-MAT no rank has an interior tile at all, which is why the
    random geometric cases exist."""
    _, _, _, plans, probes, D, kinds = err_dist_case(kind, world)
    hub, mega = dist_thresholds(kind)
    assert len(set(D)) == world
    for p in plans:
        mine = kinds[p.rank]
        deg = np.diff(p.rowptr)
        has_ghost = rows_with_ghosts(p)
        assert p.n_ghost_a > 0 and has_ghost.any()
        assert all(0 <= r < p.n_local for r in mine.values()) and len(set(mine.values())) >= 5
        assert {row[p.rank] for row in probes} == set(mine.values())  # every kind is planted
        assert mine["first"] == 0 and mine["last"] == p.n_local - 1
        assert deg[mine["longest"]] == deg.max()
        assert has_ghost[mine["ghost"]] and deg[mine["ghost"]] <= min(hub, mega)
        if "no_ghost" in mine:
            assert not has_ghost[mine["no_ghost"]] and 0 < deg[mine["no_ghost"]] <= min(hub, mega)
        if "mega_ghost" in mine:
            assert has_ghost[mine["mega_ghost"]] and deg[mine["mega_ghost"]] > mega
            assert mine["mega_ghost"] != mine["longest"]
        for te, tn in LIGHT_TILE_GEOMETRIES:
            tiles = light_tiles(p.rowptr, te, tn, hub, mega)
            boundary = [bool(has_ghost[b:e].any()) for b, e in tiles]
            tile_of = {r: k for k, (b, e) in enumerate(tiles) for r in mine.values() if b <= r < e}
            assert boundary[tile_of[mine["ghost"]]]
            if kind == "rgg":
                assert 0 < sum(boundary) < len(tiles), (p.rank, te, tn)
                assert not boundary[tile_of[mine["interior"]]], (p.rank, te, tn)
            else:
                assert all(boundary), (p.rank, te, tn)
