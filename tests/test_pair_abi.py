"""The pairwise engine's C ABI without a GPU: symbols, argument errors (all checked before any
HIP call), the host restatement of the matching (fu_pair_matching) against Python ints, and
the test helper itself (tests/pair_cases.py): the trace for the pinned oracle against Python
floats, and its convergence."""
import ctypes

import numpy as np
import pytest

import fu
from fu import _lib as L
from lossy_cases import hub60
from pair_cases import class_graph, matching_py, oracle_pair, pair_count, pair_python, pairs_of_round, rr256_d8
from parity_util import assert_same_bits

PAIR_SYMBOLS = ["fu_pair_create", "fu_pair_create_from_graph", "fu_pair_set_seed", "fu_pair_set_option",
                "fu_pair_set_values", "fu_pair_reset", "fu_pair_run", "fu_pair_run_timed", "fu_pair_set_targets",
                "fu_pair_max_err", "fu_pair_get_estimates", "fu_pair_get_flows", "fu_pair_get_cache", "fu_pair_get_round",
                "fu_pair_get_stats", "fu_pair_synchronize", "fu_pair_destroy", "fu_pair_matching"]


def test_every_pair_symbol_loads():
    for s in PAIR_SYMBOLS:
        assert hasattr(L.lib, s), s
        assert s in L.EXPORTED
    assert L.lib.fu_version() == 2
    assert hasattr(fu, "PairwiseSync") and hasattr(fu, "pair_matching")


def _create(rp, col, rev, v):
    out = L.vp()
    rc = L.lib.fu_pair_create(len(rp) - 1, int(rp[-1]), L.ptr(rp), L.ptr(col), None if rev is None else L.ptr(rev),
                              L.ptr(v), 0, ctypes.byref(out))
    if rc == 0:
        L.lib.fu_pair_destroy(out)
    return rc


def test_asymmetric_csr_is_a_graph_error():
    rp = np.array([0, 1, 1], dtype=np.int64)
    col = np.array([1], dtype=np.int32)
    assert _create(rp, col, None, np.ones(2)) == -5
    assert "not symmetric" in L.last_error()
    with pytest.raises(fu.FuError) as ei:
        fu.PairwiseSync(rowptr=rp, col=col, values=np.ones(2))
    assert ei.value.code == -5
    g = fu.Graph.from_csr(rp, col, require_symmetric=False)
    with pytest.raises(fu.FuError) as ei:
        fu.PairwiseSync(g, np.ones(2))
    assert ei.value.code == -5


def test_wrong_caller_rev_is_a_graph_error():
    """Two entries of a correct rev swapped (both still in range), an entry out of range and a
    negative one: FU_ERR_GRAPH before any HIP call, so no bad access can reach a device."""
    g = hub60()
    rp, col, rev = g.arrays()
    v = np.ones(g.n)
    for bad in ("swap", "range", "negative"):
        r = rev.copy()
        if bad == "swap":
            r[[3, 57]] = r[[57, 3]]
        elif bad == "range":
            r[10] = g.E
        else:
            r[10] = -1
        assert _create(rp, col, r, v) == -5, bad
        assert "rev" in L.last_error()
    if fu.device_count() == 0:  # the correct rev passes every check and reaches the device probe
        assert _create(rp, col, rev, v) == -2
        assert "no HIP device" in L.last_error()


def test_other_bad_arguments():
    g = hub60()
    with pytest.raises(ValueError):
        fu.PairwiseSync(g, np.ones((g.n, 2)))
    with pytest.raises(ValueError):
        fu.PairwiseSync(g, np.ones(g.n + 1))
    rp, col, _ = g.arrays()
    c = col.copy()
    c[0] = g.n
    assert _create(rp, c, None, np.ones(g.n)) == -1
    assert _create(np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32), None, np.ones(1)) == -1  # n = 0
    assert L.lib.fu_pair_run(None, 1, 0, None) == -1
    assert L.lib.fu_pair_run(None, -1, 0, None) == -1
    assert L.lib.fu_pair_get_stats(None, None) == -1
    assert L.lib.fu_pair_set_seed(None, 1) == -1
    assert L.lib.fu_pair_set_option(None, b"match", 1) == -1
    mate, ini = np.zeros(g.n, dtype=np.int32), np.zeros(g.n, dtype=np.uint8)
    assert L.lib.fu_pair_matching(g.n, L.ptr(rp), L.ptr(col), 1, -1, L.ptr(mate), L.ptr(ini)) == -1  # round < 0
    assert L.lib.fu_pair_matching(g.n, L.ptr(rp), L.ptr(c), 1, 0, L.ptr(mate), L.ptr(ini)) == -1  # col out of range
    assert L.lib.fu_pair_matching(g.n, L.ptr(rp), L.ptr(col), 1, 0, None, L.ptr(ini)) == -1
    if fu.device_count() > 0:
        with fu.PairwiseSync(g, np.ones(g.n)) as eng:
            with pytest.raises(fu.FuError) as ei:
                eng.run(-1)
            assert ei.value.code == -1
            with pytest.raises(fu.FuError):
                eng.set_option("match", 2)
            with pytest.raises(fu.FuError):
                eng.run(2, err_every=1)  # no targets


# ------------------------------------------------------------------------------------
# the matching
# ------------------------------------------------------------------------------------
def _graphs():
    iso = fu.Graph.from_edges(9, [0, 1, 4], [1, 2, 5])  # nodes 3, 6, 7, 8 have degree 0
    return {"hub60": hub60(), "rr256_d8": rr256_d8(), "class": class_graph(), "isolated": iso}


@pytest.mark.parametrize("name", ["hub60", "rr256_d8", "class", "isolated"])
def test_matching_equals_python_ints_and_is_a_matching(name):
    g = _graphs()[name]
    rounds = (0, 1, 2, 1000) if name == "class" else (0, 1, 2, 3, 7, 1000, 2 ** 40)
    seeds = (0, 11) if name == "class" else (0, 11, 0xFEDCBA9876543210)
    src = np.repeat(np.arange(g.n), np.diff(g.rowptr))
    edges = set(zip(src.tolist(), g.col.tolist()))
    paired = 0
    for seed in seeds:
        for r in rounds:
            mate, ini = fu.pair_matching(g, seed, r)
            assert mate.dtype == np.int32 and ini.dtype == np.uint8
            m_py, i_py = matching_py(g.rowptr, g.col, seed, r)
            assert mate.tolist() == m_py and ini.tolist() == i_py, (seed, r)
            for i in range(g.n):
                j = int(mate[i])
                if j < 0:
                    assert ini[i] == 0
                    continue
                assert int(mate[j]) == i and (i, j) in edges
                assert int(ini[i]) + int(ini[j]) == 1  # exactly one initiator per pair
                paired += 1
            assert (mate[g.degrees == 0] == -1).all()
    assert paired > 0
    if name == "isolated":  # six nodes with edges: two rounds can well agree
        return
    a, b = fu.pair_matching(g, 11, 1), fu.pair_matching(g, 11, 2)
    assert not np.array_equal(a[0], b[0])
    assert not np.array_equal(a[0], fu.pair_matching(g, 12, 1)[0])


def test_matching_rate():
    """About 0.2 pairs per node and round on a regular graph of degree 8 (a CPU model of the rule
    gave 0.20-0.21): between 0.15 and 0.25 over 20 rounds of RR-256."""
    g = rr256_d8()
    pairs = pair_count(*g.arrays(), 5, 20)
    assert 0.15 < pairs / (20 * g.n) < 0.25


def test_matching_accepts_a_raw_csr_pair():
    g = hub60()
    a = fu.pair_matching(g, 3, 4)
    b = fu.pair_matching((g.rowptr, g.col), 3, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    mate, ini = fu.pair_matching((np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32)), 0, 0)
    assert mate.tolist() == [-1] and ini.tolist() == [0]


# ------------------------------------------------------------------------------------
# the helper itself (conditions on the yardstick: they hold without the engine)
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [1, 2, 30])
def test_helper_trace_equals_python_floats(rounds):
    g = hub60()
    v = fu.uniform_values(g.n, seed=4)
    last, f, c, _ = oracle_pair(*g.arrays(), v, rounds, 11)
    l_py, f_py, c_py = pair_python(*g.arrays(), v, rounds, 11)
    assert_same_bits(last, l_py, "last")
    assert_same_bits(f, f_py, "flows")
    assert_same_bits(c, c_py, "cache")
    assert np.count_nonzero(f) > 0
    # what step 3 leaves: antisymmetric flows, and both ends caching the listener's average
    rev = g.rev
    assert_same_bits(f[rev] + 0.0, -f + 0.0, "antisymmetry")
    assert_same_bits(c[rev], c, "cache symmetry")


CONV_ROUNDS = 400  # the helper needs 337 rounds on this graph, seed and inputs (printed below)


def test_helper_converges_to_the_mean():
    """On RR-256 (degree 8) the rule reaches 1e-9 of the mean within CONV_ROUNDS rounds, and the
    mass v_i - sum_k f[k] stays the inputs' mass (gossip averaging over the matching)."""
    g = rr256_d8()
    v = fu.uniform_values(g.n, seed=0)
    mean = float(np.mean(v))
    last, f, _, snaps = oracle_pair(*g.arrays(), v, CONV_ROUNDS, 0, snaps=tuple(range(CONV_ROUNDS)))
    err = np.array([np.max(np.abs(snaps[r] - mean)) for r in range(CONV_ROUNDS)])
    reached = np.flatnonzero(err <= 1e-9 * abs(mean))
    print("rounds to 1e-9 of the mean:", int(reached[0]) + 1 if len(reached) else None)
    assert len(reached) and reached[0] + 1 <= CONV_ROUNDS
    assert err[-1] <= 1e-9 * abs(mean)
    x = v - np.add.reduceat(f, g.rowptr[:-1])  # every row has 8 slots
    assert abs(float(np.sum(x)) - float(np.sum(v))) <= 1e-9 * abs(float(np.sum(v)))


def test_helper_pairs_are_consistent():
    g = hub60()
    rp, col, rev = g.arrays()
    for r in range(5):
        for i, s, j, t in pairs_of_round(rp, col, rev, 11, r):
            assert int(col[rp[i] + s]) == j and int(col[rp[j] + t]) == i and int(rev[rp[i] + s]) == int(rp[j]) + t
