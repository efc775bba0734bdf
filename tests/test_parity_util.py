"""The bit-pattern comparison itself (tests/parity_util.py), and the two oracles against each
other over the value families of tests/test_value_domain.py: the fixtures pin both oracles on
ordinary values only, and the GPU tests trust the C oracle on all of them."""
import numpy as np
import pytest

import coracle
import oracle
from parity_util import FAMILIES, assert_same_bits, count_neg_zero

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
