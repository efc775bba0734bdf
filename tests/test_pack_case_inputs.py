"""CPU checks of the inputs of tests/test_pack_edges_gpu.py (tests/pack_cases.py): the pair
tables really are constant from round 1 on, their planted keys sit on the offsets they claim
and fall on the side of the escape that the encoder's rule gives them, and the plan's rule,
restated in numpy and applied to the C oracle's estimates, predicts the widths the GPU tests
assert. No GPU: the C oracle and numpy only."""
import numpy as np
import pytest

from pack_cases import (CONV_FIRST, CONV_HUB, CONV_MEGA, CONV_ROUNDS, M64, N_PAIRS, PAIR_CASES, PAIR_STOPS,
                        PLAN_NEED, PLAN_SAMPLES, OracleRun, code_of, converging, dkey, dkey_inv,
                        first_round_of_widths, pair_offsets, pair_table, plan_of, plan_sample, spread_distance)
from parity_util import assert_same_bits


def test_dkey_orders_like_the_values_and_inverts():
    x = np.array([-np.inf, -1.7e308, -1.25, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1.25, 1.7e308, np.inf])
    k = dkey(x)
    assert (np.diff(k.astype(object)) > 0).all()
    assert int(k[6]) - int(k[5]) == 1  # -0.0 and +0.0 are neighbours
    assert int(dkey(np.array([np.nextafter(1.25, 2.0)]))[0]) - int(dkey(np.array([1.25]))[0]) == 1
    assert int(dkey(np.array([np.nextafter(-1.25, 0.0)]))[0]) - int(dkey(np.array([-1.25]))[0]) == 1
    assert_same_bits(dkey_inv(k), x)


def test_plan_sample_is_the_fixed_edge_sample():
    """splitmix_at(0x9ac4, q) for q = 0, 1 by hand (SplitMix64's finaliser on seed + (q + 1)
    golden), and the sample's size."""
    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    col = np.arange(1000, dtype=np.int32)
    s = plan_sample(col)
    assert len(s) == PLAN_SAMPLES and PLAN_NEED == 4076
    assert s[0] == mix(0x9AC4 + 0x9E3779B97F4A7C15) % 1000
    assert s[1] == mix((0x9AC4 + 2 * 0x9E3779B97F4A7C15) & M64) % 1000


@pytest.mark.parametrize("W,centre", PAIR_CASES)
def test_pair_table_is_constant_and_planted_where_it_says(W, centre):
    p = pair_table(W, centre)
    g, v = p.g, p.v
    esc = (1 << W) - 1
    # the graph: 8192 disjoint pairs, partners with equal values, 1 <= |v| < 4/3
    assert g.n == 2 * N_PAIRS and g.E == g.n and (g.degrees == 1).all()
    assert (g.col[g.col] == np.arange(g.n)).all()
    assert_same_bits(v[g.col], v)
    assert (np.abs(v) >= 1.0).all() and (np.abs(v) < 4.0 / 3.0).all() and (np.sign(v) == np.sign(centre)).all()
    far = np.arange(g.n) // 256 != g.col // 256
    assert far.mean() > 0.95  # partners in another tile
    # the fixed point: v from round 1 on (T rounds = rounds 0 .. T-1), every flow +0.0
    run = OracleRun(g, v)
    a0, f0 = run.after(1)
    assert_same_bits(a0, v / 2.0, "round 0")
    sample = plan_sample(g.col)
    widths = {1: plan_of(a0, sample)[0]}
    for T in range(2, max(PAIR_STOPS) + 1):
        a, f = run.after(T)
        assert_same_bits(a, v, f"estimates after round {T - 1}")
        assert_same_bits(f, np.zeros(g.E), f"flows after round {T - 1}")  # +0.0, not -0.0
        widths[T], base = plan_of(a, sample)
        assert base == p.base, T
    # the plan from a_0 = v / 2 (same key distances, one binade down) already gives W, so
    # both table slots and the plan carry W once rounds 1 and 2 have run
    assert set(widths.values()) == {W}, widths
    assert p.widths == (W, W, W)
    # planted keys and the side of the escape they fall on (the encoder: 0 <= off < esc)
    key = dkey(v)
    offs = [o for grp in pair_offsets(W).values() for o in grp]
    assert set(p.planted) == set(offs)
    assert {-2, -1, 0, 1, esc - 2, esc - 1, esc, esc + 1, (1 << 32) + 3, 1 << 33} <= set(offs)
    assert W == 32 or {1 << W, (1 << W) + 5} <= set(offs)
    n_escaped = 0
    for off, (i, j) in p.planted.items():
        assert int(g.col[i]) == j and i // 256 != j // 256, off
        assert int(key[i]) == int(key[j]) == (p.base + off) & M64, off
        want = off if 0 <= off < esc else None
        assert code_of(v[i], W, p.base) == want, off
        if want is None:  # what a narrowing put in front of the compare would store instead
            n_escaped += 2
            alias = off & ((1 << W) - 1) if off >= 0 else None
            assert off < 0 or off == esc or alias < esc, off
    assert code_of(v[p.planted[-1][0]], W, p.base) is None  # reached through the unsigned wrap only
    assert ((int(key[p.planted[-1][0]]) - p.base) & M64) == M64
    assert n_escaped / g.n < 0.002
    # everything else: the centre (code 2^(W-1)) and, for W >= 16, 5 % at +-2^(W-2)
    rest = np.ones(g.n, dtype=bool)
    rest[[x for ij in p.planted.values() for x in ij]] = False
    d = key[rest].astype(object) - p.c
    if W == 8:
        assert len(p.spread) == 0 and (d == 0).all()
    else:
        D = spread_distance(W)
        assert D + 2 <= 1 << (W - 1) and D + 2 > 1 << (W // 2 - 1)
        assert set(d) == {0, D, -D}
        assert abs((d != 0).mean() - 0.05) < 0.001 and abs((d == D).sum() - (d == -D).sum()) <= 2
        assert (np.sort(np.nonzero(rest & (key != np.uint64(p.c)))[0]) == np.sort(p.spread)).all()
    # any sample of 4096 would do: the nodes outside each window, against the 20 the plan allows
    outside = {w: float(np.mean([abs(int(k) - p.c) + 2 > 1 << (w - 1) for k in key])) for w in (8, 16, 32)}
    assert outside[W] < 0.002, outside  # ~8 expected in the sample, 20 allowed
    assert all(outside[w] > 0.04 for w in (8, 16, 32) if w < W), outside  # ~200 expected


@pytest.mark.parametrize("kind", ["er", "rmat"])
def test_converging_cases_reach_every_width(kind):
    cs = converging(kind)
    deg = cs.g.degrees
    if kind == "er":
        assert cs.g.n == 4096 and (deg > CONV_HUB).any() and (deg <= CONV_HUB).any()
    else:  # light, heavy, mega-hub rows; kernel 9's classes above 128 and 256 edges
        assert cs.g.n == 2048
        for lo, hi in ((0, CONV_HUB), (CONV_HUB, CONV_MEGA), (CONV_MEGA, 128), (128, 256), (256, 1024)):
            assert ((deg > lo) & (deg <= hi)).any(), (lo, hi)
    assert (cs.v >= 1.0).all() and (cs.v < 1.0 + 2.0 ** -40).all()
    first, seq = first_round_of_widths(cs, CONV_ROUNDS)
    assert {w: first[w] for w in (32, 16, 8)} == CONV_FIRST[kind]
    # unpacked before the first 32, packed ever after (a width may flicker back at a
    # threshold: the GPU tests read the width they are at), and 8 bits at the end
    assert not any(seq[:first[32] - 1]) and all(seq[first[32] - 1:]) and seq[-1] == 8
