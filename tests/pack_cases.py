"""The inputs of tests/test_pack_edges_gpu.py (the packed estimate table at its window edges
and under option switches), shared with the CPU checks of their conditions in
tests/test_pack_case_inputs.py. Numpy, the host graph generators and the C oracle only:
nothing here touches a GPU.

The table (fu_ca_pack.h, "Packed estimate table"): an estimate a is stored as the code
off = dkey(a) - base when 0 <= off < esc (esc = 2^W - 1), else as the escape code esc, whose
reader gathers the double; base = centre - 2^(W-1). The plan takes the centre (the median key
of the first 64 sampled gather targets) and the width (the narrowest W whose window holds
4076 of the 4096 sampled keys) from the last round's estimates."""
import collections
import functools

import numpy as np

import coracle
import fu

M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------
# the order-preserving key of a double, and the plan's rule, restated in numpy
# ------------------------------------------------------------------------------------
def dkey(x):
    """uint64 keys of float64 values: negative values have all bits flipped, the others the
    sign bit set, so the keys order like the values (-0.0 right below +0.0)."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def dkey_inv(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    b = np.where(k >> np.uint64(63) != 0, k & np.uint64((1 << 63) - 1), ~k)
    return b.view(np.float64)


def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


PLAN_SAMPLES = 4096
PLAN_NEED = PLAN_SAMPLES - PLAN_SAMPLES // 200  # 4076: 99.5 % of the sample


def plan_sample(col):
    """The plan's fixed sample: the targets of 4096 pseudo-random edges (fu__create_common:
    col[splitmix_at(0x9ac4, q) % E], splitmix_at(s, i) = mix64(s + (i + 1) golden))."""
    E = len(col)
    idx = [_mix64((0x9AC4 + (q + 1) * 0x9E3779B97F4A7C15) & M64) % E for q in range(PLAN_SAMPLES)]
    return np.asarray(col)[idx]


def plan_of(a, sample):
    """(width, base) that the plan gives from the estimates a (plan_body): the centre is the
    key of rank 32 among the first 64 sampled keys, the window of W bits holds the keys at a
    distance d from it with d + 2 <= 2^(W-1)."""
    key = [int(k) for k in dkey(np.asarray(a)[sample])]
    c = sorted(key[:64])[32]
    d = [abs(k - c) for k in key]
    for w in (8, 16, 32):
        if sum(x + 2 <= 1 << (w - 1) for x in d) >= PLAN_NEED:
            return w, c - (1 << (w - 1))
    return 0, 0


def code_of(a, W, base):
    """The encoder's rule (put_code) for one estimate: its code, or None for the escape. The
    offset wraps like the kernel's unsigned subtraction; it is compared before any narrowing."""
    off = (int(dkey(np.float64(a).reshape(1))[0]) - base) & M64
    return off if off < (1 << W) - 1 else None


class OracleRun:
    """The C oracle advanced round by round: after(T) = (a, f) once T rounds (0 .. T-1) have
    run, for increasing T."""

    def __init__(self, g, v, nthreads=4):
        self.arr, self.v, self.nt, self.T = g.arrays(), v, nthreads, 0

    def after(self, T):
        assert T >= max(self.T, 1), (T, self.T)
        if self.T == 0:
            self.a, self.f = coracle.ca_sync(*self.arr, self.v, 1, nthreads=self.nt)
            self.T = 1
        if T > self.T:
            coracle.ca_rounds(*self.arr, self.v, T - self.T, self.a, self.f, nthreads=self.nt)
            self.T = T
        return self.a.copy(), self.f.copy()


# ------------------------------------------------------------------------------------
# pair_table: a constant estimate table chosen by the test
# ------------------------------------------------------------------------------------
# Disjoint pairs whose two nodes hold the same value v with 1 <= |v| < 4/3: round 0 gives v/2,
# and from round 1 on the estimate is v exactly and both flows are +0.0 (checked on the oracle
# by test_pack_case_inputs.py), so every round's table holds the input values.
PAIR_WIDTHS = (8, 16, 32)
PAIR_CENTRES = (1.25, -1.25)
N_PAIRS = 8192
SPREAD_SHARE = 0.05  # of the pairs, W >= 16: half at +2^(W-2), half at -2^(W-2)

PairTable = collections.namedtuple("PairTable", "g v W c base planted spread widths")


def pair_offsets(W):
    """The planted offsets off (key = base + off), by group."""
    esc = (1 << W) - 1
    alias = ([1 << W, (1 << W) + 5] if W < 32 else []) + [(1 << 32) + 3, 1 << 33]
    return {"low edge": [-2, -1, 0, 1], "escape": [esc - 2, esc - 1, esc, esc + 1], "alias": alias}


def spread_distance(W):
    """Where the spread pairs sit, as a distance from the centre in keys: 2^(W-2) is inside
    the W-bit window (d + 2 <= 2^(W-1)) and outside the next narrower one (2^(W-2) + 2 >
    2^(W/2-1) for W = 16 and 32), so 5 % of the sample rule out every narrower width."""
    return 1 << (W - 2)


@functools.lru_cache(maxsize=None)
def pair_table(W, centre, seed=0):
    """8192 pairs under a seeded permutation of the node ids (pair p = nodes perm[2p],
    perm[2p+1]: partners in different tiles but for ~1.5 % of the pairs). Keys: one pair per
    planted offset, 5 % of the pairs at +-2^(W-2) from the centre (W >= 16), the rest at the
    centre key c = dkey(centre). Returns the graph, the values, c, base = c - 2^(W-1),
    planted = {off: (node, partner)}, the spread pairs' node ids and the expected widths."""
    assert W in PAIR_WIDTHS and centre in PAIR_CENTRES
    rng = np.random.default_rng([seed, W, int(centre > 0)])
    c = int(dkey(np.array([centre]))[0])
    base = c - (1 << (W - 1))
    offs = list(dict.fromkeys(o for grp in pair_offsets(W).values() for o in grp))  # esc + 1 is 2^W
    keys = [(base + o) & M64 for o in offs]
    n_spread = int(SPREAD_SHARE * N_PAIRS) if W >= 16 else 0
    keys += [c + spread_distance(W) * (1 if k % 2 == 0 else -1) for k in range(n_spread)]
    keys += [c] * (N_PAIRS - len(keys))
    n = 2 * N_PAIRS
    while True:  # redrawn until no planted pair has both nodes in one 256-node tile
        perm = rng.permutation(n)
        s, d = perm[0::2], perm[1::2]
        if not (s[:len(offs)] // 256 == d[:len(offs)] // 256).any():
            break
    v = np.empty(n)
    pv = dkey_inv(np.array(keys, dtype=np.uint64))
    v[s] = pv
    v[d] = pv
    g = fu.Graph.from_edges(n, s, d)
    planted = {o: (int(s[k]), int(d[k])) for k, o in enumerate(offs)}
    spread = np.concatenate([s[len(offs):len(offs) + n_spread], d[len(offs):len(offs) + n_spread]])
    return PairTable(g, v, W, c, base, planted, spread, (W, W, W))


PAIR_CASES = [(W, centre) for W in PAIR_WIDTHS for centre in PAIR_CENTRES]
# total rounds run at each comparison (T rounds = rounds 0 .. T-1): the first rounds one by
# one, the rounds around the 8th and 16th (once the host has seen width 8 the plan runs every
# 8th round only, so until then the table may still carry round 1's base), and 40 / 41
PAIR_STOPS = (1, 2, 3, 4, 5, 6, 9, 10, 17, 18, 40, 41)


# ------------------------------------------------------------------------------------
# converging: small graphs whose table narrows to 8 bits within a few dozen rounds
# ------------------------------------------------------------------------------------
CONV_HUB, CONV_MEGA = 16, 64
Converging = collections.namedtuple("Converging", "g v sample")

# The first T (rounds run) at which the plan from a_{T-1} gives 32 / 16 / 8 bits, from the
# plan's rule applied to the C oracle's estimates after every round (seed 1;
# test_pack_case_inputs.py asserts them). The values span 2^12 keys, but the rounds start
# from zero state: round 0 gives v / (deg + 1), and on graphs of mixed degrees the estimates
# then close in on the mean by a constant factor per round, from a spread of order 1 down to
# 2^-37 (2^15 keys) before 16 bits fit. So no plan packs these inputs before round 100, however
# narrow the values are; a few hundred rounds of 4096 nodes still take milliseconds.
CONV_FIRST = {"er": {32: 102, 16: 185, 8: 224}, "rmat": {32: 153, 16: 281, 8: 341}}
CONV_ROUNDS = 360  # every width of both kinds is reached by then


@functools.lru_cache(maxsize=None)
def converging(kind, seed=1):
    """kind "er": ER(4096, 16384), run with hub_threshold 16 (degrees up to 19: heavy rows);
    "rmat": R-MAT scale 11, edge factor 8, which has rows in every row class once
    hub_threshold is 16 and mega_hub 64. Values 1 + U 2^-40."""
    if kind == "er":
        g = fu.Graph.erdos_renyi(4096, 16384, seed=seed)
    else:
        assert kind == "rmat"
        g = fu.Graph.rmat(11, 8, seed=seed)
    v = 1.0 + np.random.default_rng(seed).random(g.n) * 2.0 ** -40
    return Converging(g, v, plan_sample(g.col))


def first_round_of_widths(case, rounds):
    """{width: the first T at which the plan from a_{T-1} (the estimates after T rounds)
    gives it}, T = 1 .. rounds, and the list of widths by T."""
    run = OracleRun(case.g, case.v)
    seq = [plan_of(run.after(T)[0], case.sample)[0] for T in range(1, rounds + 1)]
    first = {}
    for T, w in enumerate(seq, start=1):
        first.setdefault(w, T)
    return first, seq
