"""Shared by the parity tests: the bit-pattern comparison behind every "bitwise" claim, and
the graph builders that more than one test module uses.

The contract (DESIGN, parity): every estimate and flow equals the reference's Python float
bit for bit wherever that float is not a NaN (the signs of zeros and infinities and every
subnormal included), and is a NaN exactly where the reference's is a NaN. A NaN's sign and
payload are not part of it: x86 generates 0xfff8000000000000, gfx950 0x7ff8000000000000,
and Python prints both as `nan`."""
import functools
import math

import numpy as np

import fu


def assert_same_bits(got, ref, what=""):
    """got and ref: float64 arrays of one shape, NaN at the same positions, and the same
    64-bit pattern at every other position (np.array_equal compares by value: it takes -0.0
    for +0.0 and fails on any NaN)."""
    got, ref = np.asarray(got), np.asarray(ref)
    tag = f"{what}: " if what != "" else ""
    assert got.dtype == np.float64 and ref.dtype == np.float64, f"{tag}dtypes {got.dtype}, {ref.dtype}: float64 wanted"
    assert got.shape == ref.shape, f"{tag}shapes {got.shape}, {ref.shape}"
    g = np.ascontiguousarray(got).reshape(-1)
    r = np.ascontiguousarray(ref).reshape(-1)
    gn, rn = np.isnan(g), np.isnan(r)
    bad = (gn != rn) | (~(gn | rn) & (g.view(np.uint64) != r.view(np.uint64)))
    if bad.any():
        k = int(np.argmax(bad))
        raise AssertionError(f"{tag}{int(bad.sum())} of {bad.size} differ, first at {k}: "
                             f"got 0x{int(g.view(np.uint64)[k]):016x} ({g[k]!r}), "
                             f"want 0x{int(r.view(np.uint64)[k]):016x} ({r[k]!r})")


def _er_with_outlier_pairs(n, m, pairs, seed):
    """ER(n, m) plus `pairs` disjoint 2-node components whose values are far from the giant
    component's mean: their estimates never enter the packed window, so every gather of
    them goes through the escape code."""
    g = fu.Graph.erdos_renyi(n, m, seed=seed)
    src = np.repeat(np.arange(g.n), np.diff(g.rowptr))
    keep = src < g.col
    ps = n + 2 * np.arange(pairs)
    s = np.concatenate([src[keep], ps])
    d = np.concatenate([g.col[keep], ps + 1])
    v = np.concatenate([fu.uniform_values(n, seed=seed), 1e6 + np.arange(2 * pairs, dtype=np.float64)])
    return fu.Graph.from_edges(n + 2 * pairs, s, d), v


CLASS_EDGE_DEGREES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024,
                      1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 12000]


def _class_edge_graph(seed):
    """Star centres of exactly the degrees above (each row class's first and last degree: heavy
    rows at > 128, multi-row blocks at > 256, the register launch's 1024, the mega hubs at >
    8192), their leaves drawn from a random background graph that never touches a centre."""
    rng = np.random.default_rng(seed)
    k, n_leaf = len(CLASS_EDGE_DEGREES), 16000
    n = k + n_leaf
    src, dst = [], []
    for c, d in enumerate(CLASS_EDGE_DEGREES):
        leaves = k + rng.choice(n_leaf, size=d, replace=False)
        src.append(np.full(d, c))
        dst.append(leaves)
    m = 3 * n_leaf
    src.append(k + rng.integers(0, n_leaf, m))
    dst.append(k + rng.integers(0, n_leaf, m))
    g = fu.Graph.from_edges(n, np.concatenate(src), np.concatenate(dst))
    assert [int(x) for x in g.degrees[:k]] == CLASS_EDGE_DEGREES
    return g


# ------------------------------------------------------------------------------------
# value families: functions of (n, seed), numpy only
# ------------------------------------------------------------------------------------
def _neg(n, seed):
    return -np.random.default_rng(seed).random(n)


def _sym(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def _wide(n, seed):
    """+-2^U(-60, 60): 36 decades, so a reassociated sum or a swapped operand shows in the
    high bits and not only in the last ulp."""
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(-60.0, 60.0, n)


def _ints(n, seed):
    return np.random.default_rng(seed).integers(0, 100, n).astype(np.float64)


def _binade(n, seed):
    """1 +- 5e-10: one binade boundary inside the cluster (the exponent changes at 1.0)."""
    return 1.0 + np.random.default_rng(seed).uniform(-5e-10, 5e-10, n)


def _subn(n, seed):
    """Mixed-sign subnormals within 50 ulps of zero: every quotient rounds to a multiple of
    2^-1074, many to -0.0 or +0.0, and the keys sit on both sides of the sign fold."""
    return np.random.default_rng(seed).integers(-50, 50, n) * 5e-324


def _huge(n, seed):
    """uniform(-1, 1) x 1.7e308: the left-to-right chains overflow, and where a chain first
    reaches +-inf (and so where inf - inf gives NaN) depends on the order of its elements."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n) * 1.7e308


FAMILIES = {"neg": _neg, "sym": _sym, "wide": _wide, "ints": _ints, "binade": _binade,
            "subn": _subn, "huge": _huge}


def count_neg_zero(x):
    """How many elements are -0.0 (bit pattern 0x8000000000000000)."""
    return int(np.count_nonzero(np.ascontiguousarray(x).view(np.uint64) == np.uint64(1 << 63)))


# ------------------------------------------------------------------------------------
# the packing cases of test_value_domain.py, shared with order_cases.py
# ------------------------------------------------------------------------------------
# components beside the giant one; their estimates never enter the packed window
NONFINITE_EXTRAS = [(np.inf, 1.0), (-np.inf, np.inf), (np.nan, 2.0), (-0.0, -0.0), (5e-324, -5e-324),
                    (1.7e308, 1.7e308, 1.7e308)]
FINITE_EXTRAS = [(-0.0, -0.0), (5e-324, -5e-324), (3.0, -7.0, 1e-300)]

# Total rounds at which each case stops. The widths come from the plan's rule (centre: the
# median key of the first 64 sampled gather targets; the narrowest width whose window holds
# 99.5 % of the 4096 sampled keys) applied on the CPU to the C oracle's estimates before
# every 4th round: the round whose plan first gives 32 / 16 / 8 bits is
#   neg 108 / 192 / 236, sym 144 / 228 / 272, binade 104 / 188 / 232, wide 160 / 244 / never.
# `wide` stays at 16 bits (checked to round 1200, and for two other seeds): the flows of the
# nodes whose value is near 2^60 carry roundings of up to 2^8, which leave those nodes'
# estimates, and their neighbours', thousands of ulps from a mean near 2^46; about 6 % of
# the values lie above 2^53, far more than the 0.5 % the 8-bit window may miss.
PACK_STOPS = {"neg": (160, 220, 300), "sym": (200, 256, 320), "binade": (160, 220, 300),
              "wide": (200, 280, 340)}
PACK_WIDTHS = {"neg": {32, 16, 8}, "sym": {32, 16, 8}, "binade": {32, 16, 8}, "wide": {32, 16}}


@functools.lru_cache(maxsize=None)
def _width_graph():
    """ER(20000, 80000): the graph of the batched engine's width cases and of its K = 16 error
    reduction case."""
    return fu.Graph.erdos_renyi(20_000, 80_000, seed=1)


# The batched engine's degree boundaries. Light rows (one thread per row and column): loads in
# groups of four edges, (fr, er) in registers up to degree 16, one block per row above 64.
# Heavy rows at width K: chunks of ce = 2048 // K edges, so a row of ce + 1 edges is the
# shortest with two chunks and one of 2 ce + 1 the shortest with three.
BATCH_LIGHT_DEGREES = [0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, 18, 63, 64, 65]


def batch_chunk_degrees(K):
    ce = 2048 // K
    return [ce - 1, ce, ce + 1, 2 * ce - 1, 2 * ce, 2 * ce + 1]


BATCH_BOUNDARY_DEGREES = sorted(set(BATCH_LIGHT_DEGREES).union(*(batch_chunk_degrees(K) for K in range(1, 17))))


@functools.lru_cache(maxsize=None)
def _batch_boundary_graph():
    """Star centres of exactly BATCH_BOUNDARY_DEGREES (node c has degree
    BATCH_BOUNDARY_DEGREES[c]), their leaves drawn from a sparse random background graph of 6000
    nodes that never touches a centre."""
    rng = np.random.default_rng(13)
    k, n_leaf = len(BATCH_BOUNDARY_DEGREES), 6000
    src, dst = [], []
    for c, d in enumerate(BATCH_BOUNDARY_DEGREES):
        src.append(np.full(d, c))
        dst.append(k + rng.choice(n_leaf, size=d, replace=False))
    src.append(k + rng.integers(0, n_leaf, 2 * n_leaf))
    dst.append(k + rng.integers(0, n_leaf, 2 * n_leaf))
    g = fu.Graph.from_edges(k + n_leaf, np.concatenate(src), np.concatenate(dst))
    assert [int(x) for x in g.degrees[:k]] == BATCH_BOUNDARY_DEGREES
    return g


def _isolated_then_heavy_rows(tail):
    """(n, n_leaf, first isolated row, isolated rows, heavy row, mega hub) of the graph below."""
    n_leaf, n_iso = 12000, 700
    if tail == "heavy_hub":
        iso0, heavy, hub = n_leaf, n_leaf + n_iso, n_leaf + n_iso + 1
    elif tail == "hub_iso_heavy":
        hub, iso0, heavy = n_leaf, n_leaf + 1, n_leaf + 1 + n_iso
    else:
        heavy, hub, iso0 = n_leaf, n_leaf + 1, n_leaf + 2
    return n_leaf + n_iso + 2, n_leaf, iso0, n_iso, heavy, hub


def _isolated_then_heavy_graph(tail):
    """Layout "given" with runs of isolated rows right before a heavy row and a mega hub:
    tail = "heavy_hub" puts [..., isolated x 700, heavy (300 edges), mega hub (9000 edges)] at
    the end, "hub_iso_heavy" [..., mega hub, isolated x 700, heavy], "iso_end" keeps the
    isolated run last (the k_isolated case)."""
    rng = np.random.default_rng(21)
    n, n_leaf, iso0, n_iso, heavy, hub = _isolated_then_heavy_rows(tail)
    base = rng.integers(0, n_leaf, size=(3 * n_leaf, 2))
    src, dst = [base[:, 0]], [base[:, 1]]
    src += [np.full(300, heavy), np.full(9000, hub)]
    dst += [rng.choice(n_leaf, 300, replace=False), rng.choice(n_leaf, 9000, replace=False)]
    g = fu.Graph.from_edges(n, np.concatenate(src), np.concatenate(dst))
    deg = g.degrees
    assert deg[heavy] == 300 and deg[hub] == 9000 and not deg[iso0:iso0 + n_iso].any()
    return g


# ------------------------------------------------------------------------------------
# planted targets: the error reduction (max_i |a_i - target_i|) with a chosen argmax
# ------------------------------------------------------------------------------------
# With component means as targets nothing controls which node holds the maximum, so a launch
# that drops its rows' contribution (or adds a spurious one) stays unseen whenever the
# maximum sits in another row class. Here the targets are the oracle's own last estimates,
# a_{R-1}, except at one probe node p, where D is added: at every round r < R node p alone
# holds the maximum, the expected entry np.max(np.abs(a_r - t)) is an exact IEEE subtraction
# and fabs on the oracle's doubles, and the runner-up says what a dropped contribution would
# have left.
def planted_D(a_rounds, shift=0):
    """The smallest power of two >= 4 max_{r,i} |a_r[i] - a_{R-1}[i]|, times 2^shift (shift
    tells apart the probes that are planted at once: ranks, columns). The factor 4 is
    headroom; the condition itself is planted_targets' assertion."""
    a_rounds = np.asarray(a_rounds)
    dev = float(np.max(np.abs(a_rounds - a_rounds[-1])))
    assert np.isfinite(dev) and dev > 0.0, dev
    m, e = math.frexp(4.0 * dev)  # 4 dev = m 2^e, 0.5 <= m < 1
    return math.ldexp(1.0, (e - 1 if m == 0.5 else e) + shift)


def planted_targets(a_rounds, p, D):
    """a_rounds: (R, n) oracle estimates of rounds 0 .. R-1. Returns (t, want_trace,
    runner_up): t = a_{R-1} with D added at node p; want_trace[r] = max_i |a_r[i] - t[i]|;
    runner_up[r] = the same maximum over i != p, which is what the entry collapses to when
    the launch that owns p drops its contribution. Asserts that at every round the maximum
    is attained at p only (runner_up[r] < |a_r[p] - t[p]|)."""
    a_rounds = np.asarray(a_rounds, dtype=np.float64)
    assert a_rounds.ndim == 2 and 0 <= p < a_rounds.shape[1]
    t = a_rounds[-1].copy()
    t[p] = t[p] + D
    err = np.abs(a_rounds - t)
    at_p = err[:, p].copy()
    err[:, p] = 0.0
    runner_up = err.max(axis=1)
    bad = ~(runner_up < at_p)
    if bad.any():
        r = int(np.argmax(bad))
        raise AssertionError(f"probe {p}, D = {D!r}: at round {r} the probe's error {at_p[r]!r} does not exceed "
                             f"the runner-up {runner_up[r]!r} at node {int(np.argmax(err[r]))}")
    return t, np.maximum(at_p, runner_up), runner_up
