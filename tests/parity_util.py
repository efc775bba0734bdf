"""Shared by the parity tests: the bit-pattern comparison behind every "bitwise" claim, and
the graph builders that more than one test module uses.

The contract (DESIGN, parity): every estimate and flow equals the reference's Python float
bit for bit wherever that float is not a NaN (the signs of zeros and infinities and every
subnormal included), and is a NaN exactly where the reference's is a NaN. A NaN's sign and
payload are not part of it: x86 generates 0xfff8000000000000, gfx950 0x7ff8000000000000,
and Python prints both as `nan`."""
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
