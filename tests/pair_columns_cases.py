"""Shared by the tests of the pairwise engine with K value columns (fu.PairwiseSyncBatch;
csrc/fu_pair.hip kp_exchange_cols and kp_heavy<Args, false>): the widths, the columns, the K-dependent
chunk of the heavy kernel and a graph whose star centres sit on its edges, and the per-column
references. The reference of column c is always pair_cases' or pair_loss_cases' restatement run on
column c alone; nothing here runs the engine.

The conditions that make the inputs meaningful are asserted in test_pair_columns_case_inputs.py.
"""
import functools

import numpy as np

import fu
from pair_cases import oracle_pair
from pair_loss_cases import oracle_pair_loss

# A lane of a pair's group of 8 carries columns l and l + 8: one column, fewer than 8, not a
# divisor of 8, exactly 8 (no lane has a second), 16 (every lane has two).
LIGHT_WIDTHS = (1, 2, 3, 5, 8, 16)
# kp_heavy<Args, false>: threads 0 .. K-1 carry a column each; the chunk shrinks with K.
HEAVY_WIDTHS = (2, 3, 16)

COLS_CHUNK = 2048  # csrc/fu_pair.hip kColsChunk: doubles staged per chunk of a heavy row


def chunk_slots(K):
    """Slots of a heavy row that kp_heavy<Args, false> stages at once at K columns."""
    return COLS_CHUNK // K


def columns(n, K, seed=0):
    """(n, K) inputs whose columns differ in scale, sign and offset: column c is
    (-8)^c * U_c + c with U_c the uniform stream at seed + c, so a column read from its
    neighbour's place is off by orders of magnitude."""
    return np.ascontiguousarray(np.stack([(-8.0) ** c * fu.uniform_values(n, seed=seed + c) + c for c in range(K)], axis=1))


def boundary_degrees(K):
    """The lane groups end at 64 slots; the heavy kernel's chunk edges at K columns."""
    cs = chunk_slots(K)
    return [64, 65, cs, cs + 1, 2 * cs + 1]


BOUNDARY_LEAVES = 3000


@functools.lru_cache(maxsize=None)
def boundary_graph(K, n_leaf=BOUNDARY_LEAVES):
    """Star centres of exactly boundary_degrees(K) (node c has degree boundary_degrees(K)[c]),
    their leaves drawn from a random background graph of n_leaf (3000) nodes that never touches
    a centre: pair_cases.class_graph at the K-column kernel's own edges. A centre's leaves are
    distinct, so K = 1 (a centre of 4097 slots) needs more leaves than the default."""
    rng = np.random.default_rng(100 + K)
    degs = boundary_degrees(K)
    k = len(degs)
    src, dst = [], []
    for c, d in enumerate(degs):
        src.append(np.full(d, c))
        dst.append(k + rng.choice(n_leaf, size=d, replace=False))
    src.append(k + rng.integers(0, n_leaf, 2 * n_leaf))
    dst.append(k + rng.integers(0, n_leaf, 2 * n_leaf))
    g = fu.Graph.from_edges(k + n_leaf, np.concatenate(src), np.concatenate(dst))
    assert [int(x) for x in g.degrees[:k]] == degs
    return g


# The runs on boundary_graph(K): BOUNDARY_ROUNDS rounds at the matching seed BOUNDARY_SEED[K],
# within which every centre both initiates and listens; and per centre whose degree is one above
# a chunk edge, (centre, seed, rounds) of a short run in whose last round that centre's pair
# stands on a slot of the row's final, partial chunk. Found by a search over seeds with
# fu.pair_matching on the host; test_pair_columns_case_inputs.py holds them to it.
BOUNDARY_ROUNDS = 40
BOUNDARY_SEED = {2: 1, 3: 1, 16: 1}
PARTIAL_CHUNK_RUNS = {2: ((3, 422, 2), (4, 837, 4)), 3: ((3, 124, 1), (4, 501, 1)), 16: ((3, 29, 3), (4, 181, 2))}


def partial_chunk_centres(K):
    """{centre: first slot of its row's final partial chunk} for the degrees cs + 1 and 2 cs + 1."""
    cs = chunk_slots(K)
    return {3: cs, 4: 2 * cs}


# ------------------------------------------------------------------------------------
# per-column references, computed once per (graph, column, ...) and shared
# ------------------------------------------------------------------------------------
_REFS = {}


def _key(g, v):
    return (g.n, g.E, g.col.tobytes(), np.ascontiguousarray(v).tobytes())


def ref_column(g, v, rounds, seed):
    """pair_cases.oracle_pair of one column, (last, f, c)."""
    k = ("plain", _key(g, v), rounds, seed)
    if k not in _REFS:
        _REFS[k] = oracle_pair(*g.arrays(), np.ascontiguousarray(v), rounds, seed)[:3]
    return _REFS[k]


def ref_column_loss(g, v, rounds, seed, lost, tag):
    """pair_loss_cases.oracle_pair_loss of one column, (last, f, c); `tag` names `lost` in the
    cache key."""
    k = ("loss", _key(g, v), rounds, seed, tag)
    if k not in _REFS:
        _REFS[k] = oracle_pair_loss(*g.arrays(), np.ascontiguousarray(v), rounds, seed, lost)[:3]
    return _REFS[k]
