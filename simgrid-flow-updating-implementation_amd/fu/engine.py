"""Device engines behind the C ABI.

* `CollectAll`: generation-synchronous collect-all rounds on one GPU (fu_create /
  fu_run_collectall). One round = Peer.on_receive for every directed edge + Peer.avg_and_send
  for every node (flowupdating-collectall.py:93-128), as one data-parallel kernel.
* `CollectAllBatch`: the same rounds for K value columns over one graph in one pass
  (fu_batch_*): AVG, COUNT, SUM, moments and histogram bins share the graph reads and one
  K-wide estimate gather per edge; each column is bit-equal to a `CollectAll` run.
* `CollectAllLossy`: the same rounds with a loss model (fu_lossy_*): a lost message makes the
  receiver fire on its own stored flow and estimate; the reverse flow is gathered through rev.
* `CollectAllChurn`: the same rounds while nodes and links leave and join (fu_churn_*): a slot
  state per directed slot (UP, DOWN, FRESH); a removed neighbour drops out of both sums and of
  the divisor, an added one starts from zeros; `churn_live` / `churn_targets` on the host.
* `CollectAllLossyBatch`, `CollectAllChurnBatch`: K value columns under one loss pattern or one
  topology (fu_lossy_create_k, fu_churn_create_k): one col, rev, kind and loss decision per
  slot, K-wide contiguous gathers; each column bit-equal to a run of the scalar class.
* `PairwiseSync`: synchronous pairwise rounds (fu_pair_*): a matching per round chosen on the
  device, one full pairwise exchange per matched pair; `pair_matching` restates it on the host.
* `PairwiseSyncBatch`: K value columns over one matching (fu_pair_create_k): one pointer chain,
  one loss decision and K contiguous flows per pair; each column bit-equal to a `PairwiseSync`.
* `Trace` + `Replay`: the tick-level schedule of the reference run (Peer.loop, CA:70-85 /
  PW:69-84, and the SimGrid mailboxes), built natively on the host and replayed on the
  GPU one tick per batch. Used by the pairwise mode and by faithful small-platform runs.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .graph import Graph, components, means_of_components

KERNELS = {"auto": 0, "recon": 4, "stage": 8, "pregather": 9}
LAYOUTS = {"given": 0, "degree": 1}
MODE = {"collectall": 0, "ca": 0, "pairwise": 1, "pw": 1}


def handle_info(h) -> dict:
    """Kernel in use (after autotuning), autotune state, rounds done."""
    a = np.zeros(32, dtype=np.int64)
    L.call("fu_get_info", h, L.ptr(a))
    names = {4: "recon", 8: "stage", 9: "pregather"}
    return {"kernel": names.get(int(a[0]), int(a[0])),
            "autotune": ["off", "pending", "done"][int(a[2])], "rounds": int(a[3]),
            "tile": (int(a[4]), int(a[5])), "tune_passes": int(a[6]),
            "tuned_pack_width": int(a[7]), "mega_hubs": int(a[20]),
            "stage_slices": [int(x) for x in a[27:31]],
            "tune_winner_by_width": {w: _cand_name(int(a[23 + k])) for k, w in
                                     enumerate((0, 8, 16, 32)) if a[23 + k] >= 0},
            "tune_us_per_round": {k: a[8 + i] / 1e3 for i, k in
                                  enumerate(TUNE_CANDIDATES)}}


# fu_plan.h kCands order
TUNE_CANDIDATES = ("recon", "recon_512", "stage", "recon_1024", "pregather")


def _cand_name(code: int) -> str:
    kernel, geo = divmod(code, 10)
    if kernel == 8:
        return "stage"
    if kernel == 9:
        return "pregather"
    return "recon" + {3: "_512", 1: "_1024", 2: "_1024x256"}.get(geo, "")


_OPS = ("create", "create_from_graph", "destroy", "reset", "set_targets", "set_values", "run", "run_timed", "max_err",
        "get_estimates", "get_flows", "get_round", "get_stats", "synchronize")


def _c_names(prefix: str, **irregular) -> dict:
    """Operation -> C entry point: prefix + operation, but for the names given."""
    return {**{op: prefix + op for op in _OPS}, **irregular}


class _Handle:
    """What the round engines share on the Python side: one device handle `_h` behind the C
    entry points named in `_C`, n nodes, E slots and `_cols` values per node (None: one, and
    arrays of shape (n,); K: arrays of shape (n, K))."""

    _C: dict = {}
    _cols = None
    _NDIM = 1
    _ROWS = "len(values)"  # how the class's messages call the number of value rows
    _REV_LEN_CHECKED = True

    def _call(self, op: str, *args):
        return L.call(self._C[op], self._h, *args)

    def _shape(self, rows: int) -> tuple:
        return (rows,) if self._cols is None else (rows, self._cols)

    def _open(self, graph, values, rowptr, col, rev, device, extra=lambda v: ()):
        """The handle from a Graph or a raw CSR; extra(values) goes in front of the values in
        the C call (the batch's K)."""
        v = np.asarray(values, dtype=np.float64)
        if v.ndim != self._NDIM:
            raise ValueError(f"values must have shape {'(n,)' if self._NDIM == 1 else '(n, K)'}, got {v.shape}")
        self.values = np.ascontiguousarray(v)
        extra = extra(v)
        out = L.vp()
        if graph is not None:
            if v.shape[0] != graph.n:
                raise ValueError(f"{self._ROWS} != graph.n")
            L.call(self._C["create_from_graph"], graph._h, *extra, L.ptr(self.values), int(device), ctypes.byref(out))
            self.n, self.E = graph.n, graph.E
        else:
            rp = np.ascontiguousarray(rowptr, dtype=np.int64)
            c = np.ascontiguousarray(col, dtype=np.int32)
            r = None if rev is None else np.ascontiguousarray(rev, dtype=np.int32)
            n = len(rp) - 1
            if v.shape[0] != n:
                raise ValueError(f"{self._ROWS} != n")
            if self._REV_LEN_CHECKED and r is not None and len(r) != len(c):
                raise ValueError("len(rev) != len(col)")
            L.call(self._C["create"], n, int(rp[-1]), L.ptr(rp), L.ptr(c), L.ptr(r), *extra, L.ptr(self.values),
                   int(device), ctypes.byref(out))
            self.n, self.E = n, int(rp[-1])
        self._h = out

    def reset(self):
        self._call("reset")

    def set_targets(self, target):
        t = np.ascontiguousarray(target, dtype=np.float64)
        if t.shape != self._shape(self.n):
            raise ValueError(f"targets must have shape {self._shape(self.n)}, got {t.shape}")
        self._call("set_targets", L.ptr(t))

    def _set_values(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.shape != self._shape(self.n):
            raise ValueError(f"values must have shape {self._shape(self.n)}, got {v.shape}")
        self._call("set_values", L.ptr(v))
        self.values = v

    def run(self, rounds: int, err_every: int = 0):
        """Run `rounds` rounds; with err_every > 0 returns the max-error trace."""
        if err_every > 0:
            trace = np.empty(self._shape(max(rounds // err_every, 1)))
            self._call("run", int(rounds), int(err_every), L.ptr(trace))
            return trace[:rounds // err_every]
        self._call("run", int(rounds), 0, None)
        return None

    def run_timed(self, rounds: int) -> float:
        """Device milliseconds for `rounds` rounds (HIP events on the handle's stream)."""
        ms = L.f32()
        self._call("run_timed", int(rounds), ctypes.byref(ms))
        return float(ms.value)

    def max_err(self):
        out = np.empty(self._cols or 1)
        self._call("max_err", out.ctypes.data_as(L.P(L.f64)))
        return out if self._cols else float(out[0])

    def estimates(self) -> np.ndarray:
        a = np.empty(self._shape(self.n))
        self._call("get_estimates", L.ptr(a))
        return a

    def flows(self) -> np.ndarray:
        f = np.empty(self._shape(max(self.E, 1)))
        self._call("get_flows", L.ptr(f))
        return f[:self.E]

    @property
    def rounds_done(self) -> int:
        r = L.i64()
        self._call("get_round", ctypes.byref(r))
        return int(r.value)

    def _stats(self) -> tuple:
        s = np.zeros(2, dtype=np.int64)
        self._call("get_stats", L.ptr(s))
        return int(s[0]), int(s[1])

    def synchronize(self):
        self._call("synchronize")

    def close(self):
        if getattr(self, "_h", None):
            getattr(L.lib, self._C["destroy"])(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class CollectAll(_Handle):
    """Synchronous collect-all engine on one GPU.

    >>> g = Graph.erdos_renyi(1_000_000, 4_000_000, seed=1)
    >>> eng = CollectAll(g, uniform_values(g.n, seed=0))
    >>> eng.run(1000); est = eng.estimates()
    """

    _C = _c_names("fu_", run="fu_run_collectall", run_timed="fu_run_collectall_timed")

    def __init__(self, graph: Graph | None = None, values=None, *, rowptr=None, col=None,
                 rev=None, device: int = 0, kernel: str | int = "auto",
                 hub_threshold: int | None = None, layout: str = "given"):
        """layout "degree" relabels the device graph by degree (fu_create_from_graph_ex):
        the most-gathered estimates share cache lines; inputs and outputs keep the caller's
        numbering, bits per node unchanged."""
        self.values = np.ascontiguousarray(values, dtype=np.float64)
        out = L.vp()
        if graph is not None:
            if len(self.values) != graph.n:
                raise ValueError("len(values) != graph.n")
            L.call("fu_create_from_graph_ex", graph._h, L.ptr(self.values), int(device),
                   LAYOUTS[layout], ctypes.byref(out))
            self.n, self.E = graph.n, graph.E
        else:
            if layout != "given":
                raise ValueError("layout needs a Graph")
            rp = np.ascontiguousarray(rowptr, dtype=np.int64)
            c = np.ascontiguousarray(col, dtype=np.int32)
            r = None if rev is None else np.ascontiguousarray(rev, dtype=np.int32)
            n = len(rp) - 1
            if len(self.values) != n:
                raise ValueError("len(values) != n")
            L.call("fu_create", n, int(rp[-1]), L.ptr(rp), L.ptr(c), L.ptr(r),
                   L.ptr(self.values), int(device), ctypes.byref(out))
            self.n, self.E = n, int(rp[-1])
        self._h = out
        if hub_threshold is not None:
            self.set_option("hub_threshold", hub_threshold)
        k = KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
        if k:
            self.set_option("kernel", k)

    def set_option(self, key: str, value: int):
        L.call("fu_set_option", self._h, key.encode(), int(value))

    def set_targets(self, target):
        self._target = np.ascontiguousarray(target, dtype=np.float64)
        L.call("fu_set_targets", self._h, L.ptr(self._target))

    def tune(self):
        """One autotune pass now (kernel "auto"), outside any timed region: ~55 real rounds
        at the current packing width; the state advances, so reset() before a timed run."""
        L.call("fu_tune", self._h)

    def run_marked(self, rounds_at):
        """Run rounds_at[-1] rounds in one call, recording mark k once rounds_at[k] of them
        are queued (rounds_at[0] = 0: the start). Asynchronous; see elapsed()."""
        ra = rounds_at if isinstance(rounds_at, np.ndarray) and rounds_at.dtype == np.int32 \
            and rounds_at.flags["C_CONTIGUOUS"] else np.ascontiguousarray(rounds_at, dtype=np.int32)
        L.call("fu_run_collectall_marked", self._h, len(ra), ra.ctypes.data)

    def mark(self, slot: int):
        """Record HIP event `slot` (0..63) on the engine's stream (asynchronous)."""
        L.call("fu_mark", self._h, int(slot))

    def elapsed(self, a: int, b: int) -> float:
        """Device milliseconds between marks a and b (waits for b)."""
        ms = L.f32()
        L.call("fu_mark_elapsed", self._h, int(a), int(b), ctypes.byref(ms))
        return float(ms.value)

    def info(self) -> dict:
        """Kernel in use (after autotuning), autotune state, rounds done."""
        return handle_info(self._h)

    def pack_widths(self) -> tuple:
        """Packed estimate table widths (0 = doubles): the last even / odd round's code
        table and the current encoding plan."""
        w = np.zeros(3, dtype=np.int32)
        L.call("fu_get_pack", self._h, L.ptr(w))
        return tuple(int(x) for x in w)


class CollectAllBatch(_Handle):
    """K value columns over one graph in one pass per round (fu_batch_*): each column is an
    independent run of `CollectAll`, bit for bit. `values` has shape (n, K), 1 <= K <= 16.

    >>> x = uniform_values(g.n, seed=0); one = np.zeros(g.n); one[0] = 1.0
    >>> eng = CollectAllBatch(g, np.stack([x, one], axis=1)); eng.run(1000)
    >>> avg, inv_n = eng.estimates()[0]; total = avg / inv_n    # AVG, COUNT = 1 / inv_n, SUM
    """

    _C = _c_names("fu_batch_")
    _NDIM = 2
    _ROWS = "values.shape[0]"
    _REV_LEN_CHECKED = False  # fu_batch_create proves symmetry with rev and never uploads it

    def __init__(self, graph: Graph | None = None, values=None, *, rowptr=None, col=None,
                 rev=None, device: int = 0):
        self._open(graph, values, rowptr, col, rev, device, extra=lambda v: (int(v.shape[1]),))
        self.K = self._cols = int(self.values.shape[1])

    def run(self, rounds: int, err_every: int = 0):
        """Run `rounds` rounds; with err_every > 0 returns the (rounds // err_every, K)
        max-error trace, one row per check and one entry per column."""
        return super().run(rounds, err_every)


def lossy_delivered(seed: int, round: int, first: int, count: int, p: float) -> np.ndarray:
    """uint8[count]: 1 where slot first + q is delivered in round `round` under (p, seed), the
    decision of `CollectAllLossy` restated on the host (fu_lossy_delivered; no GPU)."""
    out = np.empty(max(int(count), 1), dtype=np.uint8)
    L.call("fu_lossy_delivered", int(seed), int(round), int(first), int(count), float(p), L.ptr(out))
    return out[:int(count)]


class CollectAllLossy(_Handle):
    """Synchronous collect-all rounds under message loss (fu_lossy_*): in every round >= 1 each
    message is lost with probability `loss` (a pure function of seed, round and slot) or by a
    link mask; the receiver then fires on the flow and estimate it stored itself (CA:87-91,
    CA:117-119). loss = 0 with no mask is `CollectAll`, bit for bit.

    >>> eng = CollectAllLossy(g, uniform_values(g.n, seed=0), loss=0.1, seed=7)
    >>> eng.run(200); est = eng.estimates(); offered, lost = eng.stats
    """

    _C = _c_names("fu_lossy_")

    def __init__(self, graph: Graph | None = None, values=None, *, rowptr=None, col=None, rev=None,
                 loss: float = 0.0, seed: int = 0, device: int = 0):
        self._open(graph, values, rowptr, col, rev, device)
        if loss != 0.0 or seed != 0:
            self.set_loss(loss, seed)

    def set_loss(self, loss: float, seed: int = 0):
        """Loss probability in [0, 1] and seed of the rounds run from now on."""
        L.call("fu_lossy_set_loss", self._h, float(loss), int(seed))

    def set_link_mask(self, down):
        """down: E bytes, non-zero = slot lost in every round from now on; None clears."""
        if down is None:
            L.call("fu_lossy_set_link_mask", self._h, None)
            return
        d = np.ascontiguousarray(down, dtype=np.uint8)
        if d.shape != (self.E,):
            raise ValueError(f"mask must have shape ({self.E},), got {d.shape}")
        L.call("fu_lossy_set_link_mask", self._h, L.ptr(d) if self.E else None)

    def set_values(self, values):
        """New inputs; flows, estimates and the round counter are kept."""
        self._set_values(values)

    @property
    def stats(self) -> tuple:
        """(messages offered, messages lost) since the last reset; synchronises."""
        return self._stats()


def _columns(v):
    """The K of (n, K) values, in front of them in the *_create_k calls."""
    return (int(v.shape[1]),)


class CollectAllLossyBatch(CollectAllLossy):
    """K value columns under one loss pattern (fu_lossy_create_k): `values` has shape (n, K),
    1 <= K <= 16. One message carries all K (flow, estimate) pairs, so it is lost for every
    column at once and `stats` counts messages; column c is a `CollectAllLossy` run of column c
    with the same loss, seed and mask, bit for bit. estimates, targets and values are (n, K),
    flows (E, K), the error trace (checks, K), max_err (K,).

    >>> one = np.zeros(g.n); one[0] = 1.0
    >>> eng = CollectAllLossyBatch(g, np.stack([x, one], axis=1), loss=0.1, seed=7); eng.run(400)
    >>> avg, inv_n = eng.estimates()[5]; count, total = 1 / inv_n, avg / inv_n
    """

    _C = _c_names("fu_lossy_", create="fu_lossy_create_k", create_from_graph="fu_lossy_create_from_graph_k")
    _NDIM = 2
    _ROWS = "values.shape[0]"

    def __init__(self, graph: Graph | None = None, values=None, *, rowptr=None, col=None, rev=None,
                 loss: float = 0.0, seed: int = 0, device: int = 0):
        self._open(graph, values, rowptr, col, rev, device, extra=_columns)
        self.K = self._cols = int(self.values.shape[1])
        if loss != 0.0 or seed != 0:
            self.set_loss(loss, seed)


def _csr_of(g):
    """(rowptr, col, rev) of a Graph or of a (rowptr, col, rev) triple, rev None allowed."""
    rowptr, col, rev = g.arrays() if isinstance(g, Graph) else g
    return (np.ascontiguousarray(rowptr, dtype=np.int64), np.ascontiguousarray(col, dtype=np.int32),
            None if rev is None else np.ascontiguousarray(rev, dtype=np.int32))


def _mask(x, size: int, name: str):
    """A topology mask as uint8[size], or None; ValueError for another shape or a non-integer,
    non-boolean dtype."""
    if x is None:
        return None
    m = np.asarray(x)
    if m.dtype != np.bool_ and not np.issubdtype(m.dtype, np.integer):
        raise ValueError(f"{name} must be boolean or integer, got {m.dtype}")
    if m.shape != (size,):
        raise ValueError(f"{name} must have shape ({size},), got {m.shape}")
    return np.ascontiguousarray(m != 0, dtype=np.uint8)


def churn_live(g, alive=None, link_up=None) -> np.ndarray:
    """uint8[E]: 1 where slot k = (i -> j) is live under (alive, link_up): link_up[k] and alive[i]
    and alive[j]; None = all ones. g: a Graph or (rowptr, col, rev). The liveness rule of
    `CollectAllChurn` on the host (fu_churn_live; no GPU); FuError if link_up differs between a
    slot and its reverse."""
    rp, col, rev = _csr_of(g)
    n, E = len(rp) - 1, int(rp[-1])
    a, u = _mask(alive, n, "alive"), _mask(link_up, E, "link_up")
    out = np.empty(max(E, 1), dtype=np.uint8)
    z = lambda x: L.ptr(x) if x is not None and len(x) else None  # noqa: E731
    L.call("fu_churn_live", n, L.ptr(rp), z(col), z(rev), L.ptr(a), z(u), L.ptr(out))
    return out[:E]


def churn_targets(g, values, alive=None, link_up=None) -> np.ndarray:
    """What `CollectAllChurn` converges to under (alive, link_up): per alive node the exact mean
    of the alive inputs of its component of the live graph (`component_means` of the live
    subgraph, in the caller's numbering). A dead node's entry is its own value. values of shape
    (n, K) give (n, K): the components once, the means per column."""
    rp, col, _ = _csr_of(g)
    v = np.asarray(values, dtype=np.float64)
    if v.ndim not in (1, 2) or v.shape[0] != len(rp) - 1:
        raise ValueError(f"values must have shape (n,) or (n, K) with n = {len(rp) - 1}, got {v.shape}")
    live = churn_live(g, alive, link_up).astype(bool)
    src = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    lrp = np.concatenate([[0], np.cumsum(np.bincount(src[live], minlength=len(rp) - 1))]).astype(np.int64)
    nc, comp = components(lrp, col[live])
    if v.ndim == 1:
        return means_of_components(nc, comp, v)
    return np.stack([means_of_components(nc, comp, v[:, c]) for c in range(v.shape[1])], axis=1)


class CollectAllChurn(_Handle):
    """Synchronous collect-all rounds while nodes and links leave and join (fu_churn_*): between
    runs, `set_topology` switches nodes and links of the fixed graph off and on. A removed
    neighbour drops out of both sums and of the divisor and its flow entry is gone; an added one
    starts from zeros (CA:33-34, CA:94-96); a dead node keeps its last estimate. The alive nodes
    converge to the mean of the alive inputs of their component. With everything alive this is
    `CollectAll`, bit for bit. `CollectAllChurnBatch` runs K columns under one topology.

    >>> eng = CollectAllChurn(g, v); eng.run(100)
    >>> alive = np.ones(g.n, np.uint8); alive[:1000] = 0
    >>> eng.set_topology(alive=alive); eng.set_targets(churn_targets(g, v, alive)); eng.run(400)
    """

    _C = _c_names("fu_churn_", set_topology="fu_churn_set_topology", get_slot_state="fu_churn_get_slot_state")
    UP, DOWN, FRESH = 0, 1, 2

    def __init__(self, graph: Graph | None = None, values=None, *, rowptr=None, col=None, rev=None, device: int = 0):
        self._open(graph, values, rowptr, col, rev, device)

    def set_topology(self, alive=None, link_up=None):
        """alive: n entries, link_up: E entries (the same on a slot and its reverse), non-zero =
        on, None = all on. The whole topology of the rounds run from now on."""
        a, u = _mask(alive, self.n, "alive"), _mask(link_up, self.E, "link_up")
        self._call("set_topology", L.ptr(a), L.ptr(u) if self.E else None)

    def set_values(self, values):
        """New inputs; flows, estimates, slot states and the round counter are kept."""
        self._set_values(values)

    @property
    def stats(self) -> tuple:
        """(alive nodes, live directed slots) of the current topology."""
        return self._stats()

    def slot_state(self) -> np.ndarray:
        """uint8[E]: UP (0), DOWN (1) or FRESH (2) per slot."""
        s = np.empty(max(self.E, 1), dtype=np.uint8)
        self._call("get_slot_state", L.ptr(s))
        return s[:self.E]


class CollectAllChurnBatch(CollectAllChurn):
    """K value columns under one topology (fu_churn_create_k): `values` has shape (n, K),
    1 <= K <= 16. Topology, slot states and `stats` are per node and per slot as for one column;
    column c is a `CollectAllChurn` run of column c under the same events, bit for bit.
    estimates, targets and values are (n, K), flows (E, K), the error trace (checks, K),
    max_err (K,), per column over the alive nodes.

    >>> one = np.zeros(g.n); one[0] = 1.0; v = np.stack([x, one], axis=1)
    >>> eng = CollectAllChurnBatch(g, v); eng.run(100)
    >>> eng.set_topology(alive=alive); eng.set_targets(churn_targets(g, v, alive)); eng.run(400)
    >>> avg, inv_n = eng.estimates()[0]; alive_count, alive_sum = 1 / inv_n, avg / inv_n
    """

    _C = _c_names("fu_churn_", set_topology="fu_churn_set_topology", get_slot_state="fu_churn_get_slot_state",
                  create="fu_churn_create_k", create_from_graph="fu_churn_create_from_graph_k")
    _NDIM = 2
    _ROWS = "values.shape[0]"

    def __init__(self, graph: Graph | None = None, values=None, *, rowptr=None, col=None, rev=None, device: int = 0):
        self._open(graph, values, rowptr, col, rev, device, extra=_columns)
        self.K = self._cols = int(self.values.shape[1])


def pair_matching(g, seed: int, r: int, alive=None, link_up=None):
    """(mate, initiator) of round r under `seed` on graph g (a Graph, or a (rowptr, col) pair):
    mate[i] is i's partner or -1, initiator[i] is 1 for the proposer of a pair. The matching of
    `PairwiseSync` restated on the host (fu_pair_matching; no GPU). With `alive` (n entries) or
    `link_up` (E entries) it is the matching under that topology, the rule on the live subgraph
    (fu_pair_matching_live); both None is the matching without a topology."""
    rowptr, col = (g.rowptr, g.col) if isinstance(g, Graph) else g
    rp = np.ascontiguousarray(rowptr, dtype=np.int64)
    c = np.ascontiguousarray(col, dtype=np.int32)
    n = len(rp) - 1
    a, u = _mask(alive, n, "alive"), _mask(link_up, len(c), "link_up")
    mate = np.empty(max(n, 1), dtype=np.int32)
    init = np.empty(max(n, 1), dtype=np.uint8)
    cp = L.ptr(c) if len(c) else None
    if a is None and u is None:
        L.call("fu_pair_matching", n, L.ptr(rp), cp, int(seed), int(r), L.ptr(mate), L.ptr(init))
    else:
        L.call("fu_pair_matching_live", n, L.ptr(rp), cp, L.ptr(a), L.ptr(u) if len(c) else None, int(seed), int(r),
               L.ptr(mate), L.ptr(init))
    return mate[:n], init[:n]


def pair_lost(seed: int, round: int, first: int, count: int, p: float) -> np.ndarray:
    """uint8[count]: 1 where the message received on slot first + q in round `round` is lost
    under (p, seed) and no mask, the decision of `PairwiseSync` restated on the host
    (fu_pair_lost; no GPU)."""
    out = np.empty(max(int(count), 1), dtype=np.uint8)
    L.call("fu_pair_lost", int(seed), int(round), int(first), int(count), float(p), L.ptr(out))
    return out[:int(count)]


class PairwiseSync(_Handle):
    """Synchronous pairwise rounds (fu_pair_*): every round a matching of the graph is chosen on
    the device (a pure function of seed, round and graph) and each matched pair runs one full
    pairwise exchange: the initiator fires (PW:102-117), the listener receives and fires back,
    the initiator receives and stops there. Gossip averaging over the matching; no host-built
    schedule, so million-node graphs and thousands of rounds are one run() call.

    >>> eng = PairwiseSync(g, uniform_values(g.n, seed=0), seed=7)
    >>> eng.run(1000); est = eng.estimates(); pairs, never_fired = eng.stats

    With `loss` > 0 or a `link_mask`, each of a pair's two messages can be lost, decided by the
    slot that would receive it (a pure function of loss_seed, round and slot; `pair_lost` restates
    it). A lost first message leaves the initiator's fire standing and the listener untouched; a
    lost answer leaves both fires standing; the next message delivered over the link heals it.

    >>> eng = PairwiseSync(g, uniform_values(g.n, seed=0), seed=7, loss=0.1, loss_seed=3)
    >>> eng.run(2000); first_lost, answers_lost, complete = eng.loss_stats

    `set_topology` switches nodes and links off and on between runs, as `CollectAllChurn` does:
    the alive nodes converge to `churn_targets`, and the error runs over the alive nodes.

    >>> eng.run(500); alive = np.ones(g.n, np.uint8); alive[:1000] = 0
    >>> eng.set_topology(alive=alive); eng.set_targets(churn_targets(g, v, alive)); eng.run(2000)
    """

    _C = _c_names("fu_pair_")

    def __init__(self, graph: Graph | None = None, values=None, *, rowptr=None, col=None, rev=None,
                 seed: int = 0, loss: float = 0.0, loss_seed: int = 0, link_mask=None, device: int = 0):
        self._open(graph, values, rowptr, col, rev, device)
        self._configure(seed, loss, loss_seed, link_mask)

    def _configure(self, seed, loss, loss_seed, link_mask):
        if seed != 0:
            self.set_seed(seed)
        try:
            if loss != 0.0 or loss_seed != 0:
                self.set_loss(loss, loss_seed)
            if link_mask is not None:
                self.set_link_mask(link_mask)
        except Exception:
            self.close()  # a bad loss or mask: the handle just opened does not wait for the collector
            raise

    def set_seed(self, seed: int):
        """Seed of the matchings of the rounds run from now on."""
        L.call("fu_pair_set_seed", self._h, int(seed))

    def set_loss(self, p: float, seed: int = 0):
        """Loss probability in [0, 1] and loss seed of the rounds run from now on."""
        L.call("fu_pair_set_loss", self._h, float(p), int(seed))

    def set_link_mask(self, down):
        """down: E entries, non-zero = every message received on that slot is lost in the rounds
        run from now on; None clears the mask."""
        d = _mask(down, self.E, "link_mask")
        L.call("fu_pair_set_link_mask", self._h, L.ptr(d) if d is not None and self.E else None)

    def set_topology(self, alive=None, link_up=None):
        """alive: n entries, link_up: E entries (the same on a slot and its reverse), non-zero =
        on, None = all on: the whole topology of the rounds run from now on, `CollectAllChurn`'s.
        A slot that stops being live loses its flow and cache on both ends; one that becomes live
        starts from the zeros it holds; the matching runs on the live subgraph."""
        a, u = _mask(alive, self.n, "alive"), _mask(link_up, self.E, "link_up")
        L.call("fu_pair_set_topology", self._h, L.ptr(a), L.ptr(u) if self.E else None)

    @property
    def topology_stats(self) -> tuple:
        """(alive nodes, live directed slots) of the current topology; (n, E) before any."""
        s = np.zeros(2, dtype=np.int64)
        L.call("fu_pair_get_topology_stats", self._h, L.ptr(s))
        return int(s[0]), int(s[1])

    def slot_live(self) -> np.ndarray:
        """uint8[E]: 1 where the slot is live."""
        s = np.empty(max(self.E, 1), dtype=np.uint8)
        L.call("fu_pair_get_slot_live", self._h, L.ptr(s))
        return s[:self.E]

    def set_option(self, key: str, value: int):
        """"match": 0 = proposers push (atomicMin, default), 1 = listeners scan their rows."""
        L.call("fu_pair_set_option", self._h, key.encode(), int(value))

    def set_values(self, values):
        """New inputs; flows, caches, last averages and the round counter are kept."""
        self._set_values(values)

    def estimates(self) -> np.ndarray:
        """Every node's average at its last fire (0.0 before its first)."""
        return super().estimates()

    def cache(self) -> np.ndarray:
        """The cached estimate of every slot."""
        c = np.empty(self._shape(max(self.E, 1)))
        L.call("fu_pair_get_cache", self._h, L.ptr(c))
        return c[:self.E]

    @property
    def stats(self) -> tuple:
        """(pairs matched, nodes that have never fired) since the last reset; synchronises."""
        return self._stats()

    @property
    def loss_stats(self) -> tuple:
        """(first messages lost, answers lost, complete exchanges) since the last reset: the
        three outcomes of the matched pairs; synchronises."""
        s = np.zeros(3, dtype=np.int64)
        L.call("fu_pair_get_loss_stats", self._h, L.ptr(s))
        return int(s[0]), int(s[1]), int(s[2])


class PairwiseSyncBatch(PairwiseSync):
    """K value columns over one matching (fu_pair_create_k): `values` has shape (n, K),
    1 <= K <= 16. One message carries all K (flow, estimate) pairs, so the matching of a round,
    the loss outcomes of a pair, the link mask, `stats` and `loss_stats` are those of one
    `PairwiseSync` with the same seeds; column c is a `PairwiseSync` run of column c, bit for bit.
    estimates, targets and values are (n, K), flows and cache (E, K), the error trace
    (checks, K), max_err (K,).

    >>> one = np.zeros(g.n); one[0] = 1.0
    >>> eng = PairwiseSyncBatch(g, np.stack([x, one], axis=1), seed=7); eng.run(2000)
    >>> avg, inv_n = eng.estimates()[5]; count, total = 1 / inv_n, avg / inv_n
    """

    _C = _c_names("fu_pair_", create="fu_pair_create_k", create_from_graph="fu_pair_create_from_graph_k")
    _NDIM = 2
    _ROWS = "values.shape[0]"

    def __init__(self, graph: Graph | None = None, values=None, *, rowptr=None, col=None, rev=None,
                 seed: int = 0, loss: float = 0.0, loss_seed: int = 0, link_mask=None, device: int = 0):
        self._open(graph, values, rowptr, col, rev, device, extra=_columns)
        self.K = self._cols = int(self.values.shape[1])
        self._configure(seed, loss, loss_seed, link_mask)


class Trace:
    """Tick-level schedule of the reference run (fu_trace_build), value-independent.

    decl_rowptr/decl_col: declared neighbour lists (actors.xml, ACT:4-27) in deployment
    order. mode: 'collectall' | 'pairwise'. order: 'fwd' | 'rev' | 'rand:<seed>'.
    """

    def __init__(self, decl_rowptr, decl_col, mode: str, ticks: int, order: str = "fwd",
                 faults: str | None = None, route_s=None, net=None):
        """route_s: optional n x n transfer times in seconds (sender row); a message matched at
        tick t is consumed from tick t + floor(T) + 1 (fu_trace_build_routes).
        net: optional link model (fu.platform.Platform.link_net): transfers share the
        links' bandwidth (max-min fair, weighted by LV08's sharing penalty when net holds
        weight_S > 0, capped by the TCP window with tcp_gamma > 0, each transfer loading its
        reverse route with crosstraffic > 0: fu_trace_build_links_cross); exclusive with
        route_s."""
        rp = np.ascontiguousarray(decl_rowptr, dtype=np.int64)
        c = np.ascontiguousarray(decl_col, dtype=np.int32)
        self.n = len(rp) - 1
        self.decl_deg = np.diff(rp)
        self.mode = mode
        self.ticks = int(ticks)
        self.order = order
        out = L.vp()
        self._route = None
        if route_s is not None:
            self._route = np.ascontiguousarray(route_s, dtype=np.float64)
            if self._route.shape != (self.n, self.n):
                raise ValueError("route_s must be n x n")
        if net is not None:
            if route_s is not None:
                raise ValueError("route_s and net are exclusive")
            self._net = {k: np.ascontiguousarray(net[k], dtype=dt) for k, dt in (
                ("bw", np.float64), ("lat", np.float64), ("shared", np.int32),
                ("route_off", np.int64), ("route_links", np.int32))}
            if len(self._net["route_off"]) != self.n * self.n + 1:
                raise ValueError("net['route_off'] must have n * n + 1 entries")
            nl = len(self._net["bw"])
            z = lambda a: L.ptr(a) if len(a) else None  # noqa: E731
            L.call("fu_trace_build_links_cross", self.n, L.ptr(rp), L.ptr(c) if len(c) else None, MODE[mode],
                   self.ticks, order.encode(), faults.encode() if faults else None, nl, z(self._net["bw"]),
                   z(self._net["lat"]), z(self._net["shared"]), L.ptr(self._net["route_off"]),
                   z(self._net["route_links"]), float(net.get("bytes", 154.0)),
                   float(net.get("lat_factor", 13.01)), float(net.get("bw_factor", 0.97)),
                   float(net.get("weight_S", 0.0)), float(net.get("tcp_gamma", 0.0)),
                   float(net.get("crosstraffic", 0.0)), ctypes.byref(out))
        else:
            L.call("fu_trace_build_routes", self.n, L.ptr(rp), L.ptr(c) if len(c) else None, MODE[mode],
                   self.ticks, order.encode(), faults.encode() if faults else None,
                   None if self._route is None else L.ptr(self._route), ctypes.byref(out))
        self._h = out
        self.faults = faults
        dr, dl = L.i64(), L.i64()
        L.call("fu_trace_fault_stats", self._h, ctypes.byref(dr), ctypes.byref(dl))
        self.dropped, self.delayed = int(dr.value), int(dl.value)
        info = np.zeros(8, dtype=np.int64)
        L.call("fu_trace_info", self._h, L.ptr(info))
        (self.n_union_edges, self.n_tasks, self.n_events, self.n_out_ids, self.n_msgs,
         _, self.dynamic_additions, self.messages_sent) = (int(x) for x in info)
        self._arrays = None

    def arrays(self) -> dict:
        if self._arrays is None:
            a = {
                "rowptr": np.empty(self.n + 1, dtype=np.int64),
                "col": np.empty(max(self.n_union_edges, 1), dtype=np.int32),
                "tick_task_off": np.empty(self.ticks + 1, dtype=np.int64),
                "tasks": np.empty((max(self.n_tasks, 1), 3), dtype=np.int32),
                "events": np.empty((max(self.n_events, 1), 4), dtype=np.int32),
                "out_ids": np.empty(max(self.n_out_ids, 1), dtype=np.int32),
                "first_avg_seq": np.empty(self.n, dtype=np.int64),
                "fires": np.empty(self.n, dtype=np.int32),
            }
            L.call("fu_trace_export", self._h, *(L.ptr(a[k]) for k in (
                "rowptr", "col", "tick_task_off", "tasks", "events", "out_ids",
                "first_avg_seq", "fires")))
            a["col"] = a["col"][:self.n_union_edges]
            a["tasks"] = a["tasks"][:self.n_tasks]
            a["events"] = a["events"][:self.n_events]
            a["out_ids"] = a["out_ids"][:self.n_out_ids]
            self._arrays = a
        return self._arrays

    def last_avg_order(self) -> list[int]:
        """Nodes in the key order of global_values['last_avg'] (order of first average)."""
        seq = self.arrays()["first_avg_seq"]
        nodes = [i for i in range(self.n) if seq[i] >= 0]
        return sorted(nodes, key=lambda i: seq[i])

    def free(self):
        if getattr(self, "_h", None):
            L.lib.fu_trace_free(self._h)
            self._h = None

    def __del__(self):
        self.free()


class Replay:
    """GPU replay of a Trace with node values."""

    def __init__(self, trace: Trace, values, device: int = 0, persistent: bool = False,
                 registers: bool = True):
        self.trace = trace
        self.values = np.ascontiguousarray(values, dtype=np.float64)
        if len(self.values) != trace.n:
            raise ValueError("len(values) != trace.n")
        out = L.vp()
        L.call("fu_replay_create_from_trace", trace._h, L.ptr(self.values), int(device),
               ctypes.byref(out))
        self._h = out
        self.n = trace.n
        self.E = trace.n_union_edges
        if persistent:
            L.call("fu_replay_set_option", self._h, b"persistent", 1)
            L.call("fu_replay_set_option", self._h, b"persistent_reg", int(registers))
        self.tick = 0

    def run(self, tick_end: int, snapshot_ticks=()):
        """Run ticks [current, tick_end); returns {tick: last_avg copy} for snapshot_ticks."""
        st = np.ascontiguousarray(sorted(snapshot_ticks), dtype=np.int32)
        snaps = np.empty((max(len(st), 1), self.n))
        L.call("fu_replay_run", self._h, int(tick_end), len(st),
               L.ptr(st) if len(st) else None, L.ptr(snaps) if len(st) else None)
        self.tick = int(tick_end)
        return {int(t): snaps[k].copy() for k, t in enumerate(st)}

    def run_timed(self, tick_end: int) -> float:
        ms = L.f32()
        L.call("fu_replay_run_timed", self._h, int(tick_end), ctypes.byref(ms))
        self.tick = int(tick_end)
        return float(ms.value)

    def state(self):
        last = np.empty(self.n)
        fl = np.empty(max(self.E, 1))
        es = np.empty(max(self.E, 1))
        L.call("fu_replay_get", self._h, L.ptr(last), L.ptr(fl), L.ptr(es))
        return last, fl[:self.E], es[:self.E]

    def set_option(self, key: str, value: int):
        L.call("fu_replay_set_option", self._h, key.encode(), int(value))

    def info(self) -> list[int]:
        """fu_replay_get_info: [persistent, register kernel used, its row registers (8 / 16 /
        0), collect-all fires in the trace, blocks of the generic persistent launch, unique
        message slots, max union degree, current tick]."""
        info = np.zeros(8, dtype=np.int64)
        L.call("fu_replay_get_info", self._h, L.ptr(info))
        return [int(x) for x in info]

    def close(self):
        if getattr(self, "_h", None):
            L.lib.fu_replay_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()
