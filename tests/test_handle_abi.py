"""The handle scaffold the batched, lossy, pairwise and churn engines share (fu_batch_*,
fu_lossy_*, fu_pair_*, fu_churn_*), without a GPU: every argument and graph check runs before the
first HIP call, so each bad input below returns its code and leaves its text in fu_last_error()
on any host. One table, looped over the four engines; the texts are the library's, written out in
full, the function-name prefix included.

The engines differ in one check on purpose: fu_batch_create only asks that rev[k] lie in the
neighbour's row at a slot that points back (its kernels never read rev), while fu_lossy_create,
fu_pair_create and fu_churn_create also ask for an involution (theirs gather through it).
test_batch_keeps_its_symmetric_only_rev_check pins that difference on a doubled edge."""
import ctypes
import math

import numpy as np
import pytest

import fu
from fu import _lib as L

ENGINES = ("batch", "lossy", "pair", "churn")
ARG, HIP, GRAPH = -1, -2, -5
NULL = object()  # "pass a null pointer here"

# a path of 3: 0 - 1 - 2
PATH_RP = np.array([0, 1, 3, 4], dtype=np.int64)
PATH_COL = np.array([1, 0, 2, 1], dtype=np.int32)
PATH_REV = np.array([1, 0, 3, 2], dtype=np.int32)
# two nodes joined by a doubled edge; both of node 0's slots name slot 2 of node 1
DOUBLED_RP = np.array([0, 2, 4], dtype=np.int64)
DOUBLED_COL = np.array([1, 1, 0, 0], dtype=np.int32)
DOUBLED_REV = np.array([2, 2, 0, 1], dtype=np.int32)
# two nodes, each with a loop and the edge to the other; rev pairs each loop with itself
LOOPS_RP = np.array([0, 2, 4], dtype=np.int64)
LOOPS_COL = np.array([0, 1, 0, 1], dtype=np.int32)
LOOPS_REV = np.array([0, 2, 1, 3], dtype=np.int32)


def _p(a):
    return None if a is NULL or a is None else L.ptr(a)


def _create(eng, rp, col, rev, *, n=None, e=None, value=None, k=2, out=True):
    """(code, text) of fu_<eng>_create; a handle that does get made (a host with a GPU) is
    destroyed at once."""
    n = len(rp) - 1 if n is None else n
    e = int(rp[-1]) if e is None else e
    if value is None:
        value = np.ones((max(n, 1), max(k, 1))) if eng == "batch" else np.ones(max(n, 1))
    h = L.vp()
    args = [n, e, _p(rp), _p(col), _p(rev)] + ([k] if eng == "batch" else []) + \
        [_p(value), 0, ctypes.byref(h) if out else None]
    rc = getattr(L.lib, f"fu_{eng}_create")(*args)
    text = L.last_error()
    if rc == 0:
        getattr(L.lib, f"fu_{eng}_destroy")(h)
    return rc, text


def _from_graph(eng, g, *, value=True, k=2, out=True):
    n = 2
    v = (np.ones((n, max(k, 1))) if eng == "batch" else np.ones(n)) if value else None
    h = L.vp()
    args = [g] + ([k] if eng == "batch" else []) + [_p(v), 0, ctypes.byref(h) if out else None]
    rc = getattr(L.lib, f"fu_{eng}_create_from_graph")(*args)
    text = L.last_error()
    if rc == 0:
        getattr(L.lib, f"fu_{eng}_destroy")(h)
    return rc, text


def _past_validation(eng, got):
    """Every check passed: without a GPU the next thing is the device probe's error."""
    if fu.device_count() == 0:
        assert got == (HIP, f"fu_{eng}_create: no HIP device visible"), (eng, got)
    else:
        assert got[0] == 0, (eng, got)


def _arr(x, dt):
    return np.array(x, dtype=dt)


# (what, kwargs of _create, tail of the text after "fu_<eng>_create: ", code)
_BAD = "bad arguments"
_ROWPTR = "rowptr[0] must be 0 and rowptr[n] == e"
_REV = "rev is not the reverse-edge pairing (the graph must be symmetric) at edge "
CREATE_ROWS = [
    ("null out", dict(rp=PATH_RP, col=PATH_COL, rev=None, out=False), _BAD, ARG),
    ("null rowptr", dict(rp=NULL, col=PATH_COL, rev=None, n=3, e=4), _BAD, ARG),
    ("null value", dict(rp=PATH_RP, col=PATH_COL, rev=None, value=NULL), _BAD, ARG),
    ("n == 0", dict(rp=PATH_RP, col=PATH_COL, rev=None, n=0), _BAD, ARG),
    ("n < 0", dict(rp=PATH_RP, col=PATH_COL, rev=None, n=-3), _BAD, ARG),
    ("e < 0", dict(rp=PATH_RP, col=PATH_COL, rev=None, e=-1), _BAD, ARG),
    ("e > 0, null col", dict(rp=PATH_RP, col=NULL, rev=None), _BAD, ARG),
    ("rowptr[0] != 0", dict(rp=_arr([1, 1, 3, 4], np.int64), col=PATH_COL, rev=None), _ROWPTR, ARG),
    ("rowptr[n] != e", dict(rp=PATH_RP, col=PATH_COL, rev=None, e=3), _ROWPTR, ARG),
    ("rowptr not monotone", dict(rp=_arr([0, 3, 1, 4], np.int64), col=PATH_COL, rev=None), "rowptr not monotone", ARG),
    ("col too large", dict(rp=PATH_RP, col=_arr([1, 3, 2, 1], np.int32), rev=None), "col index out of range at edge 1", ARG),
    ("col negative", dict(rp=PATH_RP, col=_arr([1, 0, 2, -1], np.int32), rev=None), "col index out of range at edge 3", ARG),
    ("rev too large", dict(rp=PATH_RP, col=PATH_COL, rev=_arr([1, 0, 4, 2], np.int32)), _REV + "2", GRAPH),
    ("rev negative", dict(rp=PATH_RP, col=PATH_COL, rev=_arr([-1, 0, 3, 2], np.int32)), _REV + "0", GRAPH),
    ("rev into the wrong row", dict(rp=PATH_RP, col=PATH_COL, rev=_arr([3, 2, 1, 0], np.int32)), _REV + "0", GRAPH),
    # a row that holds its own id: fu_graph_from_csr's rule, for raw arrays too
    ("self-loop", dict(rp=PATH_RP, col=_arr([1, 1, 2, 1], np.int32), rev=None), "self-loop at node 1", GRAPH),
    ("self-loop, with a rev", dict(rp=PATH_RP, col=_arr([1, 1, 2, 1], np.int32), rev=PATH_REV), "self-loop at node 1", GRAPH),
    # both loops paired with themselves, an involution: every rev check would pass
    ("self-loops, rev[k] == k", dict(rp=LOOPS_RP, col=LOOPS_COL, rev=LOOPS_REV), "self-loop at node 0", GRAPH),
    ("self-loop on the last row", dict(rp=_arr([0, 1, 4], np.int64), col=_arr([1, 0, 1, 1], np.int32), rev=None),
     "self-loop at node 1", GRAPH),
]


@pytest.mark.parametrize("eng", ENGINES)
def test_create_argument_and_graph_errors(eng):
    for what, kw, tail, code in CREATE_ROWS:
        assert _create(eng, **kw) == (code, f"fu_{eng}_create: {tail}"), (eng, what)
    # an asymmetric graph without a rev: the rev builder's own text, which names no caller
    got = _create(eng, _arr([0, 1, 1], np.int64), _arr([1], np.int32), None)
    assert got == (GRAPH, "graph is not symmetric (edge 0 has no reverse edge)"), eng


@pytest.mark.parametrize("eng", ENGINES)
def test_more_edges_than_an_int32_rev_holds(eng):
    """Only the scalar e is large: the check comes before any array is read. The batched engine
    keeps no rev on the device and has no such limit; there the same call fails on rowptr[n]."""
    got = _create(eng, PATH_RP, PATH_COL, None, e=2 ** 31)
    tail = _ROWPTR if eng == "batch" else "more than 2^31-1 directed edges (rev is int32)"
    assert got == (ARG, f"fu_{eng}_create: {tail}")
    if eng != "batch":  # 2^31 - 1 itself passes that check and fails the next
        assert _create(eng, PATH_RP, PATH_COL, None, e=2 ** 31 - 1) == (ARG, f"fu_{eng}_create: {_ROWPTR}")


@pytest.mark.parametrize("eng", ("lossy", "churn"))
def test_self_loop_through_the_k_column_creates(eng):
    """fu_lossy_create_k and fu_churn_create_k share the front half of the one-column creates."""
    v = np.ones((2, 3))
    h = L.vp()
    rc = getattr(L.lib, f"fu_{eng}_create_k")(2, 4, _p(LOOPS_RP), _p(LOOPS_COL), _p(LOOPS_REV), 3, _p(v), 0, ctypes.byref(h))
    assert (rc, L.last_error()) == (GRAPH, f"fu_{eng}_create_k: self-loop at node 0")


def test_churn_live_refuses_a_self_loop():
    out, alive = np.zeros(4, dtype=np.uint8), np.ones(2, dtype=np.uint8)
    for rev in (LOOPS_REV, None):
        rc = L.lib.fu_churn_live(2, _p(LOOPS_RP), _p(LOOPS_COL), _p(rev), _p(alive), None, _p(out))
        assert (rc, L.last_error()) == (GRAPH, "fu_churn_live: self-loop at node 0")
    assert not out.any()  # nothing written


@pytest.mark.parametrize("k", [0, 17, -1])
def test_batch_column_count(k):
    v = np.ones((3, 1))
    assert _create("batch", PATH_RP, PATH_COL, None, k=k, value=v) == \
        (ARG, f"fu_batch_create: k must be in 1..16, got {k}")
    g = fu.Graph.from_csr(PATH_RP, PATH_COL)
    assert _from_graph("batch", g._h, k=k) == (ARG, f"fu_batch_create_from_graph: k must be in 1..16, got {k}")
    # the null checks come first, the CSR checks after
    assert _create("batch", PATH_RP, PATH_COL, None, k=k, value=NULL) == (ARG, "fu_batch_create: bad arguments")
    assert _create("batch", PATH_RP, PATH_COL, None, k=k, value=v, e=3)[1] == f"fu_batch_create: k must be in 1..16, got {k}"


@pytest.mark.parametrize("eng", ENGINES)
def test_create_from_graph_errors(eng):
    name = f"fu_{eng}_create_from_graph"
    sym = fu.Graph.from_csr(_arr([0, 1, 2], np.int64), _arr([1, 0], np.int32))
    asym = fu.Graph.from_csr(_arr([0, 1, 1], np.int64), _arr([1], np.int32), require_symmetric=False)
    assert _from_graph(eng, None) == (ARG, name + ": bad arguments")
    assert _from_graph(eng, sym._h, value=False) == (ARG, name + ": bad arguments")
    assert _from_graph(eng, sym._h, out=False) == (ARG, name + ": bad arguments")
    assert _from_graph(eng, asym._h) == (GRAPH, name + ": graph is not symmetric")
    _past_validation(eng, _from_graph(eng, sym._h))


@pytest.mark.parametrize("eng", ENGINES)
def test_good_inputs_reach_the_device_probe(eng):
    """A path of 3 with and without the caller's rev, and three nodes without an edge (with and
    without a col array)."""
    _past_validation(eng, _create(eng, PATH_RP, PATH_COL, None))
    _past_validation(eng, _create(eng, PATH_RP, PATH_COL, PATH_REV))
    zero = np.zeros(4, dtype=np.int64)
    _past_validation(eng, _create(eng, zero, NULL, None))
    _past_validation(eng, _create(eng, zero, np.zeros(1, dtype=np.int32), None))


def test_batch_keeps_its_symmetric_only_rev_check():
    """The doubled edge 0 = 1 with rev = [2, 2, 0, 1]: every rev[k] lies in the neighbour's row
    at a slot that points back, which is all fu_batch_create asks; rev[rev[1]] = 0 != 1, so it
    is no involution, and the engines that gather through rev refuse it at edge 1."""
    _past_validation("batch", _create("batch", DOUBLED_RP, DOUBLED_COL, DOUBLED_REV))
    for eng in ("lossy", "pair", "churn"):
        assert _create(eng, DOUBLED_RP, DOUBLED_COL, DOUBLED_REV) == (GRAPH, f"fu_{eng}_create: {_REV}1"), eng
        # the pairing the library builds itself goes through the same check: it looks a
        # neighbour up by id, so on a doubled edge it is no involution either
        assert _create(eng, DOUBLED_RP, DOUBLED_COL, None) == (GRAPH, f"fu_{eng}_create: {_REV}1"), eng
    _past_validation("batch", _create("batch", DOUBLED_RP, DOUBLED_COL, None))


# entry point -> arguments after the null handle
SHARED = {"destroy": (), "reset": (), "set_targets": (None,), "run": (1, 0, None), "run_timed": (1, None),
          "max_err": (None,), "get_estimates": (None,), "get_flows": (None,), "get_round": (None,), "synchronize": ()}
OWN = {"batch": {},
       "lossy": {"set_values": (None,), "get_stats": (None,), "set_loss": (0.5, 1), "set_link_mask": (None,)},
       "pair": {"set_values": (None,), "get_stats": (None,), "set_seed": (1,), "set_option": (b"match", 1),
                "get_cache": (None,)},
       "churn": {"set_values": (None,), "get_stats": (None,), "set_topology": (None, None), "get_slot_state": (None,)}}


@pytest.mark.parametrize("eng", ENGINES)
def test_null_handle_calls(eng):
    for name, args in {**SHARED, **OWN[eng]}.items():
        fn = f"fu_{eng}_{name}"
        assert getattr(L.lib, fn)(None, *args) == ARG, fn
        assert L.last_error() == fn + ": bad arguments", fn
    # the handle is looked at first: a bad p or a negative round count on a null handle is the
    # same error (fu_lossy_set_loss's range check needs a live handle)
    if eng == "lossy":
        assert L.lib.fu_lossy_set_loss(None, 1.5, 0) == ARG
        assert L.last_error() == "fu_lossy_set_loss: bad arguments"
    assert getattr(L.lib, f"fu_{eng}_run")(None, -1, 0, None) == ARG
    assert L.last_error() == f"fu_{eng}_run: bad arguments"


def test_lossy_delivered_bad_arguments():
    out = np.zeros(4, dtype=np.uint8)
    for seed, rnd, first, count, p, o in ((1, -1, 0, 4, 0.5, out), (1, 0, -1, 4, 0.5, out), (1, 0, 0, -1, 0.5, out),
                                          (1, 1, 0, 4, 0.5, None), (1, 1, 0, 4, -0.1, out), (1, 1, 0, 4, 1.5, out),
                                          (1, 1, 0, 4, math.nan, out)):
        assert L.lib.fu_lossy_delivered(seed, rnd, first, count, p, _p(o)) == ARG, (rnd, first, count, p)
        assert L.last_error() == "fu_lossy_delivered: bad arguments"
    assert L.lib.fu_lossy_delivered(1, 1, 0, 0, 1.0, None) == 0  # nothing asked for, nothing written


def test_pair_matching_bad_arguments():
    mate, ini = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.uint8)

    def call(n=3, rp=PATH_RP, col=PATH_COL, rnd=0, m=mate, i=ini):
        return L.lib.fu_pair_matching(n, _p(rp), _p(col), 1, rnd, _p(m), _p(i)), L.last_error()

    bad = (ARG, "fu_pair_matching: bad arguments")
    assert call(n=0) == bad
    assert call(rp=None) == bad
    assert call(rnd=-1) == bad
    assert call(m=None) == bad
    assert call(i=None) == bad
    assert call(rp=_arr([1, 1, 3, 4], np.int64)) == bad
    assert call(col=None) == bad
    assert call(rp=_arr([0, 3, 1, 4], np.int64)) == (ARG, "fu_pair_matching: rowptr not monotone")
    assert call(col=_arr([3, 0, 2, 1], np.int32)) == (ARG, "fu_pair_matching: col index out of range at edge 0")
    assert call(col=_arr([1, 0, 2, 2], np.int32)) == (GRAPH, "fu_pair_matching: self-loop at node 2")
    assert call(n=2, rp=LOOPS_RP, col=LOOPS_COL) == (GRAPH, "fu_pair_matching: self-loop at node 0")
    assert call()[0] == 0
