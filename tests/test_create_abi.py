"""The collect-all create entry points (fu_create, fu_create_from_graph(_ex), fu_dist_create,
fu_dist_create_local) on bad arguments: every argument and CSR check runs on the host before
anything walks an array and before the first HIP call, so each row below returns its code and
leaves its text in fu_last_error() on any host, the same with and without a GPU. One table per
entry point, the library's texts written out in full. tools/create_check.cpp feeds the same rows
to the same checks under AddressSanitizer, each array a heap block of its exact length.

A bad local CSR given to fu_dist_create(_local) is reported under "fu_create: ...", as the
shared constructor always has; only the self-loop text, which is new, names fu_dist_create.

The GPU tests at the end walk the whole failing table first, then make and run good handles on
the same thread: a failed create leaves nothing on the device and nothing in fu_last_error()
that a later call could trip over. Every bad row is refused on the host: none reaches a kernel."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import coracle
import fu
from conftest import ROOT, ca_sync_fixtures, load_npz
from fu import _lib as L
from fu.dist import DistCollectAll, partition, run_local
from parity_util import assert_same_bits

ARG, HIP, GRAPH = -1, -2, -5
NULL = object()  # "pass a null pointer here"
NO_DEVICE = (HIP, "fu_create: no HIP device visible")


def _arr(x, dt):
    return np.array(x, dtype=dt)


def _i64(*x):
    return _arr(x, np.int64)


def _i32(*x):
    return _arr(x, np.int32)


def _p(a):
    return None if a is NULL or a is None else L.ptr(a)


# a path of 3: 0 - 1 - 2
PATH_RP, PATH_COL, PATH_REV = _i64(0, 1, 3, 4), _i32(1, 0, 2, 1), _i32(1, 0, 3, 2)
# a triangle, for a rev that lands in the right row at a slot that names another node
TRI_RP, TRI_COL = _i64(0, 2, 4, 6), _i32(1, 2, 0, 2, 0, 1)
# two nodes, four slots: the arrays behind the [0, 100, 4]-style row pointers
TWO_COL, TWO_REV = _i32(1, 1, 0, 0), _i32(2, 3, 0, 1)


def _finish(rc, h):
    text = L.last_error()
    if rc == 0:
        L.lib.fu_destroy(h)
    return rc, text


def _create(rp, col, rev=None, *, n=None, e=None, value=None, out=True):
    """(code, text) of fu_create; a handle that does get made (a host with a GPU) is destroyed."""
    n = len(rp) - 1 if n is None else n
    e = int(rp[-1]) if e is None else e
    value = np.ones(max(n, 1)) if value is None else value
    h = L.vp()
    rc = L.lib.fu_create(n, e, _p(rp), _p(col), _p(rev), _p(value), 0, ctypes.byref(h) if out else None)
    return _finish(rc, h)


def _past_validation(got):
    """Every check passed: without a GPU the next thing is the device probe's error."""
    if fu.device_count() == 0:
        assert got == NO_DEVICE, got
    else:
        assert got[0] == 0, got


# ------------------------------------------------------------------------------------
# fu_create
# ------------------------------------------------------------------------------------
_BAD = "fu_create: bad arguments"
_ENDS = "fu_create: rowptr[0] must be 0 and rowptr[n] == e"
_MONO = "fu_create: rowptr not monotone"
_COL = "fu_create: col index out of range at edge "
_REV = "fu_create: rev is not the reverse-edge pairing (the graph must be symmetric) at edge "
_MANY = "fu_create: more than 2^31-1 edges"
_ASYM = "graph is not symmetric (edge 0 has no reverse edge)"  # the rev builder's, names no caller

# (what, kwargs of _create, code, text). Rows without a "rev" are tried with rev NULL and with
# a rev of the right length, so both branches of fu_create are walked.
CREATE_ROWS = [
    ("null out", dict(rp=PATH_RP, col=PATH_COL, out=False), ARG, _BAD),
    ("null rowptr", dict(rp=NULL, col=PATH_COL, n=3, e=4), ARG, _BAD),
    ("null value", dict(rp=PATH_RP, col=PATH_COL, value=NULL), ARG, _BAD),
    ("n == 0", dict(rp=PATH_RP, col=PATH_COL, n=0), ARG, _BAD),
    ("n < 0", dict(rp=PATH_RP, col=PATH_COL, n=-3), ARG, _BAD),
    ("e < 0", dict(rp=PATH_RP, col=PATH_COL, e=-1), ARG, _BAD),
    ("e > 0, null col", dict(rp=PATH_RP, col=NULL), ARG, _BAD),
    # only the scalar is large: the check comes before any array is read
    ("e = 2^31", dict(rp=PATH_RP, col=PATH_COL, e=2 ** 31), ARG, _MANY),
    ("e = INT32_MAX - 64", dict(rp=PATH_RP, col=PATH_COL, e=2 ** 31 - 1 - 64), ARG, _MANY),
    ("e = INT32_MAX - 65", dict(rp=PATH_RP, col=PATH_COL, e=2 ** 31 - 1 - 65), ARG, _ENDS),
    ("rowptr[0] != 0", dict(rp=_i64(1, 1, 3, 4), col=PATH_COL), ARG, _ENDS),
    ("rowptr[n] != e", dict(rp=PATH_RP, col=PATH_COL, e=3), ARG, _ENDS),
    ("rowptr not monotone", dict(rp=_i64(0, 3, 1, 4), col=PATH_COL), ARG, _MONO),
    ("rowptr [0, 100, 4]", dict(rp=_i64(0, 100, 4), col=TWO_COL), ARG, _MONO),
    ("rowptr [0, 100, 2, 4]", dict(rp=_i64(0, 100, 2, 4), col=PATH_COL), ARG, _MONO),
    ("rowptr [0, 2^40, 4]", dict(rp=_i64(0, 2 ** 40, 4), col=TWO_COL), ARG, _MONO),
    ("rowptr [0, -5, 4]", dict(rp=_i64(0, -5, 4), col=TWO_COL), ARG, _MONO),
    ("rowptr [0, 1, -100, 4]", dict(rp=_i64(0, 1, -100, 4), col=PATH_COL), ARG, _MONO),
    ("col too large", dict(rp=PATH_RP, col=_i32(1, 3000, 2, 1)), ARG, _COL + "1"),
    ("col == n", dict(rp=PATH_RP, col=_i32(1, 0, 3, 1)), ARG, _COL + "2"),
    ("col negative", dict(rp=PATH_RP, col=_i32(1, 0, 2, -1)), ARG, _COL + "3"),
    ("col INT32_MIN", dict(rp=PATH_RP, col=_i32(-2 ** 31, 0, 2, 1)), ARG, _COL + "0"),
    ("self-loop", dict(rp=PATH_RP, col=_i32(1, 1, 2, 1)), GRAPH, "fu_create: self-loop at node 1"),
    # both loops paired with themselves: the symmetric check and the pairing check would pass
    ("self-loops, rev[k] == k", dict(rp=_i64(0, 2, 4), col=_i32(0, 1, 0, 1), rev=_i32(0, 2, 1, 3)), GRAPH,
     "fu_create: self-loop at node 0"),
    ("self-loop on the last row", dict(rp=_i64(0, 1, 4), col=_i32(1, 0, 1, 1)), GRAPH, "fu_create: self-loop at node 1"),
    ("rev too large", dict(rp=PATH_RP, col=PATH_COL, rev=_i32(1, 0, 4, 2)), GRAPH, _REV + "2"),
    ("rev far too large", dict(rp=PATH_RP, col=PATH_COL, rev=_i32(1, 0, 3, 2 ** 31 - 1)), GRAPH, _REV + "3"),
    ("rev negative", dict(rp=PATH_RP, col=PATH_COL, rev=_i32(-1, 0, 3, 2)), GRAPH, _REV + "0"),
    ("rev into the wrong row", dict(rp=PATH_RP, col=PATH_COL, rev=_i32(3, 2, 1, 0)), GRAPH, _REV + "0"),
    # slot 0 (0 -> 1) names slot 3: in row 1, but that slot holds node 2
    ("rev at another node's slot", dict(rp=TRI_RP, col=TRI_COL, rev=_i32(3, 4, 0, 5, 1, 2)), GRAPH, _REV + "0"),
    ("asymmetric, no rev", dict(rp=_i64(0, 1, 1), col=_i32(1), rev=None), GRAPH, _ASYM),
]


def _create_calls():
    """Every failing call of the table: (what, kwargs, code, text)."""
    for what, kw, code, text in CREATE_ROWS:
        if "rev" in kw:
            yield what, kw, code, text
        else:
            yield what + ", rev NULL", dict(kw, rev=None), code, text
            yield what + ", with a rev", dict(kw, rev=TWO_REV if kw["col"] is TWO_COL else PATH_REV), code, text


def _walk_failing_table():
    for what, kw, code, text in _create_calls():
        assert _create(**kw) == (code, text), what


def test_create_argument_and_graph_errors():
    _walk_failing_table()
    assert len(list(_create_calls())) == 2 * len(CREATE_ROWS) - 7


def test_create_check_order():
    """The scalars before rowptr's ends, those before monotonicity, that before the columns, all
    of them before the graph checks: a call wrong in several ways names the first."""
    both = dict(rp=_i64(0, 100, 4), col=_i32(1, 7, 0, 0))  # not monotone, and a col out of range
    assert _create(**both) == (ARG, _MONO)
    assert _create(**both, e=5) == (ARG, _ENDS)
    assert _create(**both, e=5, value=NULL) == (ARG, _BAD)
    assert _create(**both, e=2 ** 31) == (ARG, _MANY)
    assert _create(**both, e=2 ** 31, out=False) == (ARG, _BAD)
    # a col out of range at edge 3 and a self-loop at edge 1: the range first
    assert _create(PATH_RP, _i32(1, 1, 2, 9)) == (ARG, _COL + "3")
    # a self-loop and a rev that is no pairing: the loop first
    assert _create(PATH_RP, _i32(1, 1, 2, 1), _i32(3, 2, 1, 0)) == (GRAPH, "fu_create: self-loop at node 1")
    # a doubled edge is no self-loop and stays what it was: symmetric, so past the checks
    _past_validation(_create(_i64(0, 2, 4), TWO_COL, _i32(2, 2, 0, 1)))
    _past_validation(_create(_i64(0, 2, 4), TWO_COL))


# ------------------------------------------------------------------------------------
# fu_create_from_graph, fu_create_from_graph_ex
# ------------------------------------------------------------------------------------
def _from_graph(g, *, value=True, out=True, layout=None):
    v = np.ones(2) if value else None
    h = L.vp()
    o = ctypes.byref(h) if out else None
    if layout is None:
        rc = L.lib.fu_create_from_graph(g, _p(v), 0, o)
    else:
        rc = L.lib.fu_create_from_graph_ex(g, _p(v), 0, layout, o)
    return _finish(rc, h)


def test_create_from_graph_errors():
    sym = fu.Graph.from_csr(_i64(0, 1, 2), _i32(1, 0))
    asym = fu.Graph.from_csr(_i64(0, 1, 1), _i32(1), require_symmetric=False)
    assert _from_graph(None) == (ARG, "fu_create_from_graph: NULL graph")
    assert _from_graph(sym._h, value=False) == (ARG, _BAD)
    assert _from_graph(sym._h, out=False) == (ARG, _BAD)
    assert _from_graph(asym._h) == (GRAPH, "fu_create_from_graph: graph is not symmetric")
    _past_validation(_from_graph(sym._h))
    ex = (ARG, "fu_create_from_graph_ex: bad arguments")
    assert _from_graph(None, layout=0) == ex
    assert _from_graph(sym._h, value=False, layout=0) == ex
    assert _from_graph(sym._h, out=False, layout=1) == ex
    assert _from_graph(sym._h, layout=-1) == ex
    assert _from_graph(sym._h, layout=2) == ex
    for layout in (0, 1):
        assert _from_graph(asym._h, layout=layout) == (GRAPH, "fu_create_from_graph: graph is not symmetric"), layout
        _past_validation(_from_graph(sym._h, layout=layout))


# ------------------------------------------------------------------------------------
# fu_dist_create_local, fu_dist_create
# ------------------------------------------------------------------------------------
# rank 0 of the path of 3 cut at [0, 2, 3]: rows 0 and 1, node 2 in ghost slot 0 (column 2);
# it sends node 1 to rank 1 and hears one estimate from it
R0 = dict(n_local=2, e_local=3, rp=_i64(0, 1, 3), col=_i32(1, 0, 2), n_ghost_a=1, nranks=2, rank=0,
          send_a_off=_i64(0, 0, 1), send_a_idx=_i32(1), recv_a_off=_i64(0, 0, 1))
# rank 1: row 2, node 1 in ghost slot 0 (column 1)
R1 = dict(n_local=1, e_local=1, rp=_i64(0, 1), col=_i32(1), n_ghost_a=1, nranks=2, rank=1,
          send_a_off=_i64(0, 1, 1), send_a_idx=_i32(0), recv_a_off=_i64(0, 1, 1))
UID = (ctypes.c_uint8 * 128)()


def _dist_local(*, n_local, e_local, rp, col, n_ghost_a, nranks, rank, send_a_off, send_a_idx, recv_a_off, value=None,
                out=True):
    value = np.ones(max(n_local, 1)) if value is None else value
    h = L.vp()
    rc = L.lib.fu_dist_create_local(n_local, e_local, _p(rp), _p(col), _p(value), n_ghost_a, nranks, rank,
                                    _p(send_a_off), _p(send_a_idx), _p(recv_a_off), 0, ctypes.byref(h) if out else None)
    return _finish(rc, h)


def _dist(*, n_local, e_local, rp, col, n_ghost_a, nranks, rank, send_a_off, send_a_idx, recv_a_off, value=None,
          out=True, rev=None, n_ghost_f=0, send_f_off=None, send_f_idx=None, recv_f_off=None, uid=UID):
    """fu_dist_create with a zeroed unique id: no row here may get as far as the communicator."""
    value = np.ones(max(n_local, 1)) if value is None else value
    zf = np.zeros(max(nranks, 0) + 1, dtype=np.int64)
    send_f_off = zf if send_f_off is None else send_f_off
    recv_f_off = zf if recv_f_off is None else recv_f_off
    h = L.vp()
    rc = L.lib.fu_dist_create(n_local, e_local, _p(rp), _p(col), _p(rev), _p(value), n_ghost_a, n_ghost_f, nranks,
                              rank, _p(send_f_off), _p(send_f_idx), _p(recv_f_off), _p(send_a_off), _p(send_a_idx),
                              _p(recv_a_off), uid, 0, ctypes.byref(h) if out else None)
    assert rc != 0, "a row of the fu_dist_create table passed the host checks"
    return rc, L.last_error()


_DBAD = "fu_dist_create: bad arguments"
_HALO = "fu_dist_create: halo offsets inconsistent with ghost counts"
_SEND = "fu_dist_create: send_a_idx out of range"
_EST = "fu_dist_create: the halo carries estimates only (rev must be NULL, no ghost flows)"
# (what, overrides of R0, code, text): the same from both entry points
DIST_ROWS = [
    ("null out", dict(out=False), ARG, _DBAD),
    ("nranks == 0", dict(nranks=0), ARG, _DBAD),
    ("nranks < 0", dict(nranks=-2), ARG, _DBAD),
    ("rank < 0", dict(rank=-1), ARG, _DBAD),
    ("rank == nranks", dict(rank=2), ARG, _DBAD),
    ("null send_a_off", dict(send_a_off=NULL), ARG, _DBAD),
    ("null recv_a_off", dict(recv_a_off=NULL), ARG, _DBAD),
    ("n_ghost_a < 0", dict(n_ghost_a=-1), ARG, _DBAD),
    ("recv_a_off[0] != 0", dict(recv_a_off=_i64(1, 1, 1)), ARG, _HALO),
    ("recv_a_off[nranks] < n_ghost_a", dict(recv_a_off=_i64(0, 0, 0)), ARG, _HALO),
    ("recv_a_off[nranks] > n_ghost_a", dict(recv_a_off=_i64(0, 0, 2)), ARG, _HALO),
    ("n_ghost_a without a receive plan", dict(n_ghost_a=2), ARG, _HALO),
    ("send_a_off[0] != 0", dict(send_a_off=_i64(1, 1, 1)), ARG, _HALO),
    ("send_a_idx == n_local", dict(send_a_idx=_i32(2)), ARG, _SEND),
    ("send_a_idx negative", dict(send_a_idx=_i32(-1)), ARG, _SEND),
    ("send_a_idx far too large", dict(send_a_idx=_i32(2 ** 31 - 1)), ARG, _SEND),
    # the halo plan is good: the local CSR, under the shared constructor's texts
    ("null rowptr", dict(rp=NULL), ARG, _BAD),
    ("null value", dict(value=NULL), ARG, _BAD),
    ("e_local > 0, null col", dict(col=NULL), ARG, _BAD),
    ("n_local < 0", dict(n_local=-2), ARG, _SEND),  # the send list is checked against n_local first
    ("n_local < 0, nothing to send", dict(n_local=-2, send_a_off=_i64(0, 0, 0)), ARG, _BAD),
    ("e_local < 0", dict(e_local=-1), ARG, _BAD),
    ("e_local = 2^31", dict(e_local=2 ** 31), ARG, _MANY),
    ("rowptr[0] != 0", dict(rp=_i64(1, 1, 3)), ARG, _ENDS),
    ("rowptr[n] != e", dict(e_local=2), ARG, _ENDS),
    ("rowptr not monotone", dict(rp=_i64(0, 100, 3)), ARG, _MONO),
    ("rowptr negative", dict(rp=_i64(0, -1, 3)), ARG, _MONO),
    ("col == n_local + n_ghost_a", dict(col=_i32(1, 0, 3)), ARG, _COL + "2"),
    ("col negative", dict(col=_i32(-1, 0, 2)), ARG, _COL + "0"),
    ("self-loop on a local row", dict(col=_i32(1, 1, 2)), GRAPH, "fu_dist_create: self-loop at node 1"),
    ("self-loop on row 0", dict(col=_i32(0, 0, 2)), GRAPH, "fu_dist_create: self-loop at node 0"),
]


def _walk_failing_dist_table():
    for what, over, code, text in DIST_ROWS:
        assert _dist_local(**{**R0, **over}) == (code, text), ("fu_dist_create_local", what)
        assert _dist(**{**R0, **over}) == (code, text), ("fu_dist_create", what)
    # fu_dist_create alone: the parts of its plan that the estimates-only halo has no use for
    assert _dist(**R0, uid=None) == (ARG, "fu_dist_create: NULL unique_id")
    assert _dist(**R0, n_ghost_f=-1) == (ARG, _DBAD)
    assert _dist(**R0, send_f_off=NULL) == (ARG, _DBAD)
    assert _dist(**R0, recv_f_off=NULL) == (ARG, _DBAD)
    assert _dist(**R0, n_ghost_f=1) == (ARG, _HALO)  # recv_f_off[nranks] == 0 != n_ghost_f
    assert _dist(**R0, recv_f_off=_i64(1, 1, 1), n_ghost_f=1) == (ARG, _HALO)
    assert _dist(**R0, send_f_off=_i64(1, 1, 1)) == (ARG, _HALO)
    assert _dist(**R0, rev=_i32(1, 0, 3)) == (ARG, _EST)
    assert _dist(**R0, n_ghost_f=1, recv_f_off=_i64(0, 0, 1)) == (ARG, _EST)
    assert _dist(**R0, send_f_off=_i64(0, 0, 1), send_f_idx=_i32(2)) == (ARG, _EST)


def test_dist_create_argument_and_graph_errors():
    _walk_failing_dist_table()


def test_dist_rows_are_the_partition_of_the_path():
    """R0 and R1 are what fu.dist.partition makes of the path of 3 cut at [0, 2, 3]."""
    for want, rank in ((R0, 0), (R1, 1)):
        p = partition(PATH_RP, PATH_COL, PATH_REV, 2, rank, bounds=[0, 2, 3])
        got = dict(n_local=p.n_local, e_local=p.e_local, rp=p.rowptr, col=p.col, n_ghost_a=p.n_ghost_a, nranks=2,
                   rank=rank, send_a_off=p.send_a_off, send_a_idx=p.send_a_idx, recv_a_off=p.recv_a_off)
        assert got.keys() == want.keys()
        for k in want:
            assert np.array_equal(got[k], want[k]), (rank, k)


# ------------------------------------------------------------------------------------
# good inputs reach the device probe
# ------------------------------------------------------------------------------------
def test_good_inputs_reach_the_device_probe():
    """A path of 3 with and without the caller's rev, three nodes without an edge (with and
    without a col array), and both ranks of the path's 2-rank cut; col == n_local + n_ghost_a - 1
    is rank 0's ghost column."""
    _past_validation(_create(PATH_RP, PATH_COL))
    _past_validation(_create(PATH_RP, PATH_COL, PATH_REV))
    zero = np.zeros(4, dtype=np.int64)
    _past_validation(_create(zero, NULL))
    _past_validation(_create(zero, np.zeros(1, dtype=np.int32)))
    assert R0["col"][2] == R0["n_local"] + R0["n_ghost_a"] - 1
    _past_validation(_dist_local(**R0))
    _past_validation(_dist_local(**R1))
    # a ghost column is never a self-loop, whatever local row holds it
    _past_validation(_dist_local(**{**R0, "col": _i32(2, 2, 2)}))


# ------------------------------------------------------------------------------------
# the same rows under AddressSanitizer and UndefinedBehaviorSanitizer (tools/create_check.cpp)
# ------------------------------------------------------------------------------------
def test_checks_read_nothing_out_of_bounds():
    """The checks above, called from a stand-alone host program on heap blocks of each array's
    exact length. Before the checks were put in order, fu_create's rev builder walked
    rowptr = [0, 100, 4] and col = [1, 3000, 2, 1] unchecked: heap-buffer-overflow in
    fu::build_rev."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "bin/create_check"], check=True)
    p = subprocess.run([os.path.join(ROOT, "tools", "bin", "create_check")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
                                UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert " cases, 0 failed" in p.stdout, p.stdout


# ------------------------------------------------------------------------------------
# on the GPU: failed creates leave nothing behind
# ------------------------------------------------------------------------------------
def _fixture(name):
    d = load_npz(dict(ca_sync_fixtures())[name]["file"])
    rp, col = np.asarray(d["rowptr"], dtype=np.int64), np.asarray(d["col"], dtype=np.int32)
    return rp, col, fu.Graph.from_csr(rp, col).rev, np.asarray(d["values"], dtype=np.float64)


def _oracle_at(rp, col, rev, v, stops):
    """{r: (estimates, flows)} after r rounds, r in stops, from the C oracle."""
    out, done = {}, 0
    for r in sorted(stops):
        if done == 0:
            a, f = coracle.ca_sync(rp, col, rev, v, r)
        else:
            coracle.ca_rounds(rp, col, rev, v, r - done, a, f)
        done = r
        out[r] = (a.copy(), f.copy())
    return out


@pytest.mark.gpu
def test_good_handles_after_the_failing_table():
    """Every failing row first, then good handles on the same thread through the raw path: the
    path of 3 and rr64_d4, 7 rounds of kernels 4 and 8, bit-equal to the oracle. fu_last_error()
    is written by a failing call alone: after the good handles it still holds the last failed
    row's text, so none of their calls failed quietly."""
    _walk_failing_table()
    _walk_failing_dist_table()
    last = L.last_error()
    assert last == _EST
    rr = _fixture("rr64_d4")
    for rp, col, rev, v in ((PATH_RP, PATH_COL, PATH_REV, np.array([3.0, -1.5, 10.25])), rr):
        ref = _oracle_at(rp, col, rev, v, (7,))[7]
        for kernel in ("recon", "stage"):
            for r in (None, rev):
                with fu.CollectAll(rowptr=rp, col=col, rev=r, values=v, kernel=kernel) as eng:
                    eng.run(7)
                    assert eng.rounds_done == 7
                    assert_same_bits(eng.estimates(), ref[0], (len(v), kernel, r is None))
                    assert_same_bits(eng.flows(), ref[1], (len(v), kernel, r is None))
    assert L.last_error() == last
    # a failure between two runs of one handle changes nothing either
    rp, col, rev, v = rr
    ref = _oracle_at(rp, col, rev, v, (3, 7))
    with fu.CollectAll(rowptr=rp, col=col, values=v, kernel="recon") as eng:
        eng.run(3)
        assert_same_bits(eng.estimates(), ref[3][0])
        _walk_failing_table()
        eng.run(4)
        assert_same_bits(eng.estimates(), ref[7][0])
        assert_same_bits(eng.flows(), ref[7][1])


STOPS = (1, 2, 3, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rr256_d8_shuffled", "star_257"])
def test_three_ways_to_one_handle(name):
    """fu_create with the caller's rev, with rev NULL, and fu_create_from_graph on the same CSR
    (rows not sorted; one heavy row): the same estimate and flow bits after rounds 1, 2, 3, 7,
    and those are the oracle's."""
    rp, col, rev, v = _fixture(name)
    ref = _oracle_at(rp, col, rev, v, STOPS)
    engines = {"rev": fu.CollectAll(rowptr=rp, col=col, rev=rev, values=v, kernel="recon"),
               "no rev": fu.CollectAll(rowptr=rp, col=col, values=v, kernel="recon"),
               "graph": fu.CollectAll(fu.Graph.from_csr(rp, col), v, kernel="recon")}
    done = 0
    for r in STOPS:
        for how, eng in engines.items():
            eng.run(r - done)
            assert_same_bits(eng.estimates(), ref[r][0], (name, how, r))
            assert_same_bits(eng.flows(), ref[r][1], (name, how, r))
        done = r
    for eng in engines.values():
        eng.close()


@pytest.mark.gpu
def test_two_rank_cut_against_the_single_handle():
    """A 2-rank fu_dist_create_local cut of er300_m450 against fu_create on the whole graph,
    after rounds 1, 2, 3 and 7: the ranks' rows are the single handle's rows, bit for bit."""
    rp, col, rev, v = _fixture("er300_m450")
    plans = [partition(rp, col, rev, 2, r) for r in range(2)]
    ranks = [DistCollectAll(p, v[p.lo:p.hi], None, kernel="recon") for p in plans]
    one = fu.CollectAll(rowptr=rp, col=col, rev=rev, values=v, kernel="recon")
    ref = _oracle_at(rp, col, rev, v, STOPS)
    done = 0
    for r in STOPS:
        run_local(ranks, r - done)
        one.run(r - done)
        done = r
        a, f = one.estimates(), one.flows()
        assert_same_bits(a, ref[r][0], r)
        assert_same_bits(f, ref[r][1], r)
        assert_same_bits(np.concatenate([e.estimates() for e in ranks]), a, ("ranks", r))
        assert_same_bits(np.concatenate([e.flows() for e in ranks]), f, ("ranks", r))
    for e in ranks + [one]:
        e.close()


@pytest.mark.gpu
def test_failing_table_leaves_the_device_memory_alone():
    """fu_mem_info's free bytes after both failing tables equal the value before them: exactly,
    since no row gets as far as an allocation. A handle is made and destroyed first, so the
    runtime's own first-use allocations are not counted."""
    with fu.CollectAll(rowptr=PATH_RP, col=PATH_COL, values=np.ones(3)) as eng:
        eng.run(1)
    free0, _ = fu.mem_info(0)
    _walk_failing_table()
    _walk_failing_dist_table()
    free1, _ = fu.mem_info(0)
    print("free bytes before", free0, "after", free1)
    assert free1 == free0
