"""The K-column entry points of the pairwise engine without a GPU: the three symbols and their
signatures, the argument errors of fu_pair_create_k and fu_pair_create_from_graph_k (all checked
before any HIP call), the shape errors of fu.PairwiseSyncBatch (raised before any C call) and
the command line's --pair-columns."""
import ctypes
import inspect

import numpy as np
import pytest

import fu
from fu import _lib as L
from pair_cases import rr256_d8

i32, i64, vp, P = L.i32, L.i64, L.vp, L.P

SIGNATURES = {
    "fu_pair_create_k": [i32, i64, vp, vp, vp, i32, vp, i32, P(vp)],
    "fu_pair_create_from_graph_k": [vp, i32, vp, i32, P(vp)],
    "fu_pair_get_columns": [vp, P(i32)],
}


def test_the_three_symbols_and_their_signatures():
    for name, args in SIGNATURES.items():
        assert hasattr(L.lib, name), name
        assert name in L.EXPORTED
        f = getattr(L.lib, name)
        assert list(f.argtypes) == args and f.restype is ctypes.c_int, name
    assert L.lib.fu_version() == 2
    assert hasattr(fu, "PairwiseSyncBatch") and "PairwiseSyncBatch" in fu.__all__
    assert issubclass(fu.PairwiseSyncBatch, fu.PairwiseSync)
    kw = inspect.signature(fu.PairwiseSyncBatch.__init__).parameters
    assert kw["seed"].default == 0 and kw["loss"].default == 0.0 and kw["loss_seed"].default == 0
    assert kw["link_mask"].default is None
    import os

    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fu.h")) as f:
        header = f.read()
    for name in SIGNATURES:
        assert f"int {name}(" in header, name


def _create_k(rp, col, rev, k, v, out=True):
    h = L.vp()
    rc = L.lib.fu_pair_create_k(len(rp) - 1, int(rp[-1]), L.ptr(rp), L.ptr(col), None if rev is None else L.ptr(rev), k,
                                None if v is None else L.ptr(v), 0, ctypes.byref(h) if out else None)
    if rc == 0:
        L.lib.fu_pair_destroy(h)
    return rc


def test_bad_k_and_null_pointers_come_before_any_hip_call():
    g = rr256_d8()
    rp, col, rev = g.arrays()
    for k in (0, 17, -1):
        v = np.ones((g.n, max(k, 1)))
        assert _create_k(rp, col, rev, k, v) == -1, k
        assert L.last_error() == f"fu_pair_create_k: k must be in 1..16, got {k}"
        h = L.vp()
        assert L.lib.fu_pair_create_from_graph_k(g._h, k, L.ptr(v), 0, ctypes.byref(h)) == -1, k
        assert L.last_error() == f"fu_pair_create_from_graph_k: k must be in 1..16, got {k}"
    v = np.ones((g.n, 2))
    assert _create_k(rp, col, rev, 2, None) == -1
    assert L.last_error() == "fu_pair_create_k: bad arguments"
    assert _create_k(rp, col, rev, 2, v, out=False) == -1
    assert L.last_error() == "fu_pair_create_k: bad arguments"
    h = L.vp()
    assert L.lib.fu_pair_create_k(g.n, g.E, None, L.ptr(col), None, 2, L.ptr(v), 0, ctypes.byref(h)) == -1
    assert L.lib.fu_pair_create_k(g.n, g.E, L.ptr(rp), None, None, 2, L.ptr(v), 0, ctypes.byref(h)) == -1
    assert L.lib.fu_pair_create_k(0, 0, L.ptr(rp), L.ptr(col), None, 2, L.ptr(v), 0, ctypes.byref(h)) == -1  # n = 0
    assert L.lib.fu_pair_create_from_graph_k(None, 2, L.ptr(v), 0, ctypes.byref(h)) == -1
    assert L.last_error() == "fu_pair_create_from_graph: bad arguments"
    assert L.lib.fu_pair_create_from_graph_k(g._h, 2, None, 0, ctypes.byref(h)) == -1
    assert L.lib.fu_pair_create_from_graph_k(g._h, 2, L.ptr(v), 0, None) == -1
    k = i32(0)
    assert L.lib.fu_pair_get_columns(None, ctypes.byref(k)) == -1
    assert L.last_error() == "fu_pair_get_columns: bad arguments"
    c = col.copy()
    c[0] = g.n  # a column out of range is the CSR's own error, under this entry point's name
    assert _create_k(rp, c, None, 2, v) == -1
    assert "fu_pair_create_k" in L.last_error()


def test_asymmetric_graph_and_bad_rev_are_graph_errors():
    rp = np.array([0, 1, 1], dtype=np.int64)
    col = np.array([1], dtype=np.int32)
    v2 = np.ones((2, 3))
    assert _create_k(rp, col, None, 3, v2) == -5
    assert "not symmetric" in L.last_error()
    with pytest.raises(fu.FuError) as ei:
        fu.PairwiseSyncBatch(rowptr=rp, col=col, values=v2)
    assert ei.value.code == -5
    asym = fu.Graph.from_csr(rp, col, require_symmetric=False)
    with pytest.raises(fu.FuError) as ei:
        fu.PairwiseSyncBatch(asym, v2)
    assert ei.value.code == -5 and "fu_pair_create_from_graph: graph is not symmetric" in str(ei.value)
    g = rr256_d8()
    rp, col, rev = g.arrays()
    v = np.ones((g.n, 3))
    for bad in ("swapped", "out of range", "negative"):
        r = rev.copy()
        if bad == "swapped":
            r[[0, 1]] = r[[1, 0]]
        elif bad == "out of range":
            r[10] = g.E
        else:
            r[10] = -1
        assert _create_k(rp, col, r, 3, v) == -5, bad
        assert "rev" in L.last_error()
    if fu.device_count() == 0:  # what passes every check reaches the device probe
        assert _create_k(rp, col, rev, 3, v) == -2
        assert "no HIP device" in L.last_error()
        assert _create_k(rp, col, None, 16, np.ones((g.n, 16))) == -2


def test_shape_errors_are_value_errors_before_any_c_call(monkeypatch):
    g = rr256_d8()
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    with pytest.raises(ValueError):
        fu.PairwiseSyncBatch(g, np.ones(g.n))  # (n,)
    with pytest.raises(ValueError):
        fu.PairwiseSyncBatch(g, np.ones((g.n + 1, 2)))
    with pytest.raises(ValueError):
        fu.PairwiseSyncBatch(rowptr=g.rowptr, col=g.col, rev=g.rev, values=np.ones((g.n + 1, 2)))
    with pytest.raises(ValueError):
        fu.PairwiseSyncBatch(rowptr=g.rowptr, col=g.col, rev=g.rev, values=np.ones(g.n))
    with pytest.raises(ValueError):
        fu.PairwiseSyncBatch(g, np.ones((g.n, 2, 1)))
    assert calls == []
    # a handle that was never opened on the device still checks widths before it calls C
    eng = fu.PairwiseSyncBatch.__new__(fu.PairwiseSyncBatch)
    eng._h, eng.n, eng.E, eng.K, eng._cols = None, g.n, g.E, 3, 3
    for bad in (np.ones(g.n), np.ones((g.n, 2)), np.ones((g.n, 4)), np.ones((g.n + 1, 3)), np.ones((3, g.n))):
        with pytest.raises(ValueError):
            eng.set_targets(bad)
        with pytest.raises(ValueError):
            eng.set_values(bad)
    with pytest.raises(ValueError):
        eng.set_link_mask(np.zeros((g.E, 3), dtype=np.uint8))  # the mask is per slot, not per column
    assert calls == []


def _cli_error(argv, capsys):
    from fu.__main__ import main

    with pytest.raises(SystemExit) as ex:
        main(argv)
    assert ex.value.code == 2
    return capsys.readouterr().err


def test_cli_pair_columns_needs_pairs_and_a_width_in_range(capsys):
    base = ["bench-graph", "er:n=200,m=800", "--rounds", "4"]
    assert "--pair-columns" in _cli_error(base + ["--pair-columns", "3"], capsys)
    assert "--pair-columns" in _cli_error(base + ["--pair-columns", "3", "--loss", "0.1"], capsys)
    assert "--pair-columns" in _cli_error(base + ["--pair-columns", "3", "--churn", "0.1"], capsys)
    assert "--pair-columns" in _cli_error(["collectall", "--pair-columns", "3", "--pairs"], capsys)
    for k in ("0", "17"):
        assert "1..16" in _cli_error(base + ["--pairs", "--pair-columns", k], capsys)
    assert "--columns" in _cli_error(base + ["--pairs", "--columns", "3"], capsys)
    assert "--columns" in _cli_error(base + ["--pairs", "--columns", "3", "--pair-columns", "3"], capsys)


def test_cli_pair_columns_reaches_the_batch_engine(capsys, monkeypatch):
    """--pairs --pair-columns K hands _columns(n, K) to the K-column class (a stand-in here: no
    GPU), --loss goes with it, and the line is the --pairs line with columns=K appended."""
    import fu.__main__ as cli

    made = {}

    class Stand:
        stats = (7, 0)
        loss_stats = (2, 1, 4)

        def __init__(self, g, v, seed=0, device=0):
            made["shape"], made["seed"], made["count"] = v.shape, seed, v[:, 1].copy()

        def set_loss(self, p, seed=0):
            made["loss"] = (p, seed)

        def run_timed(self, rounds):
            return 1.0

        def set_targets(self, t):
            made["targets"] = t.shape

        def max_err(self):
            return np.array([0.25, 0.5, 0.125])

    monkeypatch.setattr(cli, "PairwiseSyncBatch", Stand)
    argv = ["bench-graph", "er:n=200,m=800", "--rounds", "4", "--pairs", "--pair-seed", "4", "--pair-columns", "3"]
    assert cli.main(argv) == 0
    line = capsys.readouterr().out.strip()
    assert made["shape"] == (200, 3) and made["targets"] == (200, 3) and made["seed"] == 4 and "loss" not in made
    assert made["count"][0] == 1.0 and not made["count"][1:].any()  # the COUNT indicator
    assert line.endswith(" max_err=5.000e-01 pairs=7 columns=3") and " rounds=4 " in line
    assert cli.main(argv + ["--loss", "0.25", "--loss-seed", "9"]) == 0
    assert made["loss"] == (0.25, 9)
    assert capsys.readouterr().out.strip().endswith(" pairs=7 lost=3 columns=3")
