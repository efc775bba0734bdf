"""The pairwise engine's topology entry points without a GPU: the symbols, the argument errors
(all checked before any HIP call), the Python shape errors and the command line."""
import inspect

import numpy as np
import pytest

import fu
from fu import _lib as L
from pair_cases import rr256_d8

TOPOLOGY_SYMBOLS = ["fu_pair_set_topology", "fu_pair_get_topology_stats", "fu_pair_get_slot_live", "fu_pair_matching_live"]


def test_the_symbols_load():
    for s in TOPOLOGY_SYMBOLS:
        assert hasattr(L.lib, s), s
        assert s in L.EXPORTED
    for cls in (fu.PairwiseSync, fu.PairwiseSyncBatch):
        for name in ("set_topology", "topology_stats", "slot_live"):
            assert hasattr(cls, name), name
        kw = inspect.signature(cls.set_topology).parameters
        assert kw["alive"].default is None and kw["link_up"].default is None
    kw = inspect.signature(fu.pair_matching).parameters
    assert list(kw) == ["g", "seed", "r", "alive", "link_up"] and kw["alive"].default is None and kw["link_up"].default is None
    for name in ("PairwiseSync", "PairwiseSyncBatch", "pair_matching", "churn_live", "churn_targets"):
        assert name in fu.__all__


def test_bad_arguments_come_before_any_hip_call():
    out = np.zeros(2, dtype=np.int64)
    one = np.ones(8, dtype=np.uint8)
    assert L.lib.fu_pair_set_topology(None, None, None) == -1
    assert "fu_pair_set_topology" in L.last_error()
    assert L.lib.fu_pair_set_topology(None, L.ptr(one), L.ptr(one)) == -1
    assert L.lib.fu_pair_get_topology_stats(None, L.ptr(out)) == -1
    assert "fu_pair_get_topology_stats" in L.last_error()
    assert L.lib.fu_pair_get_slot_live(None, L.ptr(one)) == -1
    assert "fu_pair_get_slot_live" in L.last_error()
    g = rr256_d8()
    rp, col, _ = g.arrays()
    mate, ini = np.zeros(g.n, dtype=np.int32), np.zeros(g.n, dtype=np.uint8)
    up = np.ones(g.E, dtype=np.uint8)
    ok = (g.n, L.ptr(rp), L.ptr(col), None, L.ptr(up), 1, 0, L.ptr(mate), L.ptr(ini))
    assert L.lib.fu_pair_matching_live(*ok) == 0
    for q, bad in ((0, 0), (1, None), (6, -1), (7, None), (8, None)):
        args = list(ok)
        args[q] = bad
        assert L.lib.fu_pair_matching_live(*args) == -1, q
        assert "fu_pair_matching_live" in L.last_error()


def test_asymmetric_link_up_names_the_slot():
    g = rr256_d8()
    rev = np.asarray(g.rev)
    up = np.ones(g.E, dtype=np.uint8)
    k = 37
    up[max(k, rev[k])] = 0  # the first offending slot is the smaller of the two
    with pytest.raises(fu.FuError) as ei:
        fu.pair_matching(g, 1, 0, link_up=up)
    assert ei.value.code == -1
    assert f"fu_pair_matching_live: link_up differs between slot {min(k, rev[k])} and its reverse" in str(ei.value)
    up[:] = 2  # any non-zero byte is true
    fu.pair_matching(g, 1, 0, link_up=up)


def test_python_shape_errors():
    g = rr256_d8()
    with pytest.raises(ValueError):
        fu.pair_matching(g, 1, 0, alive=np.ones(g.n + 1, dtype=np.uint8))
    with pytest.raises(ValueError):
        fu.pair_matching(g, 1, 0, link_up=np.ones(g.E - 1, dtype=np.uint8))
    with pytest.raises(ValueError):
        fu.pair_matching(g, 1, 0, alive=np.ones(g.n))  # a float mask


@pytest.mark.gpu
def test_errors_on_a_live_handle():
    g = rr256_d8()
    rev = np.asarray(g.rev)
    with fu.PairwiseSync(g, np.ones(g.n)) as eng:
        with pytest.raises(ValueError):
            eng.set_topology(alive=np.ones(g.n - 1, dtype=np.uint8))
        with pytest.raises(ValueError):
            eng.set_topology(link_up=np.ones(g.E))
        up = np.ones(g.E, dtype=np.uint8)
        up[max(5, rev[5])] = 0
        with pytest.raises(fu.FuError) as ei:
            eng.set_topology(link_up=up)
        assert ei.value.code == -1
        assert f"fu_pair_set_topology: link_up differs between slot {min(5, rev[5])} and its reverse" in str(ei.value)
        assert eng.topology_stats == (g.n, g.E) and eng.slot_live().all()  # the refused call changed nothing
        assert L.lib.fu_pair_get_topology_stats(eng._h, None) == -1
        assert L.lib.fu_pair_get_slot_live(eng._h, None) == -1


def _cli_error(argv, capsys):
    from fu.__main__ import main

    with pytest.raises(SystemExit) as ex:
        main(argv)
    assert ex.value.code == 2
    return capsys.readouterr().err


def test_cli_errors(capsys):
    base = ["bench-graph", "er:n=200,m=800", "--rounds", "4"]
    assert "--pair-churn needs" in _cli_error(base + ["--pair-churn", "0.1"], capsys)
    assert "--pair-churn needs" in _cli_error(base + ["--pair-churn", "0.1", "--loss", "0.1"], capsys)
    for f in ("-0.1", "1.0", "1.5", "nan"):
        assert "--pair-churn must be in [0, 1)" in _cli_error(base + ["--pairs", "--pair-churn", f], capsys), f
    assert "exclusive" in _cli_error(base + ["--pairs", "--churn", "0.1"], capsys)


def test_cli_runs_the_topology_call_between_the_halves(capsys, monkeypatch):
    """--pairs --pair-churn reaches the engine (a stand-in here: no GPU): half of the rounds, the
    topology of the --churn stream, the rest; alive= follows pairs=."""
    import fu.__main__ as cli

    calls = []

    class Stand:
        stats = (7, 0)
        loss_stats = (2, 1, 4)

        def __init__(self, g, v, seed=0, device=0):
            self.n = g.n

        def set_loss(self, p, seed=0):
            calls.append(("loss", p, seed))

        def run_timed(self, rounds):
            calls.append(("run", rounds))
            return 1.0

        def set_topology(self, alive=None, link_up=None):
            calls.append(("topology", np.asarray(alive).copy()))
            self.alive = int(np.count_nonzero(alive))

        @property
        def topology_stats(self):
            return (self.alive, 0)

        def set_targets(self, t):
            calls.append(("targets", np.asarray(t).copy()))

        def max_err(self):
            return 0.5

    monkeypatch.setattr(cli, "PairwiseSync", Stand)
    monkeypatch.setattr(cli, "PairwiseSyncBatch", Stand)
    spec = ["bench-graph", "er:n=200,m=800", "--rounds", "9", "--pairs"]
    assert cli.main(spec + ["--pair-churn", "0.25", "--churn-seed", "3"]) == 0
    line = capsys.readouterr().out.strip()
    dead = fu.uniform_values(200, seed=3, lo=0.0, hi=1.0) < 0.25
    assert [c[0] for c in calls] == ["run", "topology", "run", "targets"]
    assert calls[0][1] == 4 and calls[2][1] == 5
    assert np.array_equal(calls[1][1] != 0, ~dead) and 0 < dead.sum() < 200
    g = fu.Graph.from_spec("er:n=200,m=800", seed=1)  # --seed defaults to 1
    assert np.array_equal(calls[3][1], fu.churn_targets(g, fu.uniform_values(200, seed=0), ~dead))
    assert line.endswith(f" pairs=7 alive={200 - int(dead.sum())}")
    calls.clear()
    assert cli.main(spec + ["--pair-churn", "0.25", "--loss", "0.1", "--pair-columns", "2"]) == 0
    line = capsys.readouterr().out.strip()
    assert [c[0] for c in calls] == ["loss", "run", "topology", "run", "targets"] and calls[4][1].shape == (200, 2)
    assert " pairs=7 alive=" in line and line.endswith(" lost=3 columns=2")
    calls.clear()
    assert cli.main(spec) == 0
    assert "alive=" not in capsys.readouterr().out and [c[0] for c in calls] == ["run", "targets"]
