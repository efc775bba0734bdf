"""The pairwise engine's loss entry points without a GPU: the four symbols, argument errors (all
checked before any HIP call), the host restatement of the loss decision (fu_pair_lost) against
Python ints, and the command line."""
import inspect

import numpy as np
import pytest

import fu
from fu import _lib as L
from pair_cases import rr256_d8
from pair_loss_cases import pair_lost_np, pair_lost_py

LOSS_SYMBOLS = ["fu_pair_set_loss", "fu_pair_set_link_mask", "fu_pair_get_loss_stats", "fu_pair_lost"]


def test_the_four_symbols_load():
    for s in LOSS_SYMBOLS:
        assert hasattr(L.lib, s), s
        assert s in L.EXPORTED
    assert L.lib.fu_version() == 2
    assert hasattr(fu, "pair_lost") and "pair_lost" in fu.__all__
    kw = inspect.signature(fu.PairwiseSync.__init__).parameters
    assert kw["loss"].default == 0.0 and kw["loss_seed"].default == 0 and kw["link_mask"].default is None
    for name in ("set_loss", "set_link_mask", "loss_stats"):
        assert hasattr(fu.PairwiseSync, name), name


def test_bad_arguments_come_before_any_hip_call():
    """A NULL handle and a p outside [0, 1] (NaN included) are FU_ERR_ARG on a host without a GPU."""
    out = np.zeros(3, dtype=np.int64)
    assert L.lib.fu_pair_set_loss(None, 0.5, 1) == -1
    assert L.lib.fu_pair_set_link_mask(None, None) == -1
    assert L.lib.fu_pair_set_link_mask(None, L.ptr(np.zeros(4, dtype=np.uint8))) == -1
    assert L.lib.fu_pair_get_loss_stats(None, L.ptr(out)) == -1
    assert "fu_pair_get_loss_stats" in L.last_error()
    one = np.zeros(8, dtype=np.uint8)
    for p in (-0.1, 1.5, float("nan")):
        assert L.lib.fu_pair_lost(1, 0, 0, 8, p, L.ptr(one)) == -1, p
        assert "fu_pair_lost" in L.last_error()
    assert L.lib.fu_pair_lost(1, -1, 0, 8, 0.5, L.ptr(one)) == -1  # round < 0
    assert L.lib.fu_pair_lost(1, 0, -1, 8, 0.5, L.ptr(one)) == -1  # first < 0
    assert L.lib.fu_pair_lost(1, 0, 0, -1, 0.5, L.ptr(one)) == -1  # count < 0
    assert L.lib.fu_pair_lost(1, 0, 0, 8, 0.5, None) == -1
    assert L.lib.fu_pair_lost(1, 0, 0, 0, 0.5, None) == 0  # nothing asked for
    assert L.lib.fu_pair_lost(1, 0, 2 ** 63 - 4, 8, 0.5, L.ptr(one)) == -1  # first + count past int64
    assert L.lib.fu_pair_lost(1, 0, 2 ** 63 - 9, 8, 0.5, L.ptr(one)) == 0
    with pytest.raises(fu.FuError) as ei:
        fu.pair_lost(1, 0, 0, 8, 1.5)
    assert ei.value.code == -1


@pytest.mark.gpu
def test_bad_p_and_bad_masks_on_a_live_handle(monkeypatch):
    g = rr256_d8()
    with fu.PairwiseSync(g, np.ones(g.n)) as eng:
        for p in (-0.1, 1.5, float("nan")):
            with pytest.raises(fu.FuError) as ei:
                eng.set_loss(p)
            assert ei.value.code == -1
        assert L.lib.fu_pair_get_loss_stats(eng._h, None) == -1
        with pytest.raises(ValueError):
            eng.set_link_mask(np.zeros(g.E + 1, dtype=np.uint8))
        with pytest.raises(ValueError):
            eng.set_link_mask(np.zeros(g.E))  # a float mask
        eng.set_link_mask(np.zeros(g.E, dtype=bool))
        eng.set_link_mask(None)
        assert eng.loss_stats == (0, 0, 0)
    closed = []
    real_close = fu.PairwiseSync.close
    monkeypatch.setattr(fu.PairwiseSync, "close", lambda self: (closed.append(self._h is not None), real_close(self)))
    for p in (-0.1, 1.5, float("nan")):
        with pytest.raises(fu.FuError):
            fu.PairwiseSync(g, np.ones(g.n), loss=p)
    with pytest.raises(ValueError):
        fu.PairwiseSync(g, np.ones(g.n), link_mask=np.zeros(3, dtype=np.uint8))
    assert closed.count(True) == 4  # the constructor closed the handle it had opened, each time


@pytest.mark.parametrize("r", [0, 1, 2 ** 31])
def test_pair_lost_equals_python_ints(r):
    E = rr256_d8().E
    for seed in (0, 5, 0xFEDCBA9876543210):
        for p in (0.0, 0.1, 0.5, 1.0):
            got = fu.pair_lost(seed, r, 0, E, p)
            assert got.dtype == np.uint8 and got.shape == (E,)
            assert got.tolist() == pair_lost_py(seed, r, 0, E, p), (seed, p)
            assert np.array_equal(got.astype(bool), pair_lost_np(seed, r, E, p)), (seed, p)
            if p == 0.0:
                assert not got.any()
            if p == 1.0:
                assert got.all()
    # a window of the same round, and the rate
    assert fu.pair_lost(5, r, 100, 50, 0.5).tolist() == fu.pair_lost(5, r, 0, E, 0.5)[100:150].tolist()
    assert 0.2 < fu.pair_lost(5, r, 0, E, 0.3).mean() < 0.4


def test_the_loss_stream_is_not_the_matching_stream():
    """The loss key is splitmix_at(~seed, r), the matching's splitmix_at(seed, r): with one number
    for both seeds the decisions are those of the complement, not of the number itself, and
    round 0 is a round like any other."""
    E = rr256_d8().E
    a = fu.pair_lost(11, 3, 0, E, 0.5)
    from lossy_cases import M64, splitmix_at_py

    same_key = [1 if (splitmix_at_py(splitmix_at_py(11, 3), k) >> 11) * 2.0 ** -53 < 0.5 else 0 for k in range(E)]
    comp_key = [1 if (splitmix_at_py(splitmix_at_py(~11 & M64, 3), k) >> 11) * 2.0 ** -53 < 0.5 else 0 for k in range(E)]
    assert a.tolist() == comp_key and a.tolist() != same_key
    assert fu.pair_lost(11, 0, 0, E, 0.5).any()
    assert not np.array_equal(fu.pair_lost(11, 0, 0, E, 0.5), fu.pair_lost(11, 1, 0, E, 0.5))


def _cli_error(argv, capsys):
    from fu.__main__ import main

    with pytest.raises(SystemExit) as ex:
        main(argv)
    assert ex.value.code == 2
    return capsys.readouterr().err


def test_cli_accepts_pairs_with_loss_and_keeps_its_refusals(capsys, monkeypatch):
    """--pairs --loss reaches the engine (a stand-in here: no GPU) with the loss and its seed;
    --churn stays exclusive with either, --columns stays refused with --pairs."""
    import fu.__main__ as cli

    made = {}

    class Stand:
        stats = (7, 0)
        loss_stats = (2, 1, 4)

        def __init__(self, g, v, seed=0, device=0):
            made["seed"] = seed

        def set_loss(self, p, seed=0):
            made["loss"] = (p, seed)

        def run_timed(self, rounds):
            return 1.0

        def set_targets(self, t):
            pass

        def max_err(self):
            return 0.5

    monkeypatch.setattr(cli, "PairwiseSync", Stand)
    assert cli.main(["bench-graph", "er:n=200,m=800", "--rounds", "4", "--pairs", "--pair-seed", "4", "--loss", "0.25",
                     "--loss-seed", "9"]) == 0
    line = capsys.readouterr().out.strip()
    assert made == {"seed": 4, "loss": (0.25, 9)}
    assert line.endswith(" pairs=7 lost=3") and " rounds=4 " in line
    made.clear()
    assert cli.main(["bench-graph", "er:n=200,m=800", "--rounds", "4", "--pairs"]) == 0
    assert capsys.readouterr().out.strip().endswith(" pairs=7") and "loss" not in made
    base = ["bench-graph", "er:n=200,m=800", "--rounds", "4"]
    for extra in (["--loss", "0.1"], ["--pairs"], ["--loss", "0.1", "--pairs"]):
        assert "exclusive" in _cli_error(base + ["--churn", "0.1"] + extra, capsys)
    for extra in (["--pairs"], ["--pairs", "--loss", "0.1"]):
        assert "--columns" in _cli_error(base + ["--columns", "3"] + extra, capsys)
