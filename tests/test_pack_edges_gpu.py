"""The packed estimate table (fu_ca_pack.h: put_code, ld_est, gather_packed; k_stage,
k_hub_flows, kernel 9's staging) where it is least comfortable: estimates planted on the
edges of the code window, and options, resets and readbacks at a packed width. The inputs
are tests/pack_cases.py; tests/test_pack_case_inputs.py holds them to their conditions on the
CPU. Every comparison is by bit pattern against the C oracle.

Rounds are counted as T = rounds run so far (rounds 0 .. T-1), the oracle's count."""
import pytest

import fu
from pack_cases import (CONV_FIRST, CONV_HUB, CONV_MEGA, CONV_ROUNDS, PAIR_CASES, PAIR_STOPS, OracleRun,
                        converging, pair_table)
from parity_util import assert_same_bits

pytestmark = pytest.mark.gpu

KERNELS = ["recon", "stage", "pregather"]
KERNEL_CODE = {"recon": 4, "stage": 8, "pregather": 9}
FU_ERR_STATE = -4


class _Refs:
    """The oracle's (a, f) after T rounds of one case, kept per T; the oracle runs forward
    and starts over for an earlier T that was never asked for."""
    _all = {}

    def __init__(self, g, v):
        self.g, self.v, self.memo, self.run = g, v, {}, OracleRun(g, v)

    @classmethod
    def of(cls, name, g, v):
        if name not in cls._all:
            cls._all[name] = cls(g, v)
        return cls._all[name]

    def after(self, T):
        if T not in self.memo:
            if T < max(self.run.T, 1):
                self.run = OracleRun(self.g, self.v)
            a, f = self.run.after(T)
            a.setflags(write=False)
            f.setflags(write=False)
            self.memo[T] = (a, f)
        return self.memo[T]


def _same(eng, refs, T, what=""):
    assert eng.rounds_done == T, (what, eng.rounds_done, T)
    a_ref, f_ref = refs.after(T)
    assert_same_bits(eng.estimates(), a_ref, f"{what} estimates after {T} rounds")
    assert_same_bits(eng.flows(), f_ref, f"{what} flows after {T} rounds")


def _conv_engine(kind, kernel, pack_every=1):
    cs = converging(kind)
    eng = fu.CollectAll(cs.g, cs.v, kernel=kernel, hub_threshold=CONV_HUB)
    if kind == "rmat":
        eng.set_option("mega_hub", CONV_MEGA)
    eng.set_option("pack_every", pack_every)
    if kernel != "auto":
        assert eng.info()["kernel"] == kernel
    return eng, _Refs.of(kind, cs.g, cs.v)


def _run_to_width_8(eng, kind, settle=2):
    """Rounds up to the first plan of 8 bits (read from the handle, at most CONV_ROUNDS), then
    `settle` more, so both table slots were written under a packed plan. Returns T."""
    T = eng.rounds_done
    step = CONV_FIRST[kind][8] - 4 - T
    while True:
        eng.run(step)
        T += step
        if eng.pack_widths()[2] == 8:
            break
        assert T < CONV_ROUNDS, (T, eng.pack_widths())
        step = 2
    eng.run(settle)
    return T + settle


# ------------------------------------------------------------------------------------
# a. window edges
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("W,centre", PAIR_CASES)
def test_planted_window_edges_bitwise(W, centre, kernel):
    """A constant table with one pair on each offset around the window: the last code
    (esc - 1), the first escape (esc), the keys below the base (an escape only through the
    unsigned wrap of dkey(a) - base) and the offsets that alias to a valid code once narrowed
    to W or 32 bits. Each planted node's partner sits in another tile, so its estimate is
    gathered through the table every round. (Kernel 9 encodes the table like the others but
    gathers the doubles it stages: its cases hold the writer to the bounds of the table and
    the widths, kernels 4 and 8 also read every planted code.)"""
    p = pair_table(W, centre)
    refs = _Refs.of(("pair", W, centre), p.g, p.v)
    eng = fu.CollectAll(p.g, p.v, kernel=kernel)
    eng.set_option("pack_every", 1)
    off = fu.CollectAll(p.g, p.v, kernel=kernel)
    off.set_option("pack", 0)
    assert eng.info()["kernel"] == kernel and off.info()["kernel"] == kernel
    T = 0
    for stop in PAIR_STOPS:
        eng.run(stop - T)
        off.run(stop - T)
        T = stop
        _same(eng, refs, T, "packed")
        _same(off, refs, T, "pack 0")
        if T >= 3:
            assert eng.pack_widths() == p.widths, T
        assert off.pack_widths() == (0, 0, 0), T
    assert eng.info()["kernel"] == kernel
    eng.close()
    off.close()


# ------------------------------------------------------------------------------------
# b. pack off and on at a packed width
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_pack_off_then_on_at_width_8(kernel):
    """pack 0 clears the plan at once and leaves the two table slots to drain: the round after
    still reads the codes of the round before. pack 1 then brings a width back."""
    eng, refs = _conv_engine("er", kernel)
    T = _run_to_width_8(eng, "er")
    _same(eng, refs, T)
    w = eng.pack_widths()
    assert w[2] == 8 and w[0] in (8, 16) and w[1] in (8, 16), w
    eng.set_option("pack", 0)
    w = eng.pack_widths()
    assert w[2] == 0 and w[0] > 0 and w[1] > 0, w  # the plan only: both slots still hold codes
    for k in (1, 2, 3):
        eng.run(1)
        T += 1
        _same(eng, refs, T, f"pack 0, round {k}")
        w = eng.pack_widths()
        assert w[2] == 0 and w[(T - 1) & 1] == 0, (k, w)  # the slot that round T-1 wrote
        if k >= 2:
            assert w == (0, 0, 0), (k, w)
    eng.set_option("pack", 1)
    for k in range(1, 21):
        eng.run(1)
        T += 1
        _same(eng, refs, T, f"pack 1, round {k}")
        if eng.pack_widths()[2]:
            break
    assert eng.pack_widths()[2] in (8, 16), (k, eng.pack_widths())
    for k in range(10):
        eng.run(1)
        T += 1
        _same(eng, refs, T, f"packed again, round {k}")
    w = eng.pack_widths()
    assert all(x in (8, 16) for x in w), w
    eng.close()


# ------------------------------------------------------------------------------------
# c. rebuilds at a packed width
# ------------------------------------------------------------------------------------
def _three_rounds(eng, refs, T, what):
    for k in range(3):
        eng.run(1)
        T += 1
        _same(eng, refs, T, f"{what}, round {k}")
    w = eng.pack_widths()
    assert all(x in (8, 16) for x in w), (what, w)
    return T


def test_tile_rebuilds_at_a_packed_width_recon():
    """Kernel 4: each option that rebuilds the tiles or changes their geometry, one at a time,
    on R-MAT rows of every class while the table is packed."""
    eng, refs = _conv_engine("rmat", "recon")
    T = _run_to_width_8(eng, "rmat")
    _same(eng, refs, T)
    for key, val in (("tile_edges", 512), ("tile_edges", 1024), ("tile_edges", 2048), ("wave_heavy", 0),
                     ("wave_heavy", 1), ("mega_hub", 200), ("mega_hub", CONV_MEGA), ("hub_threshold", 32),
                     ("hub_threshold", CONV_HUB)):
        eng.set_option(key, val)
        if key == "tile_edges":
            assert eng.info()["tile"][0] == val
        T = _three_rounds(eng, refs, T, f"{key} {val}")
    eng.close()


def test_stage_layouts_at_a_packed_width_and_hub_threshold_refused():
    """Kernel 8: every slice layout forced while the table is packed (a layout narrower than
    the table reads it from global memory), and back to the choice by width. hub_threshold
    after the staging exists is refused and changes nothing."""
    eng, refs = _conv_engine("rmat", "stage")
    T = _run_to_width_8(eng, "rmat")
    _same(eng, refs, T)
    for layout in (0, 1, 2, 3, -1):
        eng.set_option("stage_layout", layout)
        T = _three_rounds(eng, refs, T, f"stage_layout {layout}")
    before = eng.info()
    with pytest.raises(fu.FuError, match="hub_threshold must be set before kernel 8") as ei:
        eng.set_option("hub_threshold", 32)
    assert ei.value.code == FU_ERR_STATE
    assert eng.info() == before
    T = _three_rounds(eng, refs, T, "hub_threshold refused")
    eng.close()


def test_lag_switches_at_a_packed_width_pregather():
    """Kernel 9: lag on, off and on again while the table is packed (each switch writes the
    lagged flows and drops the staging), flows read after every round."""
    eng, refs = _conv_engine("rmat", "pregather")
    T = _run_to_width_8(eng, "rmat")
    _same(eng, refs, T)
    for lag in (1, 0, 1, 0):
        eng.set_option("lag", lag)
        T = _three_rounds(eng, refs, T, f"lag {lag}")
    assert eng.info()["kernel"] == "pregather"
    eng.close()


# ------------------------------------------------------------------------------------
# d. reset from a packed width
# ------------------------------------------------------------------------------------
OTHER = {"recon": "stage", "stage": "pregather", "pregather": "recon"}


@pytest.mark.parametrize("kernel", KERNELS)
def test_reset_from_width_8_first_rounds(kernel):
    """fu_reset with 8-bit codes in both slots: round 0 clears the three PackCtl, and rounds
    1 and 2 read doubles, not the codes left behind; then the same with the kernel changed
    between the reset and the first round."""
    eng, refs = _conv_engine("er", kernel)
    for other in (None, OTHER[kernel]):
        T = _run_to_width_8(eng, "er")
        _same(eng, refs, T)
        w = eng.pack_widths()
        assert all(x in (8, 16) for x in w), w
        eng.reset()
        if other:
            eng.set_option("kernel", KERNEL_CODE[other])
        assert eng.info()["kernel"] == (other or kernel) and eng.rounds_done == 0
        T = 0
        for stop in (1, 2, 3, 4, 8, 9):
            eng.run(stop - T)
            T = stop
            _same(eng, refs, T, f"after reset ({other or kernel})")
            if T <= 3:
                assert eng.pack_widths() == (0, 0, 0), T
    eng.close()


# ------------------------------------------------------------------------------------
# e. the width readback runs the plan that is due
# ------------------------------------------------------------------------------------
# 24 rounds from T0 with pack_every 4: from zero state, and across the first plan of 32, 16
# and 8 bits (CONV_FIRST["er"]: 102, 185, 224 with a plan after every round; here the plans
# run from a_T at T = 104, 188 and 224)
@pytest.mark.parametrize("T0", [0, 96, 176, 216])
@pytest.mark.parametrize("kernel", KERNELS)
def test_width_readback_every_round_changes_nothing(kernel, T0):
    """fu_get_pack runs a pending plan itself. One handle is read after every round, one is
    never read before the end: the same bits at 4, 5, 8, 9 and 24 rounds, the same widths at
    the end."""
    read, refs = _conv_engine("er", kernel, pack_every=4)
    quiet, _ = _conv_engine("er", kernel, pack_every=4)
    if T0:
        read.run(T0)
        quiet.run(T0)
    seen = set()
    for k in range(1, 25):
        read.run(1)
        quiet.run(1)
        seen.update(read.pack_widths())
        if k in (4, 5, 8, 9, 24):
            _same(read, refs, T0 + k, "read every round")
            _same(quiet, refs, T0 + k, "never read")
    assert read.pack_widths() == quiet.pack_widths()
    want = {0: {0}, 96: {0, 32}, 176: {32, 16}, 216: {16, 8}}[T0]
    assert seen == want, seen
    read.close()
    quiet.close()


# ------------------------------------------------------------------------------------
# f. first autotune pass at a packed width, then reset
# ------------------------------------------------------------------------------------
def test_first_autotune_pass_at_a_packed_width_then_reset():
    """Calls too short for a pass until the table is packed, then a long call: the first pass
    runs at a packed width, so no winner exists for width 0. fu_reset must then arm a pass
    (as on a new handle) and not keep the packed width's winner at width 0."""
    eng, refs = _conv_engine("er", "auto", pack_every=4)
    assert eng.info()["autotune"] == "pending"
    T = 0
    while not eng.pack_widths()[2]:
        eng.run(16)
        eng.synchronize()
        T += 16
        assert T < CONV_ROUNDS
    info = eng.info()
    assert info["tune_passes"] == 0 and info["autotune"] == "pending" and info["tune_winner_by_width"] == {}
    eng.run(64)
    eng.synchronize()
    T += 64
    info = eng.info()
    winners = info["tune_winner_by_width"]
    assert info["tune_passes"] >= 1 and info["autotune"] == "done", info
    assert 0 not in winners and set(winners) <= {8, 16, 32} and info["tuned_pack_width"] in winners, info
    assert max(info["tune_us_per_round"].values()) > 0, info
    _same(eng, refs, T, "before the reset")
    passes = info["tune_passes"]
    eng.reset()
    assert eng.info()["autotune"] == "pending"
    eng.run(64)
    eng.synchronize()
    info = eng.info()
    assert info["tune_passes"] == passes + 1 and info["autotune"] == "done", info
    assert 0 in info["tune_winner_by_width"] and info["tuned_pack_width"] == 0, info
    _same(eng, refs, 64, "after the reset")
    eng.close()
