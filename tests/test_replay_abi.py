"""The argument checks of the tick replay (fu_replay_*), without a GPU: every one of them runs
before the first HIP call, so each bad input below returns FU_ERR_ARG and leaves its text, with the
offending task or event index, in fu_last_error() on any host, and never writes *out.

The trace is hand-written over the path 0 - 1 - 2 (union degrees 1, 2, 1):
  tick 0, task 0: node 0 fires pairwise with slot 0 (k = 1), message 0;
  tick 1, task 1: node 1 receives message 0 on slot 0, then fires collect-all over both slots,
                  messages out_ids[0..2) = 1, 2."""
import ctypes

import numpy as np
import pytest

import fu
from fu import _lib as L

ARG, HIP = -1, -2
RECV, FIRE_CA, FIRE_PW = 0, 1, 2
UNTOUCHED = 0x5A5A5A5A


def _good():
    return dict(n=3, ticks=2, n_msgs=3,
                rowptr=np.array([0, 1, 3, 4], dtype=np.int64),
                value=np.array([1.0, 2.0, 3.0]),
                tto=np.array([0, 1, 2], dtype=np.int64),
                tasks=np.array([[0, 0, 1], [1, 1, 3]], dtype=np.int32),
                events=np.array([[FIRE_PW, 0, 1, 0], [RECV, 0, 0, 0], [FIRE_CA, 2, 0, 0]], dtype=np.int32),
                out_ids=np.array([1, 2], dtype=np.int32))


def _create(**change):
    """(code, text) of fu_replay_create on the trace above with `change` applied: a scalar or an
    array replaces the field, (index, value) sets one element, None passes a null pointer while
    the counts stay. A handle that does get made (a host with a GPU) is destroyed at once."""
    a = _good()
    counts = dict(n_tasks=len(a["tasks"]), n_events=len(a["events"]), n_out_ids=len(a["out_ids"]))
    for key, val in change.items():
        if isinstance(val, tuple):
            a[key][val[0]] = val[1]
        else:
            a[key] = val
    h = L.vp(UNTOUCHED)
    rc = L.lib.fu_replay_create(a["n"], L.ptr(a["rowptr"]), L.ptr(a["value"]), a["ticks"], L.ptr(a["tto"]),
                                counts["n_tasks"], L.ptr(a["tasks"]), counts["n_events"], L.ptr(a["events"]),
                                counts["n_out_ids"], L.ptr(a["out_ids"]), a["n_msgs"], 0, ctypes.byref(h))
    text = L.last_error()
    if rc == 0:
        L.lib.fu_replay_destroy(h)
    else:
        assert h.value == UNTOUCHED, change
    return rc, text


def test_the_hand_written_trace_passes_every_check():
    """Without a GPU the next thing after the checks is the device probe's error."""
    got = _create()
    if fu.device_count() == 0:
        assert got == (HIP, "fu_replay_create: no HIP device visible")
    else:
        assert got[0] == 0, got


CREATE_ROWS = [
    ("n == 0", dict(n=0), "bad arguments"),
    ("n < 0", dict(n=-3), "bad arguments"),
    ("ticks < 0", dict(ticks=-1), "bad arguments"),
    ("tick_task_off[0] != 0", dict(tto=(0, 1)), "tick_task_off inconsistent"),
    ("tick_task_off[ticks] != n_tasks", dict(tto=(2, 1)), "tick_task_off inconsistent"),
    ("task node too large", dict(tasks=((1, 0), 3)), "bad task 1"),
    ("task node negative", dict(tasks=((0, 0), -1)), "bad task 0"),
    ("task with e < b", dict(tasks=((1, 2), 0)), "bad task 1"),
    ("task past the events", dict(tasks=((1, 2), 4)), "bad task 1"),
    ("RECV slot >= deg", dict(events=((1, 1), 2)), "bad event 1"),
    ("RECV message >= n_msgs", dict(events=((1, 2), 3)), "bad event 1"),
    ("FIRE_CA k > deg", dict(events=((2, 1), 3)), "bad event 2"),
    ("FIRE_CA out ids past n_out_ids", dict(events=((2, 2), 1)), "bad event 2"),
    ("FIRE_PW k <= slot", dict(events=((0, 2), 0)), "bad event 0"),
    ("FIRE_PW message >= n_msgs", dict(events=((0, 3), 3)), "bad event 0"),
    ("unknown event kind", dict(events=((1, 0), 3)), "bad event 1"),
    ("out_id >= n_msgs", dict(out_ids=(1, 3)), "bad out_id"),
    ("out_id negative", dict(out_ids=(0, -1)), "bad out_id"),
    ("null tasks, n_tasks > 0", dict(tasks=None), "bad arguments"),
    ("null events, n_events > 0", dict(events=None), "bad arguments"),
    ("null out_ids, n_out_ids > 0", dict(out_ids=None), "bad arguments"),
    ("null rowptr", dict(rowptr=None), "bad arguments"),
    ("null value", dict(value=None), "bad arguments"),
    ("null tick_task_off", dict(tto=None), "bad arguments"),
]


@pytest.mark.parametrize("what,change,tail", CREATE_ROWS, ids=[r[0] for r in CREATE_ROWS])
def test_create_argument_errors(what, change, tail):
    assert _create(**change) == (ARG, "fu_replay_create: " + tail), what


def test_create_null_out():
    a = _good()
    rc = L.lib.fu_replay_create(3, L.ptr(a["rowptr"]), L.ptr(a["value"]), 2, L.ptr(a["tto"]), 2, L.ptr(a["tasks"]), 3,
                                L.ptr(a["events"]), 2, L.ptr(a["out_ids"]), 3, 0, None)
    assert (rc, L.last_error()) == (ARG, "fu_replay_create: bad arguments")


def test_create_from_null_trace():
    h = L.vp(UNTOUCHED)
    assert L.lib.fu_replay_create_from_trace(None, L.ptr(np.ones(3)), 0, ctypes.byref(h)) == ARG
    assert L.last_error() == "fu_replay_create_from_trace: NULL trace"
    assert h.value == UNTOUCHED


def test_null_handle_calls():
    assert L.lib.fu_replay_destroy(None) == 0
    ms, info = L.f32(0.0), np.zeros(8, dtype=np.int64)
    calls = {"run": (0, 0, None, None), "run_timed": (0, ctypes.byref(ms)), "get": (None, None, None),
             "set_option": (b"persistent", 1), "get_info": (L.ptr(info),)}
    for name, args in calls.items():
        fn = "fu_replay_" + name
        assert getattr(L.lib, fn)(None, *args) == ARG, fn
        assert L.last_error().startswith(fn + ": "), (fn, L.last_error())
