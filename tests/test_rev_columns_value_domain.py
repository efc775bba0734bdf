"""The inputs and references of tests/test_rev_columns_value_domain_gpu.py, on the CPU
(rev_columns_vd_cases): the Python rules of the lossy and churn engines, with every message
delivered and everything alive, reproduce the reference's collect-all recordings on the fp64
value domain (so a lossless K-column run must give those bits, and a disagreement on the GPU is
the kernel's alone); the column layouts hold the recordings' inputs where they say; and the
recordings, masks and planted values reach what the GPU cases rely on: -0.0 in estimates and
flows, both infinities and NaN, finite estimates beside NaN ones, lost messages in both heavy
rows, special values on both sides of a chunk edge."""
import numpy as np
import pytest

import fu
import rule_cases
import vd_cases
from parity_util import assert_same_bits
from rev_columns_cases import HEAVY_WIDTHS, chunk_slots, heavy_boundary_graph
from rev_columns_vd_cases import (CA_LAYOUTS, ENGINES, ERR_SPEC, FILL_SEED, HEAVY_LAYOUTS, HEAVY_STOPS, RULE_LAYOUTS,
                                  alive_in_round, error_case, fillers, fixture, graph, heavy_churn_steps, heavy_columns,
                                  heavy_lossy_stops, layout, planted_column, reference_rounds, stops, vd_columns)
from vd_cases import CA_FAMILIES, RULE_FAMILIES, counts, is_neg_zero


# ------------------------------------------------------------------------------------
# 1. the premise: without loss and with everything alive both rules are the collect-all recordings
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", CA_FAMILIES)
@pytest.mark.parametrize("engine", ENGINES)
def test_lossless_python_rules_equal_the_collect_all_recordings(engine, family):
    d = vd_cases.ca(family)
    assert d.stops == [1, 3, 8, 17]
    per_round = reference_rounds(engine, "ca", family)
    for q, stop in enumerate(d.stops):
        assert_same_bits(per_round[stop - 1][0], d.last_avg[q], (engine, family, stop, "estimates"))
        assert_same_bits(per_round[stop - 1][1], d.flows[q], (engine, family, stop, "flows"))


@pytest.mark.parametrize("family", RULE_FAMILIES)
@pytest.mark.parametrize("engine", ENGINES)
def test_python_rules_equal_the_rule_recordings_round_by_round(engine, family):
    """The per-round runs that the error reduction cases take their estimates from pass through
    the recordings at every stop."""
    d = fixture(engine, family)
    per_round = reference_rounds(engine, engine, family)
    assert len(per_round) == d.stops[-1]
    for q, stop in enumerate(d.stops):
        assert_same_bits(per_round[stop - 1][0], d.last_avg[q], (engine, family, stop, "estimates"))
        assert_same_bits(per_round[stop - 1][1], d.flows[q], (engine, family, stop, "flows"))


# ------------------------------------------------------------------------------------
# 2. the layouts
# ------------------------------------------------------------------------------------
def _check_layout(kind, V, fams, spec):
    n = graph(kind).n
    assert V.shape == (n, len(spec)) and V.dtype == np.float64 and V.flags["C_CONTIGUOUS"]
    assert fams == {c: f for c, f in enumerate(spec) if f is not None}
    for c, f in enumerate(spec):
        want = fu.uniform_values(n, seed=FILL_SEED + c) if f is None else fixture(kind, f).values
        assert_same_bits(np.ascontiguousarray(V[:, c]), want, (kind, c, f))


@pytest.mark.parametrize("place", ["first", "last"])
@pytest.mark.parametrize("K", [2, 3, 5, 16])
@pytest.mark.parametrize("kind", ["ca", "lossy", "churn"])
def test_vd_columns_puts_the_recordings_where_asked(kind, K, place):
    fams = CA_FAMILIES if kind == "ca" else RULE_FAMILIES
    if K < len(fams):
        with pytest.raises(AssertionError):
            vd_columns(kind, K, place)
        return
    m = len(fams)
    spec = fams + (None,) * (K - m) if place == "first" else (None,) * (K - m) + fams[::-1]
    V, got = vd_columns(kind, K, place)
    _check_layout(kind, V, got, spec)
    if place == "first":
        assert [got[c] for c in range(m)] == list(fams)
    else:
        assert [got[K - 1 - c] for c in range(m)] == list(fams)
    # the filler columns differ from each other and from the recordings
    assert len({V[:, c].tobytes() for c in range(K)}) == K


def test_the_lossless_layouts():
    assert CA_LAYOUTS["k5"] == CA_FAMILIES
    assert {CA_LAYOUTS["k2-huge-special"], CA_LAYOUTS["k2-subn-special_off"]} == {("huge", "special"), ("subn", "special_off")}
    assert CA_LAYOUTS["k3"] == ("special", None, "subn")
    k16 = CA_LAYOUTS["k16"]
    assert len(k16) == 16 and k16.count(None) == 1
    fam_cols = [f for f in k16 if f is not None]
    orders = [tuple(fam_cols[q:q + 5]) for q in (0, 5, 10)]
    assert all(sorted(o) == sorted(CA_FAMILIES) for o in orders) and len(set(orders)) == 3
    for name, spec in CA_LAYOUTS.items():
        V, fams = layout("ca", spec)
        _check_layout("ca", V, fams, spec)
    assert sorted(RULE_LAYOUTS.values()) == [(2, "first"), (3, "first"), (16, "first"), (16, "last")]


# ------------------------------------------------------------------------------------
# 3. what the recordings reach
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ca", "lossy", "churn"])
def test_subn_columns_reach_negative_zero(kind):
    d = fixture(kind, "subn")
    assert is_neg_zero(d.last_avg[-1]).any() and is_neg_zero(d.flows[-1]).any()
    assert np.isfinite(d.last_avg).all() and np.isfinite(d.flows).all()


def test_huge_holds_both_infinities_and_then_nan():
    d = vd_cases.ca("huge")
    assert d.stops[1] == 3 and d.stops[-1] == 17
    _, pinf, ninf, _ = counts(d.flows[1])
    assert pinf > 0 and ninf > 0
    assert np.isnan(d.flows[-1]).any() and np.isnan(d.last_avg[-1]).any()


def test_wide_stays_finite():
    d = vd_cases.ca("wide")
    assert np.isfinite(d.last_avg).all() and np.isfinite(d.flows).all()


@pytest.mark.parametrize("kind", ENGINES)
def test_special_columns_hold_nan_beside_finite_estimates(kind):
    a = fixture(kind, "special").last_avg[-1]
    assert np.isnan(a).any() and int(np.isfinite(a).sum()) >= 100


def test_both_heavy_rows_lose_messages():
    """kOwn occurs in the row of three chunks (K = 2) and in the row of 128 + 2 slots (K = 16)."""
    g = graph("lossy")
    assert g.rowptr[1] - g.rowptr[0] == 2101 and g.rowptr[2] - g.rowptr[1] == 130
    lost = ~g.delivered[1:g.stops[-1]]
    for i in (0, 1):
        in_row = lost[:, g.rowptr[i]:g.rowptr[i + 1]]
        assert in_row.any() and not in_row.all(), i
    assert stops("lossy") == g.stops and stops("churn") == graph("churn").stops


@pytest.mark.parametrize("engine", ENGINES)
def test_error_case_inputs(engine):
    """The subn and filler traces are finite and end in +0.0; the special trace is NaN from the
    round the rule first holds a NaN (among the alive nodes) and in no earlier round; the targets
    are finite."""
    V, target, want, a_rounds = error_case(engine)
    assert ERR_SPEC == ("special", None, "subn") and V.shape[1] == 3 and np.isfinite(target).all()
    assert np.isfinite(want[:, 1:]).all() and (want[:, 1:] >= 0.0).all()
    assert_same_bits(want[-1, 1:], np.zeros(2), "the last check is +0.0")
    assert (want[:-1, 1] > 0.0).all() and want[:-1, 2].any()
    has_nan = []
    for r in range(len(want)):
        on = alive_in_round(r) if engine == "churn" else slice(None)
        has_nan.append(bool(np.isnan(a_rounds[r][on, 0]).any()))
    first = has_nan.index(True)
    assert all(has_nan[first:]) and [bool(x) for x in np.isnan(want[:, 0])] == has_nan
    assert not np.isnan(a_rounds[:, :, 1:]).any()


# ------------------------------------------------------------------------------------
# 4. special values at the chunk edges of each K
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", HEAVY_WIDTHS)
def test_planted_neighbours_sit_where_claimed(K):
    g, rows = heavy_boundary_graph(K)
    ce = chunk_slots(K)
    v, claims = planted_column(K)
    many = {h: d for d, h in rows.items() if d > ce}
    assert len(many) >= 2 and ce + 1 in many.values() and 2 * ce + 1 in many.values()
    by_row = {h: {} for h in many}
    for h, pos, x in claims:
        assert_same_bits(v[g.col[g.rowptr[h] + pos]:][:1], np.array([x]), (K, h, pos))
        by_row[h][pos] = x
    for h, d in many.items():
        assert by_row[h][ce - 1] == np.inf and np.isnan(by_row[h][d - 1])
        if d - 1 != ce:
            assert is_neg_zero(np.array([by_row[h][ce]]))[0]
    planted = ~np.isfinite(v) | is_neg_zero(v)
    assert int(planted.sum()) == len({int(g.col[g.rowptr[h] + pos]) for h, pos, _ in claims})
    assert_same_bits(v[~planted], fu.uniform_values(g.n, seed=FILL_SEED + 50)[~planted])


def test_the_heavy_layouts():
    """subn, huge and the planted column last at every K of HEAVY_WIDTHS; K = 2 takes two handles."""
    assert sorted({K for K, _ in HEAVY_LAYOUTS.values()}) == sorted(HEAVY_WIDTHS)
    for K in HEAVY_WIDTHS:
        specs = [spec for k, spec in HEAVY_LAYOUTS.values() if k == K]
        assert all(len(s) == K and s[-1] == "planted" for s in specs)
        assert {f for s in specs for f in s if f is not None} == {"subn", "huge", "planted"}
    for name in HEAVY_LAYOUTS:
        g, V, spec = heavy_columns(name)
        assert V.shape == (g.n, len(spec)) and V.flags["C_CONTIGUOUS"]
        assert_same_bits(np.ascontiguousarray(V[:, -1]), planted_column(len(spec))[0])


@pytest.mark.parametrize("name", sorted(HEAVY_LAYOUTS))
def test_planted_values_reach_the_heavy_rows_and_stay_in_their_column(name):
    """On the Python rules alone: after two rounds the planted column's estimate of every row of
    more than one chunk is not finite; the subn and filler columns are finite after every step and
    stop."""
    K, spec = HEAVY_LAYOUTS[name]
    g, rows = heavy_boundary_graph(K)
    many = [h for d, h in rows.items() if d > chunk_slots(K)]
    p = spec.index("planted")
    quiet = [c for c, f in enumerate(spec) if f in (None, "subn")]
    steps = heavy_churn_steps(name)
    assert not np.isfinite(steps[0].a[many, p]).any()  # the script starts with run(2)
    lossy = heavy_lossy_stops(name)
    assert HEAVY_STOPS[1] == 2 and not np.isfinite(lossy[2][0][many, p]).any()
    for s in steps:
        assert np.isfinite(s.a[:, quiet]).all() and np.isfinite(s.f[:, quiet]).all()
    for stop in HEAVY_STOPS:
        assert np.isfinite(lossy[stop][0][:, quiet]).all() and np.isfinite(lossy[stop][1][:, quiet]).all()
    if "subn" in spec:
        c = spec.index("subn")
        assert is_neg_zero(steps[0].a[:, c]).any() and is_neg_zero(lossy[2][0][:, c]).any()
    if "huge" in spec:
        c = spec.index("huge")
        assert not np.isfinite(steps[-1].f[:, c]).all() and not np.isfinite(lossy[HEAVY_STOPS[-1]][1][:, c]).all()
    assert fillers(spec) == [c for c, f in enumerate(spec) if f is None]
