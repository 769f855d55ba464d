"""CPU: the reference fixtures of operator-ordered maintenance of the turbine (tests/golden/operator_turbine/,
tools/make_turbine_maintenance_golden.py) are well formed and not vacuous.  This is the coverage gate of the turbine catalog: every
catalogued type occurs in some fixture with the reference's success and every such call passed the closure check on the live reference
(what it writes outside the carried state is never read by a step); every type that is not offered is recorded with the difference the
check saw; each conditional handler is seen on both sides of its condition, each cap and floor from both sides.  No library, no compute."""
import os

import numpy as np
import pytest

from turbine_maintenance_golden import (ACTIONS, KINDS, NOT_OFFERED, REFUSED_FIXTURE, REPLAYED, THRUST, TurbineGolden, order_succeeds,
                                        turbine_fixture_names)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = REPLAYED + (REFUSED_FIXTURE,)
# catalogued handlers that move no carried member whatever the state
READ_ONLY = {("turbine", "turbine_performance_test"), ("turbine", "thermal_stress_analysis"), ("bearing", "turbine_bearing_inspection"),
             ("bearing", "bearing_clearance_check"), ("bearing", "bearing_alignment")}


def _changed(g, j):
    b, a = g.op_before[j], g.op_after[j]
    return ~((b == a) | (np.isnan(b) & np.isnan(a)))


def _col(g, label):
    return g.op_labels.index(label)


@pytest.fixture(scope="module")
def goldens():
    return {n: TurbineGolden(n) for n in NAMES}


def _calls(goldens, kind, action, names=REPLAYED):
    return [(goldens[n], j, o) for n in names for j, o in enumerate(goldens[n].ops) if goldens[n].kind_name(o) == (kind, action)]


def test_fixtures_live_in_their_own_directory():
    """tests/golden/*.npz is what every replay test parametrises over; the other operator fixtures have directories of their own"""
    from component_maintenance_golden import component_fixture_names
    from golden_util import fixture_names
    from operator_maintenance_golden import operator_fixture_names
    assert set(turbine_fixture_names()) == set(NAMES)
    for other in (fixture_names(), operator_fixture_names(), component_fixture_names()):
        assert not [n for n in other if n.startswith("ot")]
    for n in NAMES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "operator_turbine", n + ".npz")) <= 360 * 1024, n


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_well_formed_and_its_calls_act_where_they_should(goldens, name):
    g = goldens[name]
    K = len(g.ops)
    assert K > 0 and g.op_before.shape == g.op_after.shape == (K, len(g.op_labels)) and len(g.op_expect_change) == len(g.op_closed) == K
    labels = [c[2] for c in g.cols]
    assert g.op_labels == [lab for lab in labels if lab.startswith(("turb.", "tstg."))] and len(g.op_labels) == 38 + 70
    assert not g.done.any()
    for j, o in enumerate(g.ops):
        changed = _changed(g, j)
        assert changed.any() == bool(g.op_expect_change[j]), (name, j, o, [g.op_labels[q] for q in np.nonzero(changed)[0]])
        kind, action = g.kind_name(o)
        assert 0 <= o.step and o.step + int(g.meta["closure_steps"]) <= g.T
        assert g.op_names[j] == action or kind is None
        if kind is None:
            # outside the catalog: an unknown type (success 0, nothing moves) or one that is not offered (only in its own fixture)
            if (o.called, g.op_names[j]) in NOT_OFFERED:
                assert name == REFUSED_FIXTURE
            else:
                assert not o.success and not changed.any(), (name, j, o)
            continue
        assert kind == o.called and name != REFUSED_FIXTURE
        assert o.success == order_succeeds(kind, action, o.unit), (name, j, o)
        assert g.op_closed[j] == 1, (name, j, o)
        if not o.success or (kind, action) in READ_ONLY:
            assert not changed.any(), (name, j, o)
        # only what the order may touch moves: turb for the turbine, a bearing and the lubrication system; a stage's own three columns
        moved = {g.op_labels[q] for q in np.nonzero(changed)[0]}
        if kind == "stage":
            assert moved <= {"tstg.stage_%s[%d]" % (m, o.unit) for m in ("deposit_thickness", "blade_wear_factor", "efficiency_degradation")}, (name, j, moved)
        elif kind == "bearing":
            assert moved <= {"turb.bearing_metal_temp[%d]" % o.unit, "turb.bearing_wear_factor[%d]" % o.unit}, (name, j, moved)
        else:
            assert all(m.startswith("turb.") for m in moved), (name, j, moved)
    # the recorded trajectory continues from the calls: the state recorded for step t is what the first call at t was made on, and a
    # later call between the same two steps starts from the one before it
    for j, o in enumerate(g.ops):
        if j and g.ops[j - 1].step == o.step:
            want = g.op_after[j - 1]
        else:
            row = g.state[list(g.state_steps).index(o.step)]
            want = np.array([row[labels.index(m)] for m in g.op_labels])
            for lab, v in g.pokes.get(o.step, []):          # pokes of this step come before its calls
                (q,) = [q for q, c in enumerate(g.cols) if c[3] == lab]
                if labels[q] in g.op_labels:
                    want[g.op_labels.index(labels[q])] = v
        assert np.array_equal(want, g.op_before[j], equal_nan=True), (name, j, o)
    assert set(g.meta["refused"]) == {"%s:%s" % k for k in NOT_OFFERED}


def test_every_catalog_action_occurs_with_the_expected_success_and_is_closed(goldens):
    seen = {}
    for n in REPLAYED:
        g = goldens[n]
        for j, o in enumerate(g.ops):
            if o.action < len(ACTIONS) and o.success:
                seen.setdefault(ACTIONS[o.action], []).append(int(g.op_closed[j]))
    missing = [a for a in ACTIONS if a not in seen]
    assert not missing, "catalogued actions no fixture carries out: %s" % missing
    assert all(all(v) for v in seen.values()), [a for a, v in seen.items() if not all(v)]
    assert all(o.action <= len(ACTIONS) for g in goldens.values() for o in g.ops)
    # every candidate on a degraded turbine (ot1 / ot2) and on the as-built one (ot3)
    for kind, action in ACTIONS:
        assert [1 for g, j, o in _calls(goldens, kind, action, ("ot1_degraded_turbine", "ot2_stages")) if o.success], (kind, action)
        assert [1 for g, j, o in _calls(goldens, kind, action, ("ot3_as_built",)) if o.success], (kind, action)
    # every bearing and every stage at least once, with a call that acts
    assert {o.unit for n in REPLAYED for j, o in enumerate(goldens[n].ops) if o.called == "bearing" and o.success and goldens[n].op_expect_change[j]} == set(range(4))
    assert {o.unit for n in REPLAYED for j, o in enumerate(goldens[n].ops) if o.called == "stage" and o.success and goldens[n].op_expect_change[j]} == set(range(14))
    # unknown types on every kind; a bearing and a stage that do not exist
    unknown = {o.called for n in REPLAYED for j, o in enumerate(goldens[n].ops) if o.action == len(ACTIONS)}
    assert unknown == set(KINDS)
    assert [1 for o in goldens["ot2_stages"].ops if o.called == "stage" and o.unit == 14 and not o.success]
    assert [1 for o in goldens["ot2_stages"].ops if o.called == "bearing" and o.unit == 4 and not o.success]


def test_what_is_not_offered_is_recorded_with_what_the_check_saw(goldens):
    g = goldens[REFUSED_FIXTURE]
    called = {(o.called, g.op_names[j]) for j, o in enumerate(g.ops)}
    assert called == set(NOT_OFFERED)
    assert all(o.action == len(ACTIONS) for o in g.ops) and not g.op_closed.any()
    for kind, action in NOT_OFFERED:
        why = g.meta["refused"]["%s:%s" % (kind, action)]
        assert "after step" in why and "tstg.stage_blade_wear_factor" in why, why
        # on a degraded unit (the call moves carried state) and on an as-built one
        moves = [bool(_changed(g, j).any()) for j, o in enumerate(g.ops) if (o.called, g.op_names[j]) == (kind, action)]
        assert len(moves) >= 2 and any(moves)


def test_conditional_handlers_are_seen_on_both_sides(goldens):
    g = goldens["ot1_degraded_turbine"]
    B, A = g.op_before, g.op_after
    by = lambda kind, action: [(j, o) for j, o in enumerate(g.ops) if g.kind_name(o) == (kind, action)]
    # the protection test with and without an active trip: only the former resets the latch and the timers
    tests = by("turbine", "turbine_protection_test")
    active = [bool(B[j, _col(g, "turb.trip_active")]) for j, _o in tests]
    assert True in active and False in active
    for (j, _o), act in zip(tests, active):
        assert B[j, _col(g, "turb.trip_latched_mask")] != 0
        if act:
            assert all(A[j, _col(g, m)] == 0 for m in ("turb.trip_active", "turb.trip_latched_mask", "turb.timer_overspeed", "turb.timer_vibration", "turb.timer_bearing_temp"))
        else:
            assert not _changed(g, j).any()
    assert any(act and B[j, _col(g, "turb.timer_vibration")] > 0 for (j, _o), act in zip(tests, active))
    # the thrust adjustment on the thrust bearing and on a journal bearing
    thrust = by("bearing", "thrust_bearing_adjustment")
    assert {o.unit for _j, o in thrust} == {0, 1, 2, 3}
    assert all(o.success == (o.unit == THRUST) for _j, o in thrust) and all(o.success or not _changed(g, j).any() for j, o in thrust)

    def sides(kind, action, label, cut, before=True):
        """the member `label` of the calls (kind, action): below and above `cut`"""
        src = B if before else A
        v = [src[j, _col(g, label % o.unit if "%d" in label else label)] for j, o in by(kind, action) if o.success]
        return any(x < cut for x in v) and any(x > cut for x in v)
    # caps and floors from both sides: max(80, T - d) on the bearings, min(T, 90) of a replacement
    assert sides("turbine", "routine_maintenance", "turb.bearing_metal_temp[0]", 80.5)
    assert sides("bearing", "thrust_bearing_adjustment", "turb.bearing_metal_temp[%d]", 85.0)
    assert sides("bearing", "turbine_oil_change", "turb.bearing_metal_temp[%d]", 82.0) or sides("bearing", "routine_maintenance", "turb.bearing_metal_temp[%d]", 81.0) \
        or sides("bearing", "thrust_bearing_adjustment", "turb.bearing_metal_temp[%d]", 85.0)
    assert sides("bearing", "turbine_bearing_replacement", "turb.bearing_metal_temp[%d]", 90.0)
    # the oil: min(5, 0.6 c) and max(1, c) of the filter replacement; min(1, e + d) of the effectiveness; max(45, T - d) of the oil temperature
    c = [B[j, _col(g, "turb.lub_oil_contamination")] for j, _o in by("lubrication", "oil_filter_replacement")]
    assert any(0.6 * x > 5.0 for x in c) and any(0.6 * x < 5.0 and x - 0.6 * x > 1.0 for x in c) and any(x - 0.6 * x < 1.0 for x in c)
    assert sides("lubrication", "turbine_oil_change", "turb.lub_effectiveness", 0.85) and sides("lubrication", "turbine_oil_change", "turb.lub_oil_temperature", 50.0)
    assert sides("turbine", "turbine_system_optimization", "turb.lub_effectiveness", 0.95)
    w = [B[j, _col(g, "turb.lub_wear[4]")] for j, _o in by("lubrication", "oil_cooler_cleaning")]
    assert any(x > 5.0 for x in w) and any(0.0 < x < 5.0 for x in w)
    r = by("lubrication", "routine_maintenance")
    assert any(0.0 < B[j, _col(g, "turb.lub_wear[3]")] < 0.5 for j, _o in r) and any(B[j, _col(g, "turb.lub_wear[0]")] > 0.5 for j, _o in r)
    assert any(1.0 < B[j, _col(g, "turb.lub_oil_contamination")] < 1.5 for j, _o in r) and any(B[j, _col(g, "turb.lub_oil_contamination")] > 1.5 for j, _o in r)
    # the top-off adds nothing at an oil level of 100: a clean oil is floored, a dirty one keeps its values
    top = by("lubrication", "turbine_oil_top_off")
    assert {bool(g.op_expect_change[j]) for j, _o in top} == {True, False}
    # the vibration analysis moves the thermal bow by the factor 0.7, twice between the same two steps
    v = by("turbine", "vibration_analysis")
    twice = [j for (j, o), (j2, o2) in zip(v, v[1:]) if o.step == o2.step]
    assert twice and all(A[j, _col(g, "turb.thermal_bow")] == B[j, _col(g, "turb.thermal_bow")] * 0.7 for j, _o in v)
    # two calls on one stage between the same two steps
    s = goldens["ot2_stages"]
    assert [j for j in range(1, len(s.ops)) if (s.ops[j].step, s.ops[j].unit, s.ops[j].called) == (s.ops[j - 1].step, s.ops[j - 1].unit, "stage")]


def test_ot4_runs_beside_the_automatic_pump_maintenance(goldens):
    g = goldens["ot4_long_run"]
    labels = [c[2] for c in g.cols]
    performed = g.state[:, labels.index("maint.maintenance_actions_performed")]
    assert performed[-1] >= 1, "the automatic pump maintenance never acts in this run"
    assert {o.called for o in g.ops} == set(KINDS) and g.T >= 48
    assert all(o.success for o in g.ops) and max(o.step for o in g.ops) + 20 <= g.T
