"""CPU: the scattered-call fixtures of the turbine (tests/golden/operator_calls/turbine/, tools/make_scattered_turbine_calls_golden.py) are
well formed and cover what they are for: every catalogued type, every bearing and stage, the written-out edge cases (members exactly on a
cap or floor and on both sides of it, NaN members, the protection test with and without a trip, the thrust adjustment on every bearing),
and the float32 repeat of every call.  No library, no compute calls."""
import os

import numpy as np
import pytest

from turbine_maintenance_golden import ACTIONS, THRUST, UNITS, ScatteredTurbineCalls, order_succeeds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sc():
    return ScatteredTurbineCalls()


def test_files_are_small_and_say_how_they_were_drawn(sc):
    assert len(sc.names) >= 2 and len(sc) >= 250
    for n in sc.names:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "operator_calls", "turbine", n + ".npz")) <= 360 * 1024, n
    for m in sc.metas:
        assert isinstance(m["seed"], int) and m["ranges"] and m["steps_before"] >= 1 and 0 < m["else_within"] < 0.1
        assert m["dropped"] == [] and m["not_poked"] == []
    assert len(sc.written) == len(sc.calls) == len(sc.before) == len(sc.expect_change)
    assert sc.labels == [c[2] for c in __import__("nuclear_sim_amd.schema", fromlist=["SCHEMA"]).SCHEMA.columns() if c[2].startswith(("turb.", "tstg."))]


def test_every_call_is_consistent_with_the_catalog(sc):
    for j, c in enumerate(sc.calls):
        kind, name = ACTIONS[c.action]
        assert kind == c.called and 0 <= c.unit < UNITS[kind]
        assert c.success == order_succeeds(kind, name, c.unit), (j, c)
        changed = sc.changed(j)
        assert changed.any() == bool(sc.expect_change[j])
        assert c.success or not (changed.any() or sc.changed(j, f32=True).any())
        moved = {sc.labels[q] for q in np.nonzero(changed | sc.changed(j, f32=True))[0]}
        if kind == "stage":
            assert moved <= {"tstg.stage_%s[%d]" % (m, c.unit) for m in ("deposit_thickness", "blade_wear_factor", "efficiency_degradation")}, (j, c, moved)
        elif kind == "bearing":
            assert moved <= {"turb.bearing_metal_temp[%d]" % c.unit, "turb.bearing_wear_factor[%d]" % c.unit}, (j, c, moved)
        else:
            assert all(m.startswith("turb.") for m in moved), (j, c, moved)
        # the float32 repeat starts from the rounded values
        real = np.array([k == "f64" for k in sc.kinds])
        assert np.array_equal(sc.before32[j][real], sc.before[j][real].astype(np.float32).astype(np.float64), equal_nan=True)


def test_coverage_of_types_units_and_edges(sc):
    seen = {}
    for j, c in enumerate(sc.calls):
        seen.setdefault(ACTIONS[c.action], set()).add(c.unit)
    assert set(seen) == set(ACTIONS)
    assert all(seen[("bearing", a)] == {0, 1, 2, 3} for k, a in ACTIONS if k == "bearing")
    assert seen[("stage", "overhaul")] == set(range(14)) and seen[("stage", "blade_replacement")] == set(range(14))
    by = lambda kind, name: [j for j, c in enumerate(sc.calls) if ACTIONS[c.action] == (kind, name)]
    col = sc.col
    # the thrust adjustment: refused on the journal bearings, carried out on the thrust bearing with the floor seen from both sides and on it
    t = by("bearing", "thrust_bearing_adjustment")
    assert {sc.calls[j].unit for j in t if not sc.calls[j].success} == {0, 1, 3}
    temps = [sc.before[j, col["turb.bearing_metal_temp[%d]" % THRUST]] for j in t if sc.calls[j].success]
    assert 85.0 in temps and any(x < 85.0 for x in temps) and any(x > 85.0 for x in temps) and any(np.isnan(x) for x in temps)
    # the protection test with and without an active trip
    p = by("turbine", "turbine_protection_test")
    assert {int(sc.before[j, col["turb.trip_active"]]) for j in p} == {0, 1}
    for j in p:
        if sc.before[j, col["turb.trip_active"]]:
            assert all(sc.after[j, col[m]] == 0 for m in ("turb.trip_active", "turb.trip_latched_mask", "turb.timer_overspeed", "turb.timer_vibration", "turb.timer_bearing_temp"))
        else:
            assert not sc.changed(j).any()
    # members exactly on a cap or floor
    on = lambda kind, name, label, v: any(sc.before[j, col[label]] == v for j in by(kind, name))
    assert on("turbine", "turbine_system_optimization", "turb.lub_effectiveness", 0.95) and on("lubrication", "turbine_oil_change", "turb.lub_effectiveness", 0.85)
    assert on("lubrication", "turbine_oil_change", "turb.lub_oil_temperature", 50.0) and on("lubrication", "oil_cooler_cleaning", "turb.lub_wear[4]", 5.0)
    assert on("lubrication", "oil_filter_replacement", "turb.lub_oil_contamination", 2.5) and on("lubrication", "lubrication_system_test", "turb.lub_effectiveness", 0.9)
    assert on("bearing", "turbine_bearing_replacement", "turb.bearing_metal_temp[0]", 90.0) and on("turbine", "routine_maintenance", "turb.bearing_metal_temp[0]", 80.5)
    assert on("lubrication", "turbine_oil_top_off", "turb.lub_oil_contamination", 1.0) and on("lubrication", "routine_maintenance", "turb.lub_wear[0]", 0.5)
    # NaN members, and what Python's min / max make of them
    nan_calls = [j for j in range(len(sc)) if sc.calls[j].explicit and np.isnan(sc.before[j]).any()]
    assert len(nan_calls) >= 10
    j = [j for j in by("lubrication", "oil_filter_replacement") if np.isnan(sc.before[j, col["turb.lub_oil_contamination"]])][0]
    assert sc.after[j, col["turb.lub_oil_contamination"]] == 1.0
    j = [j for j in by("bearing", "turbine_bearing_replacement") if np.isnan(sc.before[j, col["turb.bearing_metal_temp[3]"]])][0]
    assert np.isnan(sc.after[j, col["turb.bearing_metal_temp[3]"]]) and sc.after[j, col["turb.bearing_wear_factor[3]"]] == 1.0
    # the vibration analysis multiplies the thermal bow by 0.7 wherever the vibration stands
    v = by("turbine", "vibration_analysis")
    disp = [sc.before[j, col["turb.vibration_displacement"]] for j in v]
    assert any(x < 50.0 / 3.0 for x in disp) and any(x > 50.0 / 3.0 for x in disp)
    assert all(sc.after[j, col["turb.thermal_bow"]] == sc.before[j, col["turb.thermal_bow"]] * 0.7 or np.isnan(sc.before[j, col["turb.thermal_bow"]]) for j in v)
