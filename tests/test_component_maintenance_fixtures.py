"""CPU: the reference fixtures of operator-ordered maintenance of steam generators and condenser (tests/golden/operator_components/,
tools/make_component_maintenance_golden.py) are well formed and not vacuous.  This is the coverage gate of the component catalog:
every catalogued action occurs in some fixture with the reference's success, every call that acts by construction changes the reference's
carried state and every other call changes none, and every catalogued action passed the closure check on the live reference (what it
writes outside the carried state is never read by a step).  No library, no compute calls."""
import os

import numpy as np
import pytest

from component_maintenance_golden import ACTIONS, CLEANING_NAMES, KINDS, UNITS, ComponentGolden, component_fixture_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("oc1_steam_generators", "oc2_condenser", "oc3_long_run")
READ_ONLY = {("steam_generator", a) for a in ("tube_bundle_inspection", "tsp_inspection", "tsp_flow_test", "tube_interior_inspection",
                                              "tube_interior_eddy_current_testing", "tube_eddy_current_testing", "primary_chemistry_optimization",
                                              "water_chemistry_adjustment")} | {
    ("condenser", "vacuum_system_test"), ("ejector", "vacuum_ejector_inspection")}


def _changed(g, j):
    b, a = g.op_before[j], g.op_after[j]
    return ~((b == a) | (np.isnan(b) & np.isnan(a)))


def _col(g, label):
    return g.op_labels.index(label)


@pytest.fixture(scope="module")
def goldens():
    return {n: ComponentGolden(n) for n in NAMES}


def test_fixtures_live_in_their_own_directory():
    """tests/golden/*.npz is what every replay test parametrises over, tests/golden/operator/*.npz what the pump tests do"""
    from golden_util import fixture_names
    from operator_maintenance_golden import operator_fixture_names
    assert set(component_fixture_names()) == set(NAMES)
    assert not [n for n in fixture_names() if n.startswith("oc")] and not [n for n in operator_fixture_names() if n.startswith("oc")]
    for n in NAMES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "operator_components", n + ".npz")) <= 360 * 1024, n


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_well_formed_and_its_calls_act_where_they_should(goldens, name):
    g = goldens[name]
    K = len(g.ops)
    assert K > 0 and g.op_before.shape == g.op_after.shape == (K, len(g.op_labels)) and len(g.op_expect_change) == len(g.op_closed) == K
    assert all(lab.startswith(("sg[", "chem[", "cond.", "sec.")) for lab in g.op_labels)
    labels = [c[2] for c in g.cols]
    assert sorted(g.op_labels) == sorted(lab for lab in labels if lab.startswith(("sg[", "chem[", "cond.", "sec.")) and lab in g.op_labels)
    assert len(g.op_labels) >= 3 * 40 + 2 * 11 + 30 + 15
    assert not g.done.any() and g.T >= 48
    for j, o in enumerate(g.ops):
        changed = _changed(g, j)
        assert changed.any() == bool(g.op_expect_change[j]), (name, j, o, [g.op_labels[q] for q in np.nonzero(changed)[0]])
        kind, action = g.kind_name(o)
        assert 0 <= o.step and o.step + int(g.meta["closure_steps"]) <= g.T
        # success: a catalogued action on a unit that exists
        assert o.success == (kind is not None and 0 <= o.unit < UNITS[kind]), (name, j, o)
        if not o.success or (kind, action) in READ_ONLY:
            assert not changed.any(), (name, j, o)
        if o.success:
            assert g.op_closed[j] == 1, (name, j, o)
            # only the sections the action may touch move
            moved = {g.op_labels[q].split(".")[0] for q in np.nonzero(changed)[0]}
            allowed = {"steam_generator": {"sg[%d]" % o.unit}, "steam_generator_system": {"sg[0]", "sg[1]", "sg[2]", "sec"},
                       "condenser": {"cond", "chem[1]"}, "ejector": {"cond"}}[kind]
            assert moved <= allowed, (name, j, o, moved)
        if o.sg_index >= 0:
            assert o.called == "steam_generator_system" and (kind in (None, "steam_generator"))
        else:
            assert kind in (None, o.called)
        assert o.cleaning in CLEANING_NAMES and np.isnan(o.tubes_to_plug)
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
    assert g.meta["refused"] and all("raises" in v for v in g.meta["refused"].values())


def test_every_catalog_action_occurs_with_the_expected_success_and_is_closed(goldens):
    seen = {}
    for g in goldens.values():
        for j, o in enumerate(g.ops):
            if o.action < len(ACTIONS) and o.success:
                seen.setdefault(ACTIONS[o.action], []).append(int(g.op_closed[j]))
    missing = [a for a in ACTIONS if a not in seen]
    assert not missing, "catalogued actions no fixture carries out: %s" % missing
    assert all(all(v) for v in seen.values()), [a for a, v in seen.items() if not all(v)]
    # and the fixtures know no action the catalog does not
    assert all(o.action <= len(ACTIONS) for g in goldens.values() for o in g.ops)


def test_oc1_covers_the_generators_conditions_and_branches(goldens):
    g = goldens["oc1_steam_generators"]
    labels = [c[2] for c in g.cols]
    at = lambda step, lab: g.state[list(g.state_steps).index(step)][labels.index(lab)]
    # three generators in different conditions when the first calls are made
    deg = [at(2, "sg[%d].tsp_ht_degradation" % i) for i in range(3)]
    scale = [at(2, "sg[%d].scale_thickness" % i) for i in range(3)]
    assert deg[0] > 0.05 and deg[1] < 0.001 and 0.001 < deg[2] < 0.05, deg
    assert scale[0] > 1.0 and scale[1] < 0.01 and 0.1 < scale[2] < 1.0, scale
    by = lambda kind, action: [(j, o) for j, o in enumerate(g.ops) if g.kind_name(o) == (kind, action)]
    # every per-generator action, on more than one generator where it acts
    for a in [a for k, a in ACTIONS if k == "steam_generator"]:
        assert by("steam_generator", a), a
    assert {o.unit for _j, o in by("steam_generator", "tsp_chemical_cleaning") if o.success} == {0, 1, 2}
    # moisture separator below 0.98 and at >= 0.99; routine maintenance on both sides of the 0.999 cap
    q = [g.op_before[j, _col(g, "sg[%d].steam_quality" % o.unit)] for j, o in by("steam_generator", "moisture_separator_maintenance")]
    assert min(q) < 0.98 and max(q) >= 0.99
    assert {bool(g.op_expect_change[j]) for j, _o in by("steam_generator", "routine_maintenance")} == {True, False}
    # scale cleaning with each cleaning_type branch: default, chemical, mechanical, anything else
    cleaning = {o.cleaning for a in ("scale_removal", "tube_interior_scale_cleaning", "primary_scale_cleaning") for _j, o in by("steam_generator", a)}
    assert cleaning >= {0, 1, 2, 5}
    for a, eff in ((0, 0.9), (1, 0.9), (2, 0.95), (5, 0.85)):
        for j, o in enumerate(g.ops):
            if o.success and g.kind_name(o)[1] in ("scale_removal", "tube_interior_scale_cleaning", "primary_scale_cleaning") and o.cleaning == a:
                c = _col(g, "sg[%d].scale_iron_oxide" % o.unit)
                assert g.op_after[j, c] == g.op_before[j, c] * (1.0 - eff), (j, o)
    # the four system actions; steam quality and load balancing on both sides
    for a in [a for k, a in ACTIONS if k == "steam_generator_system"]:
        assert by("steam_generator_system", a), a
    assert {bool(g.op_expect_change[j]) for j, _o in by("steam_generator_system", "system_steam_quality_maintenance")} == {True, False}
    lb = by("steam_generator_system", "load_balancing_maintenance")
    above = [[g.op_before[j, _col(g, "sg[%d].tsp_ht_degradation" % i)] > 0.05 for i in range(3)] for j, _o in lb]
    assert [True, True, True] in above and [False, False, False] in above
    (j3,) = [j for (j, _o), a in zip(lb, above) if all(a)]
    cleaned = [bool(_changed(g, j3)[_col(g, "sg[%d].tsp_magnetite[0]" % i)]) for i in range(3)]
    assert cleaned == [True, True, False], "the limit of two generators does not show"
    # two calls on one generator between the same two steps; unknown types; delegated calls, one to a generator that is none
    assert [j for j in range(1, len(g.ops)) if (g.ops[j].step, g.ops[j].unit, g.ops[j].action, g.ops[j].called) ==
            (g.ops[j - 1].step, g.ops[j - 1].unit, g.ops[j - 1].action, g.ops[j - 1].called) and g.ops[j].called == "steam_generator"]
    assert {o.called for o in g.ops if o.action == len(ACTIONS)} == {"steam_generator", "steam_generator_system"}
    delegated = [o for o in g.ops if o.sg_index >= 0]
    assert any(o.success for o in delegated) and any(not o.success and o.unit == 3 for o in delegated)
    # tsp_shutdown_required is not re-evaluated by a cleaning (tsp_fouling_model.py:447-487)
    for j, o in enumerate(g.ops):
        if o.success and o.called == "steam_generator":
            c = _col(g, "sg[%d].tsp_shutdown_required" % o.unit)
            assert g.op_after[j, c] == g.op_before[j, c]


def test_oc2_covers_the_condenser_and_ejector_branches(goldens):
    g = goldens["oc2_condenser"]
    by = lambda kind, action: [(j, o) for j, o in enumerate(g.ops) if g.kind_name(o) == (kind, action)]
    for k, a in ACTIONS:
        if k in ("condenser", "ejector"):
            assert by(k, a), (k, a)
    first = g.op_before[0]
    assert first[_col(g, "cond.biofouling_thickness")] > 0.5 and first[_col(g, "cond.current_air_leakage")] > 0.1
    assert first[_col(g, "cond.ej_nozzle_fouling[0]")] < 0.75 and first[_col(g, "cond.ej_nozzle_erosion[1]")] < 1.0
    assert {o.cleaning for _j, o in by("condenser", "condenser_tube_cleaning")} == {0, 1, 2, 3, 5}
    assert {o.cleaning for _j, o in by("ejector", "vacuum_ejector_cleaning")} >= {0, 1, 2, 3, 4}
    assert {o.unit for _j, o in by("ejector", "vacuum_ejector_cleaning")} == {0, 1}
    # the ejector's fall-through: a type its dispatcher does not name is general maintenance, recorded as the catalog's "general"
    general = by("ejector", "general")
    assert len(general) >= 2 and all(o.success and g.op_after[j, _col(g, "cond.ej_nozzle_fouling[%d]" % o.unit)] == 1.0 for j, o in general)
    # one unknown condenser type; the water treatment moves the condenser-owned chemistry (chem[1]) and never the shared one
    assert [o for o in g.ops if o.action == len(ACTIONS) and o.called == "condenser" and not o.success]
    for j, _o in by("condenser", "condenser_water_treatment"):
        moved = {g.op_labels[q] for q in np.nonzero(_changed(g, j))[0]}
        assert "chem[1].ph" in moved and "chem[1].chlorine_residual" in moved and not [m for m in moved if m.startswith("chem[0]")]
    # tube plugging is refused, with what the live reference does
    assert "AttributeError" in g.meta["refused"]["condenser:condenser_tube_plugging"]
    assert "KeyError" in g.meta["refused"]["steam_generator:eddy_current_testing"]


def test_oc3_runs_beside_the_automatic_pump_maintenance(goldens):
    g = goldens["oc3_long_run"]
    labels = [c[2] for c in g.cols]
    performed = g.state[:, labels.index("maint.maintenance_actions_performed")]
    assert performed[-1] >= 1, "the automatic pump maintenance never acts in this run"
    assert {g.kind_name(o)[0] for o in g.ops} >= {"steam_generator", "condenser"}
    assert all(o.success for o in g.ops) and max(o.step for o in g.ops) + 20 <= g.T
    # the operator's calls move none of the automatic system's columns
    for j, o in enumerate(g.ops):
        s = list(g.state_steps).index(o.step)
        assert not [m for m in g.op_labels if m.startswith(("maint.", "mpump["))]
