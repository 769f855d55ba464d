"""CPU: the reference fixtures of scattered operator calls (tests/golden/operator_calls/, tools/make_scattered_calls_golden.py) hold what
tests/test_scattered_calls_gpu.py relies on: enough calls drawn over the whole of both catalogs, every branch input the explicit calls
are there for, the reference's success, change where and only where a call acts by the handlers' own conditions, only the sections
an action may touch moving, and a float32 run that differs from the fp64 one.  No library, no compute calls."""
import os
import re

import numpy as np
import pytest

from component_maintenance_golden import ACTIONS, CLEANING_NAMES, KINDS, UNITS
from operator_maintenance_golden import ACTIONS as PUMP_ACTIONS, HANDLERS
from scattered_calls_golden import ScatteredCalls, same, scattered_fixture_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ_ONLY = {("steam_generator", a) for a in ("tube_bundle_inspection", "tsp_inspection", "tsp_flow_test", "tube_interior_inspection",
                                              "tube_interior_eddy_current_testing", "tube_eddy_current_testing", "primary_chemistry_optimization",
                                              "water_chemistry_adjustment")} | {
    ("condenser", "vacuum_system_test"), ("ejector", "vacuum_ejector_inspection")}
SCALE_ACTIONS = ("scale_removal", "tube_interior_scale_cleaning", "primary_scale_cleaning")


@pytest.fixture(scope="module")
def comp():
    return ScatteredCalls("components")


@pytest.fixture(scope="module")
def pumps():
    return ScatteredCalls("pumps")


def _by(g, kind, action):
    return [(j, c) for j, c in enumerate(g.calls) if ACTIONS[c.action] == (kind, action)]


def _q(g, j, i):
    return g.before[j, g.col["sg[%d].steam_quality" % i]]


def test_fixtures_live_in_their_own_directory_and_say_how_they_were_drawn(comp, pumps):
    from component_maintenance_golden import component_fixture_names
    from golden_util import fixture_names
    from operator_maintenance_golden import operator_fixture_names
    names = scattered_fixture_names()
    assert names == sorted(comp.names + pumps.names) and len(comp.names) >= 1 and len(pumps.names) >= 1
    for other in (fixture_names(), operator_fixture_names(), component_fixture_names()):
        assert not [n for n in other if n.startswith("sc_")]
    for n in names:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "operator_calls", n + ".npz")) <= 360 * 1024, n
    for g in (comp, pumps):
        for m in g.metas:
            assert isinstance(m["seed"], int) and m["ranges"] and m["steps_before"] >= 1 and 0 < m["else_within"] < 0.1
            assert all(set(d) == {"call", "action", "raises"} and d["raises"][0].isupper() for d in m["dropped"])
        assert len(g.written) == len(g.calls) == len(g.before) == len(g.expect_change)
        # the members nobody could assign are integer members: every real member of the sections was drawn
        assert all(g.kinds[g.col[m.split(".", 1)[1] if g is pumps and "." in m else m]] == "i32" for m in g.metas[0]["not_poked"])
    # the ranges the two GPU tests' own scrambles use (tests/test_component_maintenance_gpu.py _scrambled, test_operator_maintenance_gpu.py
    # _scrambled_pumps), held here as numbers so that neither file imports the other
    r = {name: (lo, hi) for name, lo, hi in comp.metas[0]["ranges"]}
    assert r["tsp_magnetite"] == (0.0, 1.2) and r["sg.scale_thickness"] == (0.0, 2.0) and r["cond.time_since_cleaning"] == (0.0, 6000.0)
    assert r["cond.ej_nozzle_erosion"] == (0.7, 1.0) and r["cond.current_air_leakage"] == (0.05, 0.15)
    r = {name: (lo, hi) for name, lo, hi in pumps.metas[0]["ranges"]}
    assert r["oil_level"] == (40.0, 100.0) and r["wear_mechanical_seals"] == (0.0, 17.0) and len(r) == 15


def test_the_drawn_calls_cover_both_catalogs_within_their_ranges(comp, pumps):
    drawn = [(j, c) for j, c in enumerate(comp.calls) if not c.explicit]
    assert len(drawn) >= 160 and {c.action for _j, c in drawn} == set(range(len(ACTIONS)))
    assert {c.cleaning for _j, c in drawn} == set(CLEANING_NAMES)
    for kind, n in UNITS.items():
        assert {c.unit for _j, c in drawn if ACTIONS[c.action][0] == kind} == set(range(n)), kind
    for name, lo, hi in comp.metas[0]["ranges"]:
        sec, _, member = name.rpartition(".")
        cols = [q for q, lab in enumerate(comp.labels) if lab.split("[")[0].split(".")[0] == (sec or lab.split("[")[0].split(".")[0]) and
                lab.split(".", 1)[1].split("[")[0] == member]
        assert cols, name
        v = comp.before[[j for j, _c in drawn]][:, cols]
        assert lo <= v.min() and v.max() <= hi and v.max() - v.min() > 0.8 * (hi - lo), (name, v.min(), v.max())
    drawn = [(j, c) for j, c in enumerate(pumps.calls) if not c.explicit]
    assert len(drawn) >= 130 and {c.action for _j, c in drawn} == set(range(len(PUMP_ACTIONS)))
    assert {c.pump for _j, c in drawn} == {0, 1, 2, 3} and {c.bearing for _j, c in drawn} == {0, 1, 2, 3}
    assert any(np.isnan(c.target_level) for _j, c in drawn) and sum(not np.isnan(c.target_level) for _j, c in drawn) > 60
    for name, lo, hi in pumps.metas[0]["ranges"]:
        v = pumps.before[[j for j, _c in drawn], pumps.col[name]]
        assert lo <= v.min() and v.max() <= hi and v.max() - v.min() > 0.8 * (hi - lo), (name, v.min(), v.max())


def test_component_calls_succeed_and_move_only_what_they_may(comp):
    g = comp
    assert sorted(g.labels) == sorted(set(g.labels)) and all(lab.startswith(("sg[", "chem[", "cond.", "sec.")) for lab in g.labels)
    assert len(g.labels) >= 3 * 40 + 2 * 11 + 30 + 15
    for j, c in enumerate(g.calls):
        kind, action = ACTIONS[c.action]
        assert KINDS[c.called] == kind and 0 <= c.unit < UNITS[kind] and c.cleaning in CLEANING_NAMES and c.success, (j, c)
        for f32 in (False, True):
            changed = g.changed(j, f32)
            if (kind, action) in READ_ONLY:
                assert not changed.any(), (j, c)
            moved = {g.labels[q].split(".")[0] for q in np.nonzero(changed)[0]}
            allowed = {"steam_generator": {"sg[%d]" % c.unit}, "steam_generator_system": {"sg[0]", "sg[1]", "sg[2]", "sec"},
                       "condenser": {"cond", "chem[1]"}, "ejector": {"cond"}}[kind]
            assert moved <= allowed, (j, c, moved)
            if kind == "ejector":
                assert all(g.labels[q].endswith("[%d]" % c.unit) and g.labels[q].startswith("cond.ej_") for q in np.nonzero(changed)[0]), (j, c)
        assert g.changed(j).any() == bool(g.expect_change[j]), (j, c, [g.labels[q] for q in np.nonzero(g.changed(j))[0]])
    assert 0.5 * len(g) < g.expect_change.sum() < len(g)
    # integer members are never rounded; the float32 run starts from float32 values and ends somewhere else than the fp64 run
    ints = np.array([k == "i32" for k in g.kinds])
    assert same(g.before[:, ints], g.before32[:, ints]).all()
    assert same(g.before32[:, ~ints], g.before32[:, ~ints].astype(np.float32).astype(np.float64)).all()
    assert (~same(g.after, g.after32)).sum() > 1000 and (~same(g.after32, g.after32.astype(np.float32).astype(np.float64))).any()


def test_explicit_component_calls_enter_every_branch_from_both_sides(comp):
    g = comp
    ex = lambda kind, action: [(j, c) for j, c in _by(g, kind, action) if c.explicit]
    deg = lambda j: [g.before[j, g.col["sg[%d].tsp_ht_degradation" % i]] for i in range(3)]
    mag = lambda j: [bool(g.changed(j)[g.col["sg[%d].tsp_magnetite[0]" % i]]) for i in range(3)]
    # load balancing: all eight patterns, the first two of those above are cleaned; exactly 0.05 is not above
    lb = ex("steam_generator_system", "load_balancing_maintenance")
    assert {tuple(d > 0.05 for d in deg(j)) for j, _c in lb} == {(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)}
    for j, _c in lb:
        above = [d > 0.05 for d in deg(j)]
        want = [a and sum(above[:i]) < 2 for i, a in enumerate(above)]
        assert mag(j) == want, (j, deg(j))
    assert [j for j, _c in lb if deg(j)[0] == 0.05 and mag(j) == [False, True, True]]
    assert [j for j, _c in lb if mag(j) == [True, False, True]], "a clean generator between two cleaned ones"
    # system steam quality: each generator on each side of 0.99; exactly 0.99, 0.999, 1.0
    sq = ex("steam_generator_system", "system_steam_quality_maintenance")
    assert {tuple(_q(g, j, i) < 0.99 for i in range(3)) for j, _c in sq} == {(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)}
    for j, _c in sq:
        assert [bool(g.changed(j)[g.col["sg[%d].steam_quality" % i]]) for i in range(3)] == [_q(g, j, i) < 0.99 for i in range(3)], j
    assert {0.99, 0.999, 1.0} <= {_q(g, j, 1) for j, _c in sq}
    # moisture separator at 1.0: pulled DOWN to the cap; routine maintenance on both sides of it, generator and system
    (ms,) = [(j, c) for j, c in ex("steam_generator", "moisture_separator_maintenance") if _q(g, j, c.unit) == 1.0]
    assert g.after[ms[0], g.col["sg[%d].steam_quality" % ms[1].unit]] == 0.999
    assert {_q(g, j, c.unit) for j, c in ex("steam_generator", "routine_maintenance")} >= {0.9985, 0.9995}
    assert {_q(g, j, i) for j, _c in ex("steam_generator_system", "routine_maintenance") for i in range(3)} >= {0.9985, 0.9995}
    for j, c in ex("steam_generator", "routine_maintenance"):
        assert g.after[j, g.col["sg[%d].steam_quality" % c.unit]] == (0.999 if _q(g, j, c.unit) > 0.998 else _q(g, j, c.unit) + 0.001)
    # the scale cleanings: every cleaning type each, and once without scale
    for a in SCALE_ACTIONS:
        calls = ex("steam_generator", a)
        assert {c.cleaning for _j, c in calls} == set(CLEANING_NAMES), a
        assert [j for j, c in calls if g.before[j, g.col["sg[%d].scale_thickness" % c.unit]] == 0.0], a
    tc = ex("condenser", "condenser_tube_cleaning")
    assert {c.cleaning for _j, c in tc} == set(CLEANING_NAMES)
    layers = ("cond.biofouling_thickness", "cond.scale_thickness", "cond.corrosion_product_thickness")
    assert [j for j, _c in tc if all(g.before[j, g.col[m]] == 0.0 for m in layers)]
    ph = [g.before[j, g.col["chem[1].ph"]] for j, _c in ex("condenser", "condenser_water_treatment")]
    assert min(ph) < 9.2 < max(ph)
    assert ex("condenser", "vacuum_leak_detection")
    # every ejector action on both units; the cleaning with all six types; fouling and erosion on both sides of each cap
    for kind, a in ACTIONS:
        if kind == "ejector":
            assert {c.unit for _j, c in ex("ejector", a)} == {0, 1}, a
    ec = ex("ejector", "vacuum_ejector_cleaning")
    assert {c.cleaning for _j, c in ec} == set(CLEANING_NAMES)
    assert all(not g.changed(j).any() for j, c in ec if c.cleaning in (3, 5)) and [1 for _j, c in ec if c.cleaning == 3]
    e = lambda j, c, m: (g.before[j, g.col["cond.ej_%s[%d]" % (m, c.unit)]], g.after[j, g.col["cond.ej_%s[%d]" % (m, c.unit)]])
    for calls, steps in (([x for x in ec if x[1].cleaning in (0, 1)], (("nozzle_fouling", 0.3), ("diffuser_fouling", 0.4))),
                         ([x for x in ec if x[1].cleaning == 2] + ex("ejector", "vacuum_ejector_mechanical_cleaning"),
                          (("nozzle_fouling", 0.4), ("diffuser_fouling", 0.5), ("nozzle_erosion", 0.1))),
                         (ex("ejector", "routine_maintenance"), (("nozzle_fouling", 0.05), ("diffuser_fouling", 0.05)))):
        for m, step in steps:
            pairs = [e(j, c, m) for j, c in calls if not np.isnan(e(j, c, m)[0])]
            assert [1 for b, a in pairs if b + step < 1.0 and a == b + step] and [1 for b, a in pairs if b + step > 1.0 and a == 1.0], (m, step)
    # a NaN member: Python's max(0.0, nan) is 0.0, its min(cap, nan) the cap
    nan = [(j, c) for j, c in enumerate(g.calls) if np.isnan(g.before[j]).any()]
    assert len(nan) == 3
    got = {}
    for j, c in nan:
        (q,) = np.nonzero(np.isnan(g.before[j]))[0]
        got[re.sub(r"\[\d+\]", "", g.labels[q])] = g.after[j, q]
    assert got == {"sg.scale_thickness": 0.0, "sg.steam_quality": 0.999, "cond.ej_nozzle_fouling": 1.0}, got


def test_pump_calls_cover_handlers_bearings_and_targets(pumps):
    g = pumps
    name = lambda c: PUMP_ACTIONS[c.action]
    ex = [(j, c) for j, c in enumerate(g.calls) if c.explicit]
    for j, c in enumerate(g.calls):
        invalid = name(c) == "bearing_replacement" and c.bearing not in (0, 1, 2, 3)
        assert c.success == (name(c) in HANDLERS and not invalid), (j, c)
        assert g.changed(j).any() == bool(g.expect_change[j]), (j, c, [g.labels[q] for q in np.nonzero(g.changed(j))[0]])
        if not c.success or name(c) in ("oil_analysis", "vibration_analysis"):
            assert not g.changed(j).any() and not g.changed(j, True).any(), (j, c)
    assert {c.via for c in g.calls} == {0, 1}
    assert {(name(c), c.pump) for _j, c in ex} >= {(h, k) for h in HANDLERS for k in range(4)}
    br = [(j, c) for j, c in ex if name(c) == "bearing_replacement"]
    assert {c.bearing for _j, c in br} == {0, 1, 2, 3, 4, -1}
    wear = ("wear_motor_bearings", "wear_pump_bearings", "wear_thrust_bearing")
    for j, c in br:
        zeroed = [g.after[j, g.col[m]] == 0.0 and g.before[j, g.col[m]] > 0.0 for m in wear]
        assert zeroed == [c.bearing in (0, q + 1) for q in range(3)], (j, c)
    # oil_top_off: a target below the level, equal to it, the default's 95.0, above 100
    level = lambda j: g.before[j, g.col["oil_level"]]
    top = [(j, c) for j, c in ex if name(c) == "oil_top_off" and not np.isnan(c.target_level)]
    assert [1 for j, c in top if c.target_level < level(j) and not g.changed(j).any()]
    assert [1 for j, c in top if c.target_level == level(j) and c.target_is_level and not g.changed(j).any()]
    assert [1 for j, c in top if c.target_level == 95.0 and g.after[j, g.col["oil_level"]] == 95.0]
    assert [1 for j, c in top if c.target_level > 100.0 and g.after[j, g.col["oil_level"]] == 100.0]
    assert len({name(c) for _j, c in ex if name(c) not in HANDLERS}) >= 2
    # the conditional handlers from both sides among the drawn calls
    for a in ("bearing_inspection", "impeller_inspection", "motor_inspection", "oil_top_off", "lubrication_system_check"):
        flags = {bool(g.expect_change[j]) for j, c in enumerate(g.calls) if name(c) == a}
        assert flags == ({True} if a == "lubrication_system_check" else {True, False}), (a, flags)
    check = [level(j) < 95.0 for j, c in enumerate(g.calls) if name(c) == "lubrication_system_check"]
    assert True in check and False in check
    reals = np.array([k == "f64" for k in g.kinds])
    assert (~same(g.after, g.after32)).sum() > 500 and same(g.before[:, ~reals], g.before32[:, ~reals]).all()
