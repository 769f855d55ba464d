"""Reference fixtures for operator-ordered maintenance of steam generators and condenser: tests/golden/operator_components/oc*.npz.

Drives REFERENCE simulators (oracle/ref_harness: refsim, trace.run_reference; needs a machine with the reference) with a script of
``perform_maintenance(type, **kwargs)`` calls on a steam generator, the steam-generator system, the condenser or a steam-jet ejector,
placed BETWEEN steps, and records, in the layout of the trajectory fixtures (oracle/ref_harness/make_golden.py) plus:

  ops[K, 8]                  (step, component kind of the object called, unit (the generator a delegated call names), catalog index, cleaning type NPB_CLEANING_*, tubes_to_plug or NaN, success,
                             sg_index or -1) of every call, in call order; ``step`` = t: the call is made after t steps, before step t;
                             catalog index = position in _lib.COMPONENT_ACTIONS, len(COMPONENT_ACTIONS) for a type outside it;
                             sg_index >= 0: the call went through the SYSTEM's perform_maintenance with that kwarg and was delegated
  op_before[K, ncol]         the reference's value of every schema column of the sections a call may touch (sg[0..2], chem[0..1], cond,
  op_after[K, ncol]          sec) immediately before / after the call
  op_labels[ncol]            the schema labels of those columns
  op_expect_change[K]        1 = the call changes carried state by construction of the scenario, 0 = it changes none
  op_closed[K]               the CLOSURE check of that call, on the live reference: simulator A is the fixture's run, with the call;
                             simulator B is a fresh simulator given the same scenario (same history, every other call included) that
                             does NOT make this call but has every schema member the call moved poked to the value A held after it;
                             1 = every schema column and observation of A and B is equal to the bit after each of the next
                             CLOSURE_STEPS steps, and the call moved no schema column outside op_labels.  0 = the handler writes
                             something the step reads and the schema does not carry: such a handler cannot be restated on the carried
                             state.  (Fresh simulators, not copy.deepcopy: a deep copy of the reference does not step like its original.)

meta["refused"] lists the reference handlers that are not offered, with what the live reference does when they are called.

trace.run_reference applies a step's pokes before that step and accepts a callable as a poke's value: the calls ride on that (the
"poke" writes a member back with the value it has).  The files go into a sub-directory because every existing replay test
parametrises over tests/golden/*.npz and would replay them without their calls.

    python tools/make_component_maintenance_golden.py [--explore] [scenario ...]

--explore prints the closure result per call and writes nothing.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "tests", "golden", "operator_components")
CLOSURE_STEPS = 8
SECTIONS = ("sg[", "chem[", "cond.", "sec.")
SG = "secondary_physics.steam_generator_system.steam_generators[%d]"
TSP = SG + ".tsp_fouling.deposits.%s_thickness[%d]"
SCALE = SG + ".tube_interior_fouling.%s"
COND = "secondary_physics.condenser.%s"
EJ = "=list(root.secondary_physics.condenser.vacuum_system.ejectors.values())[%d].%s"
KINDS = ("steam_generator", "steam_generator_system", "condenser", "ejector")
UNITS = {"steam_generator": 3, "steam_generator_system": 1, "condenser": 1, "ejector": 2}


def tsp(i, magnetite, copper, silica, biological, slope=0.02):
    """deposits of generator i: the given thickness at the top support plate, `slope` of it more per plate below"""
    out = []
    for k in range(7):
        f = 1.0 + slope * (6 - k)
        out += [(TSP % (i, "magnetite", k), magnetite * f), (TSP % (i, "copper", k), copper * f), (TSP % (i, "silica", k), silica * f),
                (TSP % (i, "biological", k), biological * f)]
    return out


def scale(i, mm):
    return [(SCALE % (i, "scale_thickness"), mm), (SCALE % (i, "scale_composition['iron_oxide']"), mm * 0.6),
            (SCALE % (i, "scale_composition['crud_deposits']"), mm * 0.3), (SCALE % (i, "scale_composition['corrosion_products']"), mm * 0.1)]


def quality(q0, q1, q2):
    return [((SG % i) + ".steam_quality", q) for i, q in enumerate((q0, q1, q2))]


def fouled_condenser(bio=0.8, sc=0.5, corr=0.3, hours=3000.0, dist=1.3):
    return [(COND % "fouling_model.biofouling_thickness", bio), (COND % "fouling_model.scale_thickness", sc),
            (COND % "fouling_model.corrosion_product_thickness", corr), (COND % "fouling_model.time_since_cleaning", hours),
            (COND % "fouling_model.fouling_distribution_factor", dist)]


def ejectors(a, b):
    out = []
    for k, (nf, df, ne) in enumerate((a, b)):
        out += [(EJ % (k, "nozzle_fouling_factor"), nf), (EJ % (k, "diffuser_fouling_factor"), df), (EJ % (k, "nozzle_erosion_factor"), ne)]
    return out


def op(step, comp, unit, action, expect, **kw):
    """one call: after `step` steps, perform_maintenance(action, **kw) on unit `unit` of component kind `comp`"""
    return dict(step=step, comp=comp, unit=unit, action=action, expect=expect, kw=kw)


def scenarios():
    S = []
    sg, sys_, cd, ej = KINDS
    # OC1: three generators in different conditions.  SG-0 fouled (about 2 mm of deposit per support plate: heat-transfer degradation
    # ~0.16 > 5 %), 1.5 mm of tube scale; SG-1 as built (deposits ~1e-9 mm, no scale to speak of); SG-2 in between (0.6 mm: ~0.04 < 5 %,
    # 0.4 mm of scale).  The steam quality is poked before the calls that read it (the step moves it by itself).
    init = tsp(0, 1.0, 0.3, 0.4, 0.2) + scale(0, 1.5) + tsp(2, 0.3, 0.1, 0.15, 0.05) + scale(2, 0.4)
    readers = ("tube_bundle_inspection", "tsp_inspection", "tsp_flow_test", "tube_interior_inspection",
               "tube_interior_eddy_current_testing", "tube_eddy_current_testing", "primary_chemistry_optimization")
    ops = [op(2, sg, 0, a, False) for a in readers] + [op(3, sg, 1, a, False) for a in readers[:3]] + [
        op(4, sg, 0, "moisture_separator_maintenance", True), op(4, sg, 1, "moisture_separator_maintenance", True),
        op(5, sg, 2, "routine_maintenance", True),
        op(6, sg, 1, "routine_maintenance", False),                    # quality already 0.999: min(0.999, q + 0.001) is q
        op(7, sg, 0, "water_chemistry_adjustment", False),             # resets the steam-generator system's own chemistry: not carried state
        op(8, sg, 0, "secondary_side_cleaning", True), op(8, sg, 1, "secondary_side_cleaning", True),
        op(10, sg, 0, "scale_removal", True),                          # default cleaning_type: chemical
        op(11, sg, 2, "tube_interior_scale_cleaning", True, cleaning_type="mechanical"),
        op(12, sg, 0, "primary_scale_cleaning", True, cleaning_type="combined"),       # anything else
        op(12, sg, 1, "primary_scale_cleaning", True, cleaning_type="chemical"),
        op(14, sg, 0, "tsp_chemical_cleaning", True), op(14, sg, 0, "tsp_chemical_cleaning", True),    # twice between the same two steps
        op(15, sg, 2, "tsp_mechanical_cleaning", True), op(16, sg, 1, "tsp_chemical_cleaning", True),
        op(18, sys_, 0, "system_coordination_maintenance", False),
        op(19, sys_, 0, "system_steam_quality_maintenance", True),     # 0.97 and 0.985 are below 0.99, 0.995 is not
        op(20, sys_, 0, "system_steam_quality_maintenance", False),    # nobody below 0.99
        op(21, sys_, 0, "load_balancing_maintenance", False),          # nobody above 5 % after the cleanings
        op(23, sys_, 0, "load_balancing_maintenance", True),           # all three above 5 %: the first two are cleaned
        op(25, sys_, 0, "routine_maintenance", True),
        op(26, sg, 0, "bogus_maintenance", False), op(26, sys_, 0, "bogus_maintenance", False),
        op(27, sys_, 0, "tsp_mechanical_cleaning", True, sg_index=2),  # delegated to SG-2
        op(27, sys_, 0, "scale_removal", True, sg_index=0, cleaning_type="mechanical"),
        op(28, sys_, 0, "tsp_chemical_cleaning", False, sg_index=3),   # no such generator: "Unknown system maintenance type"
        op(40, sg, 2, "tsp_chemical_cleaning", True), op(40, sg, 2, "scale_removal", True),
    ]
    pokes = {4: quality(0.97, 0.995, 0.985), 6: quality(0.97, 0.999, 0.985), 19: quality(0.97, 0.995, 0.985), 20: quality(0.992, 0.995, 0.99),
             22: tsp(0, 1.0, 0.3, 0.4, 0.2) + tsp(1, 0.8, 0.2, 0.3, 0.1) + tsp(2, 0.9, 0.25, 0.3, 0.15)}
    S.append(dict(name="oc1_steam_generators", steps=60, dt=5.0, noise=True, noise_seed=42, every=1, init_pokes=init, pokes=pokes, ops=ops))
    # OC2: a fouled condenser, degraded ejectors, raised air leakage; fouled again before each cleaning type
    worn = ((0.7, 0.75, 0.85), (0.9, 0.92, 0.95))
    init = fouled_condenser() + ejectors(*worn) + [(COND % "vacuum_system.current_air_leakage", 0.12)]
    ops = [
        op(2, cd, 0, "vacuum_system_test", False), op(2, ej, 0, "vacuum_ejector_inspection", False), op(2, ej, 1, "vacuum_ejector_inspection", False),
        op(3, cd, 0, "condenser_tube_cleaning", True),                 # default cleaning_type: chemical
        op(5, cd, 0, "condenser_tube_cleaning", True, cleaning_type="mechanical"),
        op(7, cd, 0, "condenser_tube_cleaning", True, cleaning_type="hydroblast"),
        op(9, cd, 0, "condenser_tube_cleaning", True, cleaning_type="brush"),          # anything else
        op(10, cd, 0, "condenser_tube_cleaning", True, cleaning_type="chemical"),
        op(11, cd, 0, "condenser_chemical_cleaning", True),
        op(13, cd, 0, "condenser_water_treatment", True), op(15, cd, 0, "vacuum_leak_detection", True),
        op(17, ej, 0, "vacuum_ejector_cleaning", True), op(17, ej, 1, "vacuum_ejector_cleaning", True, cleaning_type="mechanical"),
        op(19, ej, 0, "vacuum_ejector_cleaning", True, cleaning_type="replacement"),
        op(19, ej, 1, "vacuum_ejector_cleaning", False, cleaning_type="hydroblast"),   # none of the three: nothing is cleaned
        op(21, ej, 0, "vacuum_ejector_nozzle_replacement", True), op(21, ej, 1, "vacuum_ejector_mechanical_cleaning", True),
        op(23, ej, 0, "routine_maintenance", True), op(23, ej, 1, "general", True),
        op(24, ej, 0, "vacuum_ejector_cleaning", True, cleaning_type="chemical"),
        op(25, ej, 1, "some_other_maintenance", True),                 # the dispatcher's fall-through: general maintenance
        op(26, cd, 0, "bogus_maintenance", False),
        op(30, cd, 0, "condenser_water_treatment", True), op(30, cd, 0, "vacuum_leak_detection", True),
    ]
    pokes = {5: fouled_condenser(), 7: fouled_condenser(0.6, 0.7, 0.2, 1000.0, 1.1), 9: fouled_condenser(), 11: fouled_condenser(0.9, 0.4, 0.5, 5000.0, 1.5),
             21: ejectors(*worn), 23: ejectors(*worn), 25: ejectors(*worn)}
    S.append(dict(name="oc2_condenser", steps=60, dt=5.0, noise=True, noise_seed=42, every=1, init_pokes=init, pokes=pokes, ops=ops))
    # OC3: the data-gen runner's plant (state management and AutoMaintenanceSystem on, thresholds of the feedwater pumps only: the
    # reference's own automatic maintenance of the other components is not on the device) from fixture m1's oil levels, so that the
    # automatic top-off runs beside the operator's cleaning of a fouled generator and of the fouled condenser
    S.append(dict(name="oc3_long_run", steps=48, dt=5.0, noise=True, noise_seed=42, every=1, feedwater_thresholds_only=True,
                  runner=dict(action="oil_top_off", duration_hours=4.0, feedwater_ic={"pump_oil_levels": [58.3, 58.1, 98.0, 57.0]}),
                  init_pokes=tsp(0, 1.0, 0.3, 0.4, 0.2) + scale(0, 1.5) + fouled_condenser() + ejectors(*worn),
                  ops=[op(8, sg, 0, "tsp_chemical_cleaning", True), op(8, sg, 0, "scale_removal", True),
                       op(12, cd, 0, "condenser_tube_cleaning", True, cleaning_type="mechanical"),
                       op(12, ej, 0, "vacuum_ejector_mechanical_cleaning", True), op(20, sys_, 0, "routine_maintenance", True)]))
    return S


def target_of(sim, o):
    sp = sim.secondary_physics
    if o["comp"] == "steam_generator":
        return sp.steam_generator_system.steam_generators[o["unit"]]
    if o["comp"] == "steam_generator_system":
        return sp.steam_generator_system
    if o["comp"] == "condenser":
        return sp.condenser
    return list(sp.condenser.vacuum_system.ejectors.values())[o["unit"]]


def success_of(res):
    return bool(res["success"] if isinstance(res, dict) else res.success)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def run(sc, cols, catalog, poke_instead=None, explore=False):
    """the scenario on a fresh reference simulator.  poke_instead = (j, column indices, values): call j is NOT made; the schema members it
    moved in the run that made it are poked to the values they had after it (the closure check's simulator B)"""
    from nuclear_sim_amd import _lib
    from oracle.ref_harness import refsim, trace
    from oracle.ref_harness.trace import _val
    labels = [c[2] for c in cols]
    paths = [c[3] for c in cols]
    inside = np.array([lab.startswith(SECTIONS) for lab in labels])
    sel = np.nonzero(inside)[0]
    rows, before, after, moved_outside = [], [], [], []
    anchor = (SG % 0) + ".water_level"
    assert [o["step"] for o in sc["ops"]] == sorted(o["step"] for o in sc["ops"])
    by_step = {}
    for j, o in enumerate(sc["ops"]):
        by_step.setdefault(o["step"], []).append((j, o))

    def hook(step):
        def call(sim):
            for j, o in by_step[step]:
                b = np.array([_val(sim, p) for p in paths])
                if poke_instead is not None and poke_instead[0] == j:
                    for c, v in zip(poke_instead[1], poke_instead[2]):
                        old = trace.resolve(sim, paths[c])
                        trace._poke(sim, paths[c], bool(v) if isinstance(old, (bool, np.bool_)) else int(v) if isinstance(old, (int, np.integer)) else float(v))
                    success = np.nan
                else:
                    try:
                        with refsim.quiet():
                            res = target_of(sim, o).perform_maintenance(o["action"], **o["kw"])
                        success = float(success_of(res))
                    except Exception as e:      # noqa: BLE001
                        if not explore:
                            raise
                        print("  RAISES %r: %s %s" % (o["action"], type(e).__name__, e))
                        success = np.nan
                a = np.array([_val(sim, p) for p in paths])
                moved = ~same(b, a)
                moved_outside.append([labels[c] for c in np.nonzero(moved & ~inside)[0]])
                before.append(b); after.append(a)
                key = (o["comp"], o["action"])
                if o["kw"].get("sg_index") is not None and o["comp"] == "steam_generator_system" and key not in catalog:
                    key = ("steam_generator", o["action"])       # delegated
                unit = o["kw"]["sg_index"] if key[0] == "steam_generator" and o["comp"] != "steam_generator" else o["unit"]
                if o["comp"] == "ejector" and key not in catalog:
                    key = ("ejector", "general")                  # the ejector's dispatcher has no "unknown": everything else is general maintenance
                index = catalog.index(key) if key in catalog else len(catalog)
                rows.append((o["step"], KINDS.index(o["comp"]), unit, index, _lib.cleaning_type_index(o["kw"].get("cleaning_type")),
                             o["kw"].get("tubes_to_plug", np.nan), success, o["kw"].get("sg_index", -1)))
            return _val(sim, anchor)      # written back as it is
        return call
    sc = dict(sc)
    pokes = {t: list(lst) for t, lst in sc.get("pokes", {}).items()}
    for step in by_step:
        pokes.setdefault(step, []).append(("~" + anchor, hook(step)))
    sc["pokes"] = pokes
    ref, sim = trace.run_reference(sc, cols)
    ref["ops"] = np.array(rows, dtype=np.float64)
    ref["full_before"], ref["full_after"] = np.array(before, dtype=np.float64), np.array(after, dtype=np.float64)
    ref["op_before"], ref["op_after"] = ref["full_before"][:, sel], ref["full_after"][:, sel]
    ref["op_labels"] = np.array([labels[j] for j in sel])
    ref["op_expect_change"] = np.array([int(bool(o["expect"])) for o in sc["ops"]], dtype=np.int8)
    ref["moved_outside"] = moved_outside
    sc["pokes"] = {t: [(p, v) for p, v in lst if not p.startswith("~")] for t, lst in pokes.items()}
    sc["pokes"] = {t: lst for t, lst in sc["pokes"].items() if lst}
    return ref, sim, sc


def closure(sc0, ref, cols, catalog, explore=False):
    """the closure check of every call (module docstring): op_closed[K] and, per call, what differed"""
    labels = [c[2] for c in cols]
    closed, why = [], []
    for j, o in enumerate(sc0["ops"]):
        t = o["step"]
        moved = np.nonzero(~same(ref["full_before"][j], ref["full_after"][j]))[0]
        what = ""
        if ref["moved_outside"][j]:
            what = "moved outside the recorded sections: %s" % ref["moved_outside"][j][:4]
        elif np.isnan(ref["ops"][j, 6]):
            what = "raises"
        else:
            twin, _sim, _sc = run(sc0, cols, catalog, poke_instead=(j, moved, ref["full_after"][j][moved]), explore=explore)
            for k in range(t + 1, min(t + CLOSURE_STEPS, sc0["steps"]) + 1):
                eq = same(ref["state"][k], twin["state"][k])
                if not eq.all() or not same(ref["obs"][k - 1], twin["obs"][k - 1]).all():
                    what = "after step %d (%d after the call): %s" % (k - 1, k - t, [labels[c] for c in np.nonzero(~eq)[0][:4]] or "obs")
                    break
        closed.append(int(not what)); why.append(what)
        if explore:
            print("  %-3d %-22s %d %-36s %-28s success %s moved %-3d closed %d %s" % (
                t, o["comp"], o["unit"], o["action"], o["kw"], ref["ops"][j, 6], len(moved), closed[-1], what))
    ref["op_closed"] = np.array(closed, dtype=np.int8)
    ref["op_why"] = why


def refused():
    """what the live reference does with the handlers that are not offered"""
    from nuclear_sim_amd import _lib
    from oracle.ref_harness import refsim
    out = {}
    for (comp, action), reason in _lib.COMPONENT_ACTIONS_NOT_OFFERED.items():
        sim = refsim.make_sim(dt=5.0)
        try:
            with refsim.quiet():
                res = target_of(sim, dict(comp=comp, unit=0)).perform_maintenance(action)
            out["%s:%s" % (comp, action)] = "returns success=%s" % success_of(res)
        except Exception as e:      # noqa: BLE001 -- the point is to record whatever it raises
            out["%s:%s" % (comp, action)] = "raises %s: %s" % (type(e).__name__, e)
    return out


def check(sc, ref, catalog):
    """what keeps the fixture from being vacuous (tests/test_component_maintenance_fixtures.py re-asserts it on the committed files)"""
    ops, b, a = ref["ops"], ref["op_before"], ref["op_after"]
    assert len(ops) == len(sc["ops"])
    for j, o in enumerate(sc["ops"]):
        changed = ~same(b[j], a[j])
        assert changed.any() == bool(o["expect"]), "%s op %d %r: columns changed %s" % (sc["name"], j, o, list(ref["op_labels"][changed]))
        if ops[j, 3] < len(catalog) and 0 <= ops[j, 2] < UNITS[catalog[int(ops[j, 3])][0]]:
            assert ops[j, 6] == 1.0, (j, o)
            assert ref["op_closed"][j] == 1, "%s op %d %r is not closed: %s" % (sc["name"], j, o, ref["op_why"][j])
        else:
            assert ops[j, 6] == 0.0 and not changed.any(), (j, o)
    assert not ref["done"].any(), "the plant trips in this scenario"
    assert max(o["step"] for o in sc["ops"]) + CLOSURE_STEPS <= sc["steps"]


def main(argv):
    from nuclear_sim_amd.schema import SCHEMA
    from nuclear_sim_amd._lib import COMPONENT_ACTIONS
    from oracle.ref_harness import trace
    explore = "--explore" in argv
    names = [a for a in argv if not a.startswith("--")]
    catalog = list(COMPONENT_ACTIONS)
    cols = SCHEMA.columns()
    os.makedirs(OUT, exist_ok=True)
    seen = set()
    not_offered = refused()
    for sc in scenarios():
        if names and sc["name"] not in names:
            continue
        if explore:
            print(sc["name"])
        sc0 = sc
        ref, _sim, sc = run(sc0, cols, catalog, explore=explore)
        closure(sc0, ref, cols, catalog, explore)
        seen |= {int(r[3]) for r in ref["ops"] if r[3] < len(catalog)}
        if explore:
            print("  done:", int(ref["done"].sum()), "expect mismatches:",
                  [j for j, o in enumerate(sc["ops"]) if (~same(ref["op_before"][j], ref["op_after"][j])).any() != bool(o["expect"])])
            continue
        check(sc, ref, catalog)
        T = sc["steps"]
        steps = list(range(0, T + 1, sc.get("every", 1)))
        meta = {k: v for k, v in sc.items() if not callable(v) and k not in ("pokes", "init_pokes", "ops", "_maint_thresholds", "_maint_params")}
        if sc.get("_maint_thresholds"):
            meta["maint_thresholds"] = sc["_maint_thresholds"]
        if sc.get("_maint_params"):
            meta["maint_params"] = sc["_maint_params"]
        meta["resets"] = {}
        meta["pokes"] = {str(k): [[p, trace.poke_number(v)] for p, v in lst] for k, lst in sc.get("pokes", {}).items()}
        meta["pokes_schema"] = meta["pokes"]
        meta["init_pokes"] = [[p, trace.poke_number(v)] for p, v in sc.get("init_pokes", [])]
        meta["ops"] = [dict(step=o["step"], component=o["comp"], unit=o["unit"], action=o["action"], kwargs=o["kw"]) for o in sc["ops"]]
        meta["closure_steps"] = CLOSURE_STEPS
        meta["refused"] = not_offered
        path = os.path.join(OUT, sc["name"] + ".npz")
        np.savez_compressed(path, action=ref["action"], magnitude=ref["magnitude"], setpoint=ref["setpoint"], cooling=ref["cooling"],
                            noise_z=ref["noise_z"], obs=ref["obs"], reward=ref["reward"], done=ref["done"], info=ref["info"],
                            state_steps=np.array(steps), sec_keys=ref["sec_keys"], sec=ref["sec"], rc_keys=ref["rc_keys"], rc=ref["rc"],
                            state=ref["state"][steps], labels=np.array([c[2] for c in cols]), kinds=np.array([c[0] for c in cols]),
                            paths=np.array([c[3] for c in cols]), meta=json.dumps(meta), ops=ref["ops"], op_before=ref["op_before"],
                            op_after=ref["op_after"], op_labels=ref["op_labels"], op_expect_change=ref["op_expect_change"],
                            op_closed=ref["op_closed"])
        print(sc["name"], "steps", T, "ops", len(ref["ops"]), "successful", int(ref["ops"][:, 6].sum()), "closed", int(ref["op_closed"].sum()),
              os.path.getsize(path), "bytes ->", os.path.relpath(path, ROOT))
    if not names and not explore:
        missing = [catalog[k] for k in range(len(catalog)) if k not in seen]
        assert not missing, "catalog actions no fixture calls: %s" % missing


if __name__ == "__main__":
    main(sys.argv[1:])
