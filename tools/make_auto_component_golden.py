"""Reference fixtures for the automatic maintenance of steam generators and condenser: tests/golden/auto_components/ac*.npz + .json.

Drives REFERENCE simulators as the data-gen runner builds them (oracle/ref_harness: refsim.make_runner_sim through trace.run_reference;
needs a machine with the reference), state management and AutoMaintenanceSystem on with the composer's FULL threshold table, from
poked initial states that make the rows of SG-0..2 and the condenser fire, and records, in the layout of the trajectory fixtures
(oracle/ref_harness/make_golden.py: observations and every schema column at every step) plus:

  stamps[T + 1, 12]      StateManager.threshold_last_violation_times of the scanned rows after t steps (-1 = never), slot =
                         component * 3 + row in the order of nuclear_sim_amd._lib.CMAINT_COMPONENTS / CMAINT_PARAMS
  scanned[T, 12]         the value the reference's scan compared at step t (the state-log row's), NaN for an unused slot
  thresholds[12]         the threshold of each slot's row in the run's table (NaN = no row), comparisons[12] its comparison index
  <name>.json            the reference's work orders after the run, open and completed, on EVERY component, by number: id, component,
                         action, priority, created, planned start, completion, success; the two counters; the run's table ([name, row]
                         pairs per component kind, in the reference's dict order, which is the scan's); the rows of
                         the scanned components that resolve on the reference and stayed silent, each with its reason

The files go into a sub-directory because every replay test of tests/golden/*.npz would replay them on the unchanged oracle, which
does not maintain these components.  Before a fixture is written the tool asserts that every scanned value is at least MARGIN
(relative) away from its threshold at every step: two of the values are members the device keeps as float.

    python tools/make_auto_component_golden.py [--explore | --check | --turbine] [scenario ...]

--explore prints each run's orders and writes nothing; --check re-runs and compares with the committed files; --turbine prints the attempt
to fire the turbine's efficiency rows, which the device does not scan (turbine_probe; a full run records it in silent_rows.json).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "tests", "golden", "auto_components")
MARGIN = 1e-5
SG = "secondary_physics.steam_generator_system.steam_generators[%d]"
TSP = SG + ".tsp_fouling.deposits.magnetite_thickness[%d]"
SCALE = SG + ".tube_interior_fouling.%s"
COND = "secondary_physics.condenser.%s"
COMPONENT_IDS = ("SG-0", "SG-1", "SG-2", "SECONDARY-COMP-001-COND")      # _lib.CMAINT_COMPONENTS under the composer's naming
KIND_OF = ("steam_generator", "steam_generator", "steam_generator", "condenser")
ANCHOR = (SG % 0) + ".water_level"


def tsp_level_thickness(fraction):
    """deposit thickness [mm] that blocks `fraction` of a 23-mm hole's area (tsp_fouling_model.py:302-340)"""
    return 23.0 * (1.0 - (1.0 - fraction) ** 0.5) / 2.0


def tsp(i, fraction):
    return [(TSP % (i, k), tsp_level_thickness(fraction)) for k in range(7)]


def scale(i, mm):
    return [(SCALE % (i, "scale_thickness"), mm), (SCALE % (i, "scale_composition['crud_deposits']"), mm * 0.4)]


def fouled_condenser(bio, sc, corr):
    return [(COND % "fouling_model.biofouling_thickness", bio), (COND % "fouling_model.scale_thickness", sc),
            (COND % "fouling_model.corrosion_product_thickness", corr)]


def scenarios():
    S = []
    base = dict(steps=72, dt=5.0, noise=True, noise_seed=42, every=1, runner=dict(action="oil_top_off", duration_hours=6.0))
    # AC1: three generators and the condenser fouled from the start.  Orders on SG-0, SG-2 and the condenser in the first scan, two more
    # on the generators' wall temperature one step later, and a pump's oil top-off behind them: one queue, one counter
    S.append(dict(base, name="ac1_shared_queue",
                  init_pokes=tsp(0, 0.36) + tsp(2, 0.33) + scale(1, 2.5) + fouled_condenser(3.0, 2.0, 1.2)))
    # AC2: two rows of ONE generator crossing in the same step (the scale's thermal resistance shows in the wall temperature one step
    # after the poke, the support plates' deposits in the step of the poke): the orchestrator's choice for a generator
    S.append(dict(base, name="ac2_two_rows_one_step", steps=40, init_pokes=scale(1, 2.5), pokes={1: tsp(1, 0.40)}))
    # AC3: the support plates fouled again inside the row's one-hour cooldown (silent) and still fouled when it ends (fires again: a
    # second order for the same generator and action, an hour after the first)
    S.append(dict(base, name="ac3_row_cooldown", init_pokes=tsp(0, 0.36), pokes={6: tsp(0, 0.38)}))
    # AC4 (edited table): the row's cooldown cut to 15 minutes, the plates fouled again right after the cleaning: the row fires again
    # inside AutoMaintenanceSystem's work_order_cooldown_hours (24, compared with minutes) and no second order is created, until it has passed
    S.append(dict(base, name="ac4_work_order_cooldown", steps=40, init_pokes=tsp(0, 0.36), pokes={4: tsp(0, 0.38)},
                  table={"steam_generator": {"tsp_fouling_fraction": {"cooldown_hours": 0.25}}}))
    # AC5: steam quality poked below 0.90 on two generators.  The row stays silent, on the reference as on the device: the step clips the
    # quality it leaves behind to [0.90, 1.0] (SILENT_DEFAULT_ROWS); AC6 fires the row through an edited table
    S.append(dict(base, name="ac5_steam_quality_silent", steps=40, init_pokes=[((SG % 1) + ".steam_quality", 0.85)],
                  pokes={8: [((SG % 2) + ".steam_quality", 0.88)]}))
    # AC6 (edited table): other thresholds, comparisons, priorities and actions
    S.append(dict(base, name="ac6_edited_table", steps=40,
                  init_pokes=tsp(0, 0.22) + tsp(1, 0.36) + fouled_condenser(1.2, 0.8, 0.5),
                  table={"steam_generator": {"tsp_fouling_fraction": {"threshold": 0.2, "action": "tsp_mechanical_cleaning", "priority": "CRITICAL"},
                                             "steam_quality": {"threshold": 0.999, "comparison": "greater_equal", "action": "tube_bundle_inspection", "priority": "LOW",
                                                               "cooldown_hours": 1.0}},
                         "condenser": {"fouling_resistance": {"threshold": 0.0005, "comparison": "greater_equal", "action": "condenser_chemical_cleaning",
                                                              "priority": "EMERGENCY"}}}))
    # AC7: the condenser's tubes failing fast (vibration damage poked up: 1.8 % of the failure-rate ceiling per step): tube_leak_rate crosses
    # 0.01, the order is condenser_tube_plugging, whose handler raises after it has moved the tube counts: completed without success, counted
    S.append(dict(base, name="ac7_tube_leak", steps=40, init_pokes=[(COND % "tube_degradation.vibration_damage_accumulation", 2000.0)]))
    # AC8 (edited table): the three rows of SG-0 crossing in ONE step, their three actions all among tube_bundle_overhaul's `encompasses`: the
    # orchestrator promotes, the promoted action is no MaintenanceActionType, and the event creates no order (the rows are stamped); the
    # other generators' quality rows alone give tsp_inspection orders
    S.append(dict(base, name="ac8_overhaul_promotion", steps=40, pokes={11: scale(0, 2.5), 12: tsp(0, 0.36)},
                  table={"steam_generator": {"tsp_fouling_fraction": {"action": "tsp_mechanical_cleaning"},
                                             "steam_quality": {"threshold": 0.999, "comparison": "greater_equal", "action": "tsp_inspection", "cooldown_hours": 1.0}}}))
    # AC9 (edited table): a row whose action is a handler of the generator but no MaintenanceActionType: stamped, no order
    S.append(dict(base, name="ac9_action_is_no_type", steps=24, init_pokes=scale(1, 2.5),
                  table={"steam_generator": {"tube_wall_temperature": {"action": "primary_scale_cleaning"}}}))
    return S


# rows of the DEFAULT table no fixture can fire, with the reason (the live reference was tried: AC5)
SILENT_DEFAULT_ROWS = {
    "steam_generator:steam_quality":
        "SteamGenerator.update_state leaves steam_quality clipped to [0.90, 1.0] at every step (steam_generator.py, the quality's relaxation "
        "towards its target), so the end-of-step value the scan compares is never < 0.90; a poke of the carried member is overwritten by the "
        "next step (ac5_steam_quality_silent: 0.85 and 0.88 poked, 0.95 scanned).  ac6_edited_table fires the row with another comparison.",
}


TURBINE_IDS = tuple(["HP-%d" % k for k in range(1, 9)] + ["LP-%d" % k for k in range(1, 7)] + ["SECONDARY-COMP-001-TURB"])
STAGE = "=list(root.secondary_physics.turbine.stage_system.stages.values())[%d].%s"


def turbine_probe(cols):
    """The turbine's `efficiency` rows (fourteen stages and the turbine, `< 0.30`, action efficiency_analysis), which the device does not
    scan: an attempt to fire them on the live reference by poking carried state -- every stage's efficiency_degradation to 0.9, far past
    its design efficiency, and its deposits and blade wear to their worst.  Returns what the reference's scan saw and did."""
    from oracle.ref_harness import trace
    from oracle.ref_harness.trace import _val
    T = 12
    seen = {cid: [] for cid in TURBINE_IDS}

    def hook(sim):
        sm = sim.state_manager
        if len(sm.data):
            row = dict(sm.data.iloc[-1])
            for cid in TURBINE_IDS:
                seen[cid].append(sm._find_parameter_in_row_data(cid, "efficiency", row))
        return _val(sim, ANCHOR)
    init = []
    for k in range(14):
        init += [(STAGE % (k, "efficiency_degradation"), 0.9), (STAGE % (k, "deposit_thickness"), 5.0), (STAGE % (k, "blade_wear_factor"), 0.7)]
    sc = dict(name="turbine_probe", steps=T, dt=5.0, noise=True, noise_seed=42, every=1, runner=dict(action="oil_top_off", duration_hours=6.0),
              init_pokes=init, pokes={t: [("~" + ANCHOR, hook)] for t in range(1, T)})
    _ref, sim = trace.run_reference(sc, cols)
    hook(sim)
    sm = sim.state_manager
    fired = sorted(cid for cid in TURBINE_IDS if "efficiency" in sm.threshold_last_violation_times.get(cid, {}))
    lowest = {cid: min(v for v in seen[cid] if v is not None) for cid in TURBINE_IDS}
    orders = [o.component_id for o in list(sim.maintenance_system.work_order_manager.work_orders.values()) + list(sim.maintenance_system.work_order_manager.completed_work_orders)]
    return {"threshold": sm.maintenance_thresholds["HP-1"]["efficiency"]["threshold"], "poked": "efficiency_degradation 0.9, deposit_thickness 5.0 mm, blade_wear_factor 0.7 on all 14 stages",
            "steps": T, "lowest_efficiency_scanned": lowest, "rows_fired": fired, "orders_on_turbine_components": [c for c in orders if c in TURBINE_IDS]}


def slot_rows():
    """[(slot, component id, kind, parameter name)] of the scanned rows"""
    from nuclear_sim_amd._lib import CMAINT_PARAMS, CMAINT_NROW
    out = []
    for c, cid in enumerate(COMPONENT_IDS):
        names = [n for k, n in CMAINT_PARAMS if k == KIND_OF[c]]
        for r, n in enumerate(names):
            out.append((c * CMAINT_NROW + r, cid, KIND_OF[c], n))
    return out


def run(sc, cols):
    from oracle.ref_harness import refsim, trace
    from oracle.ref_harness.trace import _val
    T = sc["steps"]
    rows = slot_rows()
    stamps = np.full((T + 1, 12), -1.0)
    scanned = np.full((T, 12), np.nan)
    table = {}

    def record(sim, t):
        sm = sim.state_manager
        for slot, cid, _k, n in rows:
            stamps[t, slot] = sm.threshold_last_violation_times.get(cid, {}).get(n, -1.0)
        if t > 0:
            row = dict(sm.data.iloc[-1])
            for slot, cid, _k, n in rows:
                v = sm._find_parameter_in_row_data(cid, n, row)
                scanned[t - 1, slot] = np.nan if v is None else v

    def hook(t):
        def call(sim):
            if t == 0:      # another maintenance configuration: the live thresholds of the three generators and the condenser edited
                for kind, edits in sc.get("table", {}).items():
                    for cid, k in zip(COMPONENT_IDS, KIND_OF):
                        if k == kind:
                            for name, changes in edits.items():
                                sim.state_manager.maintenance_thresholds[cid][name].update(changes)
                for cid, k in zip(COMPONENT_IDS[2:], KIND_OF[2:]):
                    table[k] = [[n, {f: c.get(f) for f in ("threshold", "comparison", "action", "cooldown_hours", "priority")}]      # (pairs: the dict's order is the scan's)
                                for n, c in sim.state_manager.maintenance_thresholds[cid].items()]
            record(sim, t)
            return _val(sim, ANCHOR)      # written back as it is
        return call
    sc = dict(sc)
    pokes = {t: list(lst) for t, lst in sc.get("pokes", {}).items()}
    for t in range(T):
        pokes.setdefault(t, []).append(("~" + ANCHOR, hook(t)))
    sc["pokes"] = pokes
    ref, sim = trace.run_reference(sc, cols)
    record(sim, T)
    sc["pokes"] = {t: [(p, v) for p, v in lst if not p.startswith("~")] for t, lst in pokes.items()}
    sc["pokes"] = {t: lst for t, lst in sc["pokes"].items() if lst}
    ref["stamps"], ref["scanned"] = stamps, scanned
    ms = sim.maintenance_system
    wom = ms.work_order_manager
    orders = sorted(list(wom.work_orders.values()) + list(wom.completed_work_orders), key=lambda o: int(o.work_order_id.split("-")[1]))
    ref["orders"] = [{"work_order_id": o.work_order_id, "component_id": o.component_id, "action": o.maintenance_actions[0].action_type,
                      "priority": o.priority.name, "created": o.created_date, "planned": o.planned_start_date,
                      "completed": o.actual_completion_date, "success": None if o.actual_completion_date is None else bool(o.maintenance_actions[0].success),
                      "work_order_type": o.work_order_type.value, "title": o.title} for o in orders]
    ref["counters"] = {"work_orders_created": int(ms.work_orders_created), "maintenance_actions_performed": int(ms.maintenance_actions_performed)}
    ref["table"] = table
    ref["check_interval_minutes"] = float(ms.check_interval_hours) * 60
    # every row of the scanned components that resolves on the reference: a name outside the device's catalog must have stayed silent
    sm = sim.state_manager
    row = dict(sm.data.iloc[-1])
    silent = {}
    from nuclear_sim_amd._lib import CMAINT_PARAMS, CMAINT_ROWS_NOT_SCANNED
    for cid, kind in zip(COMPONENT_IDS, KIND_OF):
        for n in sm.maintenance_thresholds[cid]:
            if sm._find_parameter_in_row_data(cid, n, row) is not None and (kind, n) not in CMAINT_PARAMS:
                assert (kind, n) in CMAINT_ROWS_NOT_SCANNED, (cid, n)
                assert n not in sm.threshold_last_violation_times.get(cid, {}), "%s %s fired on the reference: the device does not scan it" % (cid, n)
                silent["%s:%s" % (cid, n)] = CMAINT_ROWS_NOT_SCANNED[(kind, n)]
    ref["silent"] = silent
    return ref, sim, sc


def thresholds_of(ref):
    from nuclear_sim_amd._lib import MAINT_COMPARISONS
    thr, cmp_ = np.full(12, np.nan), np.full(12, -1, dtype=np.int64)
    for slot, _cid, kind, n in slot_rows():
        c = dict(ref["table"][kind]).get(n)
        if c is not None and c.get("threshold") is not None:
            thr[slot] = c["threshold"]; cmp_[slot] = MAINT_COMPARISONS.index(c.get("comparison", "greater_than"))
    return thr, cmp_


def check(sc, ref):
    """what the tests rely on (tests/test_auto_component_fixtures.py re-asserts it on the committed files)"""
    thr, _ = thresholds_of(ref)
    d = np.abs(ref["scanned"] - thr[None, :]) / np.abs(thr[None, :])
    worst = np.nanmin(d)
    assert worst >= MARGIN, "%s: a scanned value comes within %.3g (relative) of its threshold, column %d step %d" % (
        sc["name"], worst, np.nanargmin(np.nanmin(d, axis=0)), np.nanargmin(np.nanmin(d, axis=1)))
    assert not ref["done"].any(), "the plant trips in this scenario"
    done = [o for o in ref["orders"] if o["completed"] is not None]
    assert ref["counters"]["work_orders_created"] == len(ref["orders"]) and ref["counters"]["maintenance_actions_performed"] == len(done)
    return worst


def meta_of(sc):
    from oracle.ref_harness import trace
    meta = {k: v for k, v in sc.items() if not callable(v) and k not in ("pokes", "init_pokes", "table")}
    meta["resets"] = {}
    meta["pokes"] = {str(k): [[p, trace.poke_number(v)] for p, v in lst] for k, lst in sc.get("pokes", {}).items()}
    meta["pokes_schema"] = meta["pokes"]
    meta["init_pokes"] = [[p, trace.poke_number(v)] for p, v in sc.get("init_pokes", [])]
    meta["table_edits"] = sc.get("table", {})
    return meta


def main(argv):
    from nuclear_sim_amd.schema import SCHEMA
    explore, checking = "--explore" in argv, "--check" in argv
    names = [a for a in argv if not a.startswith("--")]
    cols = SCHEMA.columns()
    if "--turbine" in argv:
        print(json.dumps(turbine_probe(cols), indent=1))
        return
    os.makedirs(OUT, exist_ok=True)
    for sc0 in scenarios():
        if names and sc0["name"] not in names:
            continue
        ref, _sim, sc = run(sc0, cols)
        if explore:
            print(sc["name"], ref["counters"], "done", int(ref["done"].sum()))
            for o in ref["orders"]:
                print("   %(work_order_id)s %(component_id)-24s %(action)-32s %(priority)-9s created %(created)6.1f planned %(planned)6.1f completed %(completed)s success %(success)s" % o)
            thr, _ = thresholds_of(ref)
            d = np.abs(ref["scanned"] - thr[None, :]) / np.abs(thr[None, :])
            print("   closest approach to a threshold (relative):", np.nanmin(d), " silent:", list(ref["silent"]))
            for slot, cid, _k, n in slot_rows():
                print("   %-24s %-22s min %.6g max %.6g stamps %s" % (cid, n, np.nanmin(ref["scanned"][:, slot]), np.nanmax(ref["scanned"][:, slot]),
                                                                      sorted(set(ref["stamps"][:, slot]) - {-1.0})))
            continue
        worst = check(sc, ref)
        T = sc["steps"]
        steps = list(range(0, T + 1, sc.get("every", 1)))
        thr, cmp_ = thresholds_of(ref)
        arrays = dict(action=ref["action"], magnitude=ref["magnitude"], setpoint=ref["setpoint"], cooling=ref["cooling"],
                      noise_z=ref["noise_z"], obs=ref["obs"], reward=ref["reward"], done=ref["done"], info=ref["info"],
                      state_steps=np.array(steps), sec_keys=ref["sec_keys"], sec=ref["sec"], rc_keys=ref["rc_keys"], rc=ref["rc"],
                      state=ref["state"][steps], labels=np.array([c[2] for c in cols]), kinds=np.array([c[0] for c in cols]),
                      paths=np.array([c[3] for c in cols]), meta=json.dumps(meta_of(sc)), stamps=ref["stamps"], scanned=ref["scanned"],
                      thresholds=thr, comparisons=cmp_)
        side = {"scenario": sc["name"], "orders": ref["orders"], "counters": ref["counters"], "table": ref["table"], "silent": ref["silent"],
                "check_interval_minutes": ref["check_interval_minutes"], "margin": MARGIN, "closest_approach": float(worst)}
        path = os.path.join(OUT, sc["name"] + ".npz")
        if checking:
            z = np.load(path, allow_pickle=False)
            for k in ("obs", "state", "stamps", "scanned", "noise_z", "setpoint"):
                np.testing.assert_array_equal(z[k], arrays[k], err_msg="%s: %s" % (sc["name"], k))
            assert json.load(open(path[:-4] + ".json")) == json.loads(json.dumps(side)), sc["name"]
            print(sc["name"], "matches the committed fixture")
            continue
        np.savez_compressed(path, **arrays)
        with open(path[:-4] + ".json", "w") as f:
            json.dump(side, f, indent=1, sort_keys=True)
        print(sc["name"], "steps", T, "orders", len(ref["orders"]), "closest approach %.3g" % worst, os.path.getsize(path), "bytes ->", os.path.relpath(path, ROOT))
    if not names and not explore and not checking:
        with open(os.path.join(OUT, "silent_rows.json"), "w") as f:
            json.dump({"default_table_rows_silent": SILENT_DEFAULT_ROWS, "turbine_efficiency_probe": turbine_probe(cols)}, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv[1:])
