"""Reference fixtures for operator-ordered maintenance: tests/golden/operator/om*.npz.

Drives REFERENCE simulators (oracle/ref_harness: refsim, trace.run_reference; needs a machine with the reference) with a script of
``pump.perform_maintenance(type, **kwargs)`` / ``pump.lubrication_system.perform_maintenance(type, **kwargs)`` calls placed BETWEEN
steps, and records, in the layout of the trajectory fixtures (oracle/ref_harness/make_golden.py) plus:

  ops[K, 6]                  (step, pump 0..3, action index, bearing NPB_BEARING_*, target_level or NaN, success) of every call, in call
                             order; ``step`` = t: the call is made after t steps, before step t (the plant's clock is t * dt)
  op_before[K, ncol_pump]    the reference's value of every schema column of that pump's section immediately before the call ...
  op_after[K, ncol_pump]     ... and immediately after it, so that the handler's effect is pinned apart from the next step's
  op_labels[ncol_pump]       the member names of those columns (schema label "pump[k].<member>")
  op_expect_change[K]        1 = the call changes plant state by construction of the scenario, 0 = it changes none (no handler, a
                             read-only analysis, the "does nothing" side of a conditional handler)

trace.run_reference applies a step's pokes before that step and accepts a callable as a poke's value: the calls ride on that (the
"poke" writes a member back with the value it has).  The files go into a sub-directory because every existing replay test
parametrises over tests/golden/*.npz and would replay them without their calls.

    python tools/make_operator_maintenance_golden.py [scenario ...]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "tests", "golden", "operator")
P = "secondary_physics.feedwater_system.pump_system.pumps['FWP-%d']"
W = P + ".lubrication_system.component_wear['%s']"
L = P + ".lubrication_system.%s"
BEARINGS = {None: 0, "all": 0, "motor_bearings": 1, "pump_bearings": 2, "thrust_bearing": 3}
HANDLERS = ("oil_change", "oil_top_off", "bearing_replacement", "seal_replacement", "component_overhaul", "system_cleaning",
            "bearing_inspection", "impeller_inspection", "impeller_replacement", "lubrication_system_check", "motor_inspection",
            "oil_analysis", "vibration_analysis")


def _degraded(pump, impeller, motor, pumpb, thrust, seals, coupling, level, contamination, acidity, moisture, leakage, vibration, additives):
    return [(W % (pump, "impeller"), impeller), (W % (pump, "motor_bearings"), motor), (W % (pump, "pump_bearings"), pumpb),
            (W % (pump, "thrust_bearing"), thrust), (W % (pump, "mechanical_seals"), seals), (W % (pump, "coupling_system"), coupling),
            (L % (pump, "oil_level"), level), (L % (pump, "oil_contamination_level"), contamination), (L % (pump, "oil_acidity_number"), acidity),
            (L % (pump, "oil_moisture_content"), moisture), (L % (pump, "seal_leakage_rate"), leakage), (L % (pump, "vibration_increase"), vibration),
            (L % (pump, "antioxidant_level"), additives), (L % (pump, "anti_wear_additive_level"), additives * 0.9),
            (L % (pump, "corrosion_inhibitor_level"), additives * 0.8)]


def op(step, pump, action, expect, via="pump", **kw):
    """one call: after `step` steps, on FWP-<pump + 1>, through the pump (`via` "pump") or its lubrication system ("lube")"""
    return dict(step=step, pump=pump, action=action, expect=expect, via=via, kw=kw)


def scenarios():
    S = []
    # OM1: every handler, on running pumps (FWP-1..3) and on the spare (FWP-4, stopped), each conditional handler on both sides of its
    # condition.  FWP-1 worn throughout (impeller 8.5 > 3, motor bearings 6 > 5 > 3) with dirty, low oil; FWP-2 nearly new with a full
    # sump (nothing to inspect away, 97 % > 95 %); FWP-3 in between (impeller 2 < 3, motor bearings 3.5: > 3, < 5); FWP-4 with one worn
    # bearing (pump bearings 6.5 > 5, impeller 1 < 3).
    init = (_degraded(1, 8.5, 6.0, 4.0, 2.0, 10.0, 2.0, 70.0, 14.0, 1.5, 0.07, 0.10, 1.0, 30.0) +
            _degraded(2, 1.0, 2.0, 1.5, 1.0, 1.0, 0.5, 97.0, 9.0, 0.8, 0.03, 0.01, 0.1, 80.0) +
            _degraded(3, 2.0, 3.5, 2.5, 1.5, 6.0, 1.0, 85.0, 11.0, 1.1, 0.05, 0.05, 0.5, 50.0) +
            _degraded(4, 1.0, 2.0, 6.5, 4.0, 12.0, 3.0, 60.0, 16.0, 1.8, 0.09, 0.12, 1.5, 20.0))
    ops = [
        # the conditional handlers where they do nothing (FWP-2; FWP-3 for the two that need wear above 5 / impeller above 3)
        op(2, 1, "bearing_inspection", False), op(2, 1, "impeller_inspection", False), op(2, 1, "motor_inspection", False),
        op(2, 1, "oil_top_off", False),                                # 97 % is above the default target of 95 %
        op(3, 2, "bearing_inspection", False), op(3, 2, "impeller_inspection", False),
        op(3, 2, "motor_inspection", True),                            # motor bearings 3.5 > 3
        # ... and where they act: FWP-1 (running), FWP-4 (the spare)
        op(4, 0, "bearing_inspection", True), op(4, 3, "bearing_inspection", True),
        op(5, 0, "impeller_inspection", True),                         # impeller above 3 and bearings above 5
        op(5, 3, "impeller_inspection", True, via="lube"),             # impeller below 3, a bearing above 5
        op(6, 0, "motor_inspection", True), op(6, 3, "motor_inspection", False),      # the spare's motor bearings: 2 < 3
        # the analyses read state only; two action types the dispatcher has no handler for
        op(7, 0, "oil_analysis", False), op(7, 3, "oil_analysis", False, via="lube"),
        op(8, 0, "vibration_analysis", False), op(8, 3, "vibration_analysis", False),
        op(9, 0, "npsh_analysis", False), op(9, 3, "routine_maintenance", False),
        # top-off: default target, an explicit one, one above 100 (min(100, target)); twice on one pump between the same two steps
        op(10, 0, "oil_top_off", True), op(10, 0, "oil_top_off", True, target_level=98.0),
        op(11, 3, "oil_top_off", True, via="lube", target_level=120.0),
        op(11, 2, "oil_top_off", False, target_level=80.0),            # 85 % is above this target
        op(12, 2, "lubrication_system_check", True),                   # oil level below 95
        op(13, 1, "lubrication_system_check", True),                   # oil level above 95
        op(14, 3, "lubrication_system_check", True, via="lube"),       # the spare, now at 100 %
        # bearing replacement with each component_id
        op(16, 0, "bearing_replacement", True, component_id="motor_bearings"),
        op(17, 0, "bearing_replacement", True, component_id="pump_bearings"),
        op(18, 2, "bearing_replacement", True, component_id="thrust_bearing"),
        op(19, 3, "bearing_replacement", True, component_id="all"), op(20, 1, "bearing_replacement", True),
        op(22, 0, "impeller_inspection", True),                        # impeller above 3, every bearing now below 5
        op(24, 0, "system_cleaning", True), op(24, 3, "system_cleaning", True),
        op(26, 0, "seal_replacement", True), op(26, 3, "seal_replacement", True, via="lube"),
        op(28, 0, "impeller_replacement", True), op(28, 3, "impeller_replacement", True),
        op(32, 2, "oil_change", True), op(32, 3, "oil_change", True),
        op(36, 0, "oil_change", True, via="lube"),
        op(40, 0, "component_overhaul", True), op(40, 3, "component_overhaul", True),
        op(44, 2, "component_overhaul", True), op(44, 2, "oil_top_off", False),      # overhauled a moment ago: full
        op(50, 1, "system_cleaning", True), op(55, 1, "oil_change", True),
    ]
    S.append(dict(name="om1_every_handler", steps=60, dt=5.0, noise=True, noise_seed=42, every=1, init_pokes=init, ops=ops))
    # OM2: the data-gen runner's plant (state management and AutoMaintenanceSystem on, the thresholds of tests/golden/maint_table.json)
    # from fixture m1's oil levels: FWP-4 at 57 % has an automatic oil_top_off order from the first step; FWP-1 (58.3 %) and FWP-2
    # (58.1 %) would cross 58 % within the run.  The operator tops FWP-1 off before it gets there (its automatic order never appears) and
    # changes FWP-4's oil while its order is open (the order still executes at its time)
    S.append(dict(name="om2_with_automatic_maintenance", steps=48, dt=5.0, noise=True, noise_seed=42, every=1,
                  runner=dict(action="oil_top_off", duration_hours=4.0, feedwater_ic={"pump_oil_levels": [58.3, 58.1, 98.0, 57.0]}),
                  ops=[op(1, 3, "oil_change", True), op(2, 0, "oil_top_off", True), op(30, 2, "npsh_analysis", False)]))
    return S


def run(sc, cols, actions):
    from oracle.ref_harness import refsim, trace
    from oracle.ref_harness.trace import _val
    labels = [c[2] for c in cols]
    members = [lab[len("pump[0]."):] for lab in labels if lab.startswith("pump[0].")]
    pump_paths = [[cols[labels.index("pump[%d].%s" % (k, m))][3] for m in members] for k in range(4)]
    rows, before, after = [], [], []
    anchor = L % (1, "oil_level")
    by_step = {}
    for o in sc["ops"]:
        by_step.setdefault(o["step"], []).append(o)

    def hook(step):
        def call(sim):
            for o in by_step[step]:
                pump = sim.secondary_physics.feedwater_system.pump_system.pumps["FWP-%d" % (o["pump"] + 1)]
                target = pump if o["via"] == "pump" else pump.lubrication_system
                before.append([_val(sim, p) for p in pump_paths[o["pump"]]])
                with refsim.quiet():
                    res = target.perform_maintenance(o["action"], **o["kw"])
                after.append([_val(sim, p) for p in pump_paths[o["pump"]]])
                rows.append((o["step"], o["pump"], actions.index(o["action"]), BEARINGS[o["kw"].get("component_id")],
                             o["kw"].get("target_level", np.nan), float(bool(res["success"]))))
            return _val(sim, anchor)      # written back as it is
        return call
    sc = dict(sc)
    assert not sc.get("pokes")
    sc["pokes"] = {step: [("~" + anchor, hook(step))] for step in by_step}
    ref, sim = trace.run_reference(sc, cols)
    ref["ops"] = np.array(rows, dtype=np.float64)
    ref["op_before"], ref["op_after"] = np.array(before, dtype=np.float64), np.array(after, dtype=np.float64)
    ref["op_labels"] = np.array(members)
    ref["op_expect_change"] = np.array([int(bool(o["expect"])) for o in sc["ops"]], dtype=np.int8)
    return ref, sim


def check(sc, ref, cols, actions, handlers):
    """what keeps the fixture from being vacuous (tests/test_operator_maintenance_abi.py re-asserts it on the committed file)"""
    ops, b, a = ref["ops"], ref["op_before"], ref["op_after"]
    assert len(ops) == len(sc["ops"])
    for j, o in enumerate(sc["ops"]):
        changed = ~((b[j] == a[j]) | (np.isnan(b[j]) & np.isnan(a[j])))
        want_success = o["action"] in handlers and o["kw"].get("component_id") in BEARINGS
        assert bool(ops[j, 5]) == want_success, (j, o, ops[j])
        assert changed.any() == bool(o["expect"]), "%s op %d %r: columns changed %s" % (sc["name"], j, o, list(ref["op_labels"][changed]))
    labels = [c[2] for c in cols]
    if sc["name"].startswith("om1"):
        seen = {(o["action"], o["pump"] == 3) for o in sc["ops"]}
        for h in handlers:
            assert (h, False) in seen and (h, True) in seen, h
        assert {o["kw"].get("component_id") for o in sc["ops"] if o["action"] == "bearing_replacement"} >= {None, "all", "motor_bearings", "pump_bearings", "thrust_bearing"}
    if sc["name"].startswith("om2"):
        st = ref["state"]
        top_off = actions.index("oil_top_off")
        wo = lambda k: st[:, labels.index("mpump[%d].wo_order[%d]" % (k, top_off))]
        assert wo(3)[1] > 0, "FWP-4 has no open automatic order when the operator changes its oil"
        assert (wo(3)[2:] == 0).any(), "FWP-4's automatic order never executes"
        assert (wo(0) == 0).all(), "FWP-1 got an automatic order although the operator topped it off"
        assert (wo(1) > 0).any(), "FWP-2, left alone, never got its automatic order"


def main(names):
    from nuclear_sim_amd.schema import SCHEMA
    from nuclear_sim_amd._lib import MAINT_ACTION_NAMES
    from oracle.ref_harness import trace
    actions = list(MAINT_ACTION_NAMES)
    cols = SCHEMA.columns()
    os.makedirs(OUT, exist_ok=True)
    for sc in scenarios():
        if names and sc["name"] not in names:
            continue
        ref, _sim = run(sc, cols, actions)
        check(sc, ref, cols, actions, HANDLERS)
        T = sc["steps"]
        steps = list(range(0, T + 1, sc.get("every", 1)))
        meta = {k: v for k, v in sc.items() if not callable(v) and k not in ("pokes", "init_pokes", "ops", "_maint_thresholds", "_maint_params")}
        if sc.get("_maint_thresholds"):
            meta["maint_thresholds"] = sc["_maint_thresholds"]
        if sc.get("_maint_params"):
            meta["maint_params"] = sc["_maint_params"]
        meta["resets"] = {}
        meta["pokes"] = {}
        meta["pokes_schema"] = {}
        meta["init_pokes"] = [[p, trace.poke_number(v)] for p, v in sc.get("init_pokes", [])]
        meta["ops"] = [dict(step=o["step"], pump=o["pump"], action=o["action"], via=o["via"], kwargs=o["kw"]) for o in sc["ops"]]
        path = os.path.join(OUT, sc["name"] + ".npz")
        np.savez_compressed(path, action=ref["action"], magnitude=ref["magnitude"], setpoint=ref["setpoint"], cooling=ref["cooling"],
                            noise_z=ref["noise_z"], obs=ref["obs"], reward=ref["reward"], done=ref["done"], info=ref["info"],
                            state_steps=np.array(steps), sec_keys=ref["sec_keys"], sec=ref["sec"], rc_keys=ref["rc_keys"], rc=ref["rc"],
                            state=ref["state"][steps], labels=np.array([c[2] for c in cols]), kinds=np.array([c[0] for c in cols]),
                            paths=np.array([c[3] for c in cols]), meta=json.dumps(meta), ops=ref["ops"], op_before=ref["op_before"],
                            op_after=ref["op_after"], op_labels=ref["op_labels"], op_expect_change=ref["op_expect_change"])
        print(sc["name"], "steps", T, "ops", len(ref["ops"]), "successful", int(ref["ops"][:, 5].sum()), os.path.getsize(path), "bytes ->",
              os.path.relpath(path, ROOT))


if __name__ == "__main__":
    main(sys.argv[1:])
