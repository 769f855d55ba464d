"""Reference fixtures for operator-ordered maintenance of the turbine: tests/golden/operator_turbine/ot*.npz.

Drives REFERENCE simulators (oracle/ref_harness; needs a machine with the reference) with a script of ``perform_maintenance(type)`` calls
on the turbine (EnhancedTurbinePhysics), one of its four bearings, its bearing-lubrication system or one of its fourteen stages, placed
BETWEEN steps, in the layout of tests/golden/operator_components/oc*.npz (tools/make_component_maintenance_golden.py, whose helpers this
generator uses):

  ops[K, 8]            (step, turbine kind of the object called, unit, catalog index, 0, NaN, success, -1) of every call, in call order;
                       catalog index = position in _lib.TURBINE_ACTIONS, len(TURBINE_ACTIONS) for a type outside it (unknown, or refused);
                       success of a stage's call: the stage's handler returns a dict without a "success" key -- 1 for its three types, 0
                       for any other (which does nothing)
  op_before / op_after [K, ncol]   the reference's value of every schema column of turb.* and tstg.* immediately before / after the call
  op_labels[ncol]      their schema labels
  op_expect_change[K]  1 = the call changes carried state by construction of the scenario
  op_closed[K]         the CLOSURE check of that call on the live reference (the component generator's docstring): simulator A makes the
                       call; a fresh simulator B with the same history does not, but has every schema member the call moved poked to A's
                       value; 1 = every schema column and observation of A and B is equal to the bit after each of the next 8 steps

Every CANDIDATE type of the four dispatchers is called, catalogued or not: a candidate whose calls are not all closed is not offered
(_lib.TURBINE_ACTIONS_NOT_OFFERED) and meta["refused"] records the first difference the check saw.

The turbine's latched trip reasons are one schema column (turb.trip_latched_mask, "=H.turbine_trip_mask(root)"); a poke of it is applied
to the reference as the list of reasons the mask stands for.

    python tools/make_turbine_maintenance_golden.py [--explore [--all-candidates]] [scenario ...]

--explore prints the closure result per call and writes nothing.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from make_component_maintenance_golden import CLOSURE_STEPS, same      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "operator_turbine")
SECTIONS = ("turb.", "tstg.")
KINDS = ("turbine", "bearing", "lubrication", "stage")
UNITS = {"turbine": 1, "bearing": 4, "lubrication": 1, "stage": 14}
TURB = "secondary_physics.turbine.%s"
BEARING = "=list(root.secondary_physics.turbine.rotor_dynamics.bearings.values())[%d].%s"
LUB = "secondary_physics.turbine.bearing_lubrication_system.%s"
LUB_WEAR = "=list(root.secondary_physics.turbine.bearing_lubrication_system.component_wear.values())[%d]"
STAGE = "=list(root.secondary_physics.turbine.stage_system.stages.values())[%d].%s"
PROT = "secondary_physics.turbine.protection_system.%s"
MASK = "=H.turbine_trip_mask(root)"
THRUST = 2          # rotor_dynamics.py:829: the third bearing is the thrust bearing
ALL_CANDIDATES = False      # --all-candidates: keep the calls of what is not offered in OT1-OT4 (to explore the closure of every candidate)

# every maintenance type the four dispatchers name (enhanced_physics.py:1055-1267, rotor_dynamics.py:381-564,
# turbine_bearing_lubrication.py:481-668, stage_system.py:341-377)
CANDIDATES = tuple(
    [("turbine", a) for a in ("turbine_performance_test", "turbine_system_optimization", "turbine_protection_test", "thermal_stress_analysis",
                              "vibration_analysis", "routine_maintenance")] +
    [("bearing", a) for a in ("turbine_bearing_inspection", "turbine_bearing_replacement", "bearing_clearance_check", "bearing_alignment",
                              "thrust_bearing_adjustment", "turbine_oil_change", "routine_maintenance")] +
    [("lubrication", a) for a in ("turbine_oil_change", "turbine_oil_top_off", "oil_filter_replacement", "oil_cooler_cleaning",
                                  "lubrication_system_test", "routine_maintenance")] +
    [("stage", a) for a in ("cleaning", "blade_replacement", "overhaul")])


def bearings(wear=None, temp=None):
    out = []
    for k in range(4):
        if wear is not None:
            out.append((BEARING % (k, "wear_factor"), wear[k]))
        if temp is not None:
            out.append((BEARING % (k, "metal_temperature"), temp[k]))
    return out


def oil(contamination=None, acidity=None, moisture=None, temperature=None, effectiveness=None, wear=None):
    out = []
    for name, v in (("oil_contamination_level", contamination), ("oil_acidity_number", acidity), ("oil_moisture_content", moisture),
                    ("oil_temperature", temperature), ("lubrication_effectiveness", effectiveness)):
        if v is not None:
            out.append((LUB % name, v))
    for k, w in enumerate(wear or ()):
        out.append((LUB_WEAR % k, w))
    return out


def stages(scale=1.0):
    """fourteen stages in different conditions: deposits, blade wear and efficiency degradation growing towards the exhaust"""
    out = []
    for k in range(14):
        out += [(STAGE % (k, "deposit_thickness"), scale * 0.02 * (k + 1)), (STAGE % (k, "blade_wear_factor"), 1.0 - scale * 0.004 * (k + 1)),
                (STAGE % (k, "efficiency_degradation"), scale * 0.003 * (k + 2))]
    return out


def trip(active, mask, timers=(0.0, 0.0, 0.0)):
    return [(PROT % "trip_active", bool(active)), (MASK, mask), (PROT % "trip_timers['overspeed']", timers[0]),
            (PROT % "trip_timers['vibration']", timers[1]), (PROT % "trip_timers['bearing_temp']", timers[2])]


def op(step, comp, unit, action, expect):
    """one call: after `step` steps, perform_maintenance(action) on unit `unit` of turbine kind `comp`"""
    return dict(step=step, comp=comp, unit=unit, action=action, expect=expect)


def scenarios():
    S = []
    tb, br, lu, st = KINDS
    system = [a for k, a in CANDIDATES if k == tb]
    bearing = [a for k, a in CANDIDATES if k == br]
    lube = [a for k, a in CANDIDATES if k == lu]
    # OT1: a degraded turbine -- worn and warm bearings, dirty oil, a bowed rotor.  The members a handler caps or floors are poked to
    # either side of the cap before the calls that read them (the step moves them by itself).
    init = bearings(wear=(0.9, 0.85, 0.8, 0.95), temp=(95.0, 100.0, 105.0, 92.0)) + \
        oil(contamination=12.0, acidity=0.4, moisture=0.05, temperature=60.0, effectiveness=0.7, wear=(12.0, 8.0, 3.0, 0.3, 20.0)) + \
        [(TURB % "rotor_dynamics.thermal_bow", 0.02)]
    ops = [op(2, tb, 0, a, a in ("vibration_analysis", "routine_maintenance", "turbine_system_optimization", "turbine_protection_test")) for a in system]      # the plant's thrust-displacement trip is active
    ops += [op(4, tb, 0, "turbine_protection_test", False),                    # no trip active: nothing is reset, the latched mask stays
            op(6, tb, 0, "turbine_protection_test", True),                     # a trip active: reset_protection_system
            op(8, tb, 0, "routine_maintenance", True),                         # bearings at 80.2 / 80.5 / 81 / 79: max(80, T - 0.5) from both sides
            op(8, tb, 0, "turbine_system_optimization", False),                # effectiveness already 1: min(1, e + 0.05) is e
            op(9, tb, 0, "vibration_analysis", True), op(9, tb, 0, "vibration_analysis", True)]      # twice between the same two steps
    # every bearing type on every bearing over steps 11-17 (the thrust adjustment: success on the third only)
    for k, a in enumerate(bearing):
        for b in range(4):
            moves = a in ("turbine_bearing_replacement", "turbine_oil_change", "routine_maintenance") or (a == "thrust_bearing_adjustment" and b == THRUST)
            ops.append(op(11 + k, br, b, a, moves))
    ops += [op(19, br, 0, "turbine_bearing_replacement", True),                # 85 C: min(T, 90) keeps it; wear 0.9 -> 1
            op(19, br, 1, "turbine_bearing_replacement", True),                # 97 C: capped to 90
            op(20, br, THRUST, "thrust_bearing_adjustment", True),             # 83 C: max(80, T - 5) floors at 80
            op(20, br, THRUST, "thrust_bearing_adjustment", False),            # 80 C already
            op(20, br, 0, "thrust_bearing_adjustment", False),                 # a journal bearing: refused by the handler
            op(21, br, 1, "turbine_oil_change", True), op(21, br, 1, "routine_maintenance", True)]
    ops += [op(23, lu, 0, a, a != "turbine_oil_top_off") for a in lube]
    ops += [op(24, lu, 0, "routine_maintenance", True),                        # dirty, warm oil and worn components: nothing is floored
            op(25, lu, 0, "oil_filter_replacement", True),                     # contamination 12: min(5, 0.6 c) caps at 5
            op(26, lu, 0, "oil_filter_replacement", True),                     # 4: 0.6 c
            op(27, lu, 0, "oil_filter_replacement", True),                     # 1.5: floored at 1
            op(28, lu, 0, "turbine_oil_change", True),                         # effectiveness 0.7 / oil at 60 C
            op(29, lu, 0, "turbine_oil_change", True),                         # effectiveness 0.95: capped; oil at 47 C: floored at 45
            op(30, lu, 0, "lubrication_system_test", True), op(30, lu, 0, "lubrication_system_test", True),
            op(31, lu, 0, "routine_maintenance", True),                        # wear 0.3 of the fourth component: floored at 0; contamination 1.2: floored at 1
            op(32, lu, 0, "oil_cooler_cleaning", True),                        # oil-cooler wear (the fifth component) 20 -> 15
            op(33, lu, 0, "oil_cooler_cleaning", True),                        # 3 -> floored at 0
            op(34, lu, 0, "turbine_oil_top_off", False),                       # level 100: nothing is added, max(1, c - 0) and max(0.05, a - 0) keep c and a
            op(35, lu, 0, "turbine_oil_top_off", True),                        # ... and floor a contamination of 0.8 at 1, an acidity of 0.03 at 0.05
            op(36, tb, 0, "bogus_maintenance", False), op(36, br, 1, "bogus_maintenance", False), op(36, lu, 0, "bogus_maintenance", False),
            op(36, st, 3, "bogus_maintenance", False)]
    pokes = {4: trip(False, 2), 6: trip(True, 2 | 4, (0.0, 300.0, 300.0)),
             8: bearings(temp=(80.2, 80.5, 81.0, 79.0)) + oil(effectiveness=1.0),
             9: [(TURB % "rotor_dynamics.thermal_bow", 0.03)],
             11: bearings(wear=(0.9, 0.85, 0.8, 0.95), temp=(95.0, 100.0, 105.0, 92.0)),
             19: bearings(wear=(0.9, 0.85, 0.8, 0.95), temp=(85.0, 97.0, 83.0, 92.0)), 20: bearings(temp=(85.0, 97.0, 83.0, 92.0)),
             23: oil(contamination=12.0, acidity=0.4, moisture=0.05, temperature=60.0, effectiveness=0.7),
             24: oil(contamination=6.0, temperature=55.0, effectiveness=0.6, wear=(12.0, 8.0, 3.0, 0.8, 20.0)),
             25: oil(contamination=12.0), 26: oil(contamination=4.0), 27: oil(contamination=1.5),
             28: oil(contamination=9.0, acidity=0.3, moisture=0.04, temperature=60.0, effectiveness=0.7),
             29: oil(contamination=9.0, acidity=0.3, moisture=0.04, temperature=47.0, effectiveness=0.95),
             30: oil(effectiveness=0.85), 31: oil(contamination=1.2, temperature=45.5, effectiveness=0.99, wear=(12.0, 8.0, 3.0, 0.3, 20.0)),
             32: oil(temperature=58.0, wear=(12.0, 8.0, 3.0, 0.3, 20.0)), 33: oil(wear=(12.0, 8.0, 3.0, 0.3, 3.0)),
             34: oil(contamination=8.0, acidity=0.3), 35: oil(contamination=0.8, acidity=0.03)}
    S.append(dict(name="ot1_degraded_turbine", steps=46, dt=5.0, noise=True, noise_seed=42, every=1, init_pokes=init, pokes=pokes, ops=ops))
    # OT2: the stages.  Every stage at least once with each type, on a fouled blade path and (late) on stages already clean.
    ops = []
    for k in range(14):
        ops.append(op(2 + k // 4, st, k, ("cleaning", "blade_replacement", "overhaul")[k % 3], True))
    for k in range(14):
        ops.append(op(8 + k // 4, st, k, ("blade_replacement", "overhaul", "cleaning")[k % 3], True))
    ops += [op(13, st, 5, "blade_replacement", True), op(13, st, 5, "overhaul", True),      # two calls on one stage between the same two steps
            op(14, st, 13, "overhaul", True), op(14, st, 0, "overhaul", True),
            op(15, st, 14, "overhaul", False), op(15, br, 4, "routine_maintenance", False),  # a stage / a bearing that does not exist
            op(16, st, 2, "inspection", False)]
    S.append(dict(name="ot2_stages", steps=26, dt=5.0, noise=True, noise_seed=42, every=1, init_pokes=stages(), pokes={8: stages(0.5), 13: stages(0.7)}, ops=ops))
    # OT3: every candidate on the AS-BUILT turbine (what a handler does to a plant that needs nothing)
    ops = []
    t = 2
    for j, (kind, a) in enumerate(CANDIDATES):
        ops.append(op(t + j // 4, kind, {tb: 0, br: j % 4, lu: 0, st: (5 * j) % 14}[kind], a, None))
    S.append(dict(name="ot3_as_built", steps=18, dt=5.0, noise=True, noise_seed=42, every=1, init_pokes=[], pokes={}, ops=ops))
    # OT4: the data-gen runner's plant (state management and AutoMaintenanceSystem on, thresholds of the feedwater pumps only) from
    # fixture m1's oil levels: the automatic top-off runs beside the operator's work on a degraded turbine
    S.append(dict(name="ot4_long_run", steps=48, dt=5.0, noise=True, noise_seed=42, every=1, feedwater_thresholds_only=True,
                  runner=dict(action="oil_top_off", duration_hours=4.0, feedwater_ic={"pump_oil_levels": [58.3, 58.1, 98.0, 57.0]}),
                  init_pokes=stages() + bearings(wear=(0.9, 0.85, 0.8, 0.95)) + oil(contamination=12.0, acidity=0.4, effectiveness=0.7),
                  pokes={},
                  ops=[op(8, st, 6, "overhaul", True), op(8, st, 13, "blade_replacement", True), op(12, br, 1, "turbine_bearing_replacement", True),
                       op(12, lu, 0, "turbine_oil_change", True), op(20, tb, 0, "routine_maintenance", True), op(24, br, THRUST, "thrust_bearing_adjustment", True)]))
    # what is NOT offered leaves OT1-OT4, which the device replays call by call, and gets a fixture of its own that records what the
    # reference does and that the call is not closed: each refused candidate on a degraded unit and on an as-built one
    from nuclear_sim_amd import _lib
    refused = [k for k in CANDIDATES if k in getattr(_lib, "TURBINE_ACTIONS_NOT_OFFERED", {})]
    if refused and not ALL_CANDIDATES:
        for sc in S:
            sc["ops"] = [o for o in sc["ops"] if (o["comp"], o["action"]) not in refused]
        ops = []
        for j, (kind, a) in enumerate(refused):
            ops += [op(2 + 4 * j, kind, 2 % UNITS[kind], a, True), op(4 + 4 * j, kind, 10 % UNITS[kind], a, None)]
        init = [p for p in stages() + bearings(wear=(0.9, 0.85, 0.8, 0.95)) + oil(contamination=12.0, acidity=0.4, effectiveness=0.7)
                if not p[0].startswith(STAGE.split("%")[0]) or int(p[0][len(STAGE.split("%")[0]):p[0].index("]")]) < 7]
        S.append(dict(name="ot5_not_offered", steps=4 * len(refused) + 10, dt=5.0, noise=True, noise_seed=42, every=1, init_pokes=init, pokes={}, ops=ops))
    return S


def target_of(sim, o):
    t = sim.secondary_physics.turbine
    if o["comp"] == "turbine":
        return t
    if o["comp"] == "bearing":
        return list(t.rotor_dynamics.bearings.values())[o["unit"]]
    if o["comp"] == "lubrication":
        return t.bearing_lubrication_system
    return list(t.stage_system.stages.values())[o["unit"]]


def success_of(o, res):
    if o["comp"] == "stage":
        return bool(res)          # {} for a type the stage does not know
    return bool(res["success"])


def install_mask_poke():
    """a poke of turb.trip_latched_mask sets TurbineProtectionSystem.trip_reasons to the reasons the mask stands for, in the order of the checks"""
    from oracle.ref_harness import trace
    from oracle.ref_harness.leaves import H
    if getattr(trace._poke, "_turbine_mask", False):
        return
    plain = trace._poke

    def poke(sim, path, v):
        turbine = sim.secondary_physics.turbine
        if path == MASK:
            turbine.protection_system.trip_reasons = [r for r, bit in H.TURBINE_TRIP_BITS.items() if int(v) & bit]
        elif path.startswith(LUB_WEAR.split("%")[0]):
            wear = turbine.bearing_lubrication_system.component_wear      # list(d.values())[k] = v would assign to a temporary
            wear[list(wear)[int(path[len(LUB_WEAR.split("%")[0]):-1])]] = v
        else:
            plain(sim, path, v)
        if path.startswith(STAGE.split("%")[0]):
            # the three factors a stage derives from its carried members at the end of every step and reads at the start of the next
            # (stage_system.py:313, 321, 325; 221-224): the device derives them from the carried members when it reads them, so a
            # poke of a carried member carries them along
            s = list(turbine.stage_system.stages.values())[int(path[len(STAGE.split("%")[0]):path.index("]")])]
            s.fouling_factor = 1.0 / (1.0 + s.deposit_thickness / 0.5)
            s.blade_condition_factor = min(s.fouling_factor, s.blade_wear_factor)
            s.actual_efficiency = max(getattr(s.config, 'min_stage_efficiency', 0.7), s.config.design_efficiency - s.efficiency_degradation)
    poke._turbine_mask = True
    trace._poke = poke


def run(sc, cols, catalog, poke_instead=None, explore=False):
    """the scenario on a fresh reference simulator.  poke_instead = (j, column indices, values): call j is NOT made; the schema members it
    moved in the run that made it are poked to the values they had after it (the closure check's simulator B)"""
    from oracle.ref_harness import refsim, trace
    from oracle.ref_harness.trace import _val
    install_mask_poke()
    labels = [c[2] for c in cols]
    paths = [c[3] for c in cols]
    inside = np.array([lab.startswith(SECTIONS) for lab in labels])
    sel = np.nonzero(inside)[0]
    rows, before, after, moved_outside = [], [], [], []
    anchor = "secondary_physics.turbine.load_demand"
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
                        old = 0 if paths[c] == MASK else trace.resolve(sim, paths[c])
                        trace._poke(sim, paths[c], bool(v) if isinstance(old, (bool, np.bool_)) else int(v) if isinstance(old, (int, np.integer)) else float(v))
                    success = np.nan
                elif o["unit"] >= UNITS[o["comp"]]:
                    success = 0.0          # no such object in the reference: there is nothing to call
                else:
                    with refsim.quiet():
                        res = target_of(sim, o).perform_maintenance(o["action"])
                    success = float(success_of(o, res))
                a = np.array([_val(sim, p) for p in paths])
                moved = ~same(b, a)
                moved_outside.append([labels[c] for c in np.nonzero(moved & ~inside)[0]])
                before.append(b); after.append(a)
                key = (o["comp"], o["action"])
                index = catalog.index(key) if key in catalog else len(catalog)
                rows.append((o["step"], KINDS.index(o["comp"]), o["unit"], index, 0, np.nan, success, -1))
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
        else:
            twin, _sim, _sc = run(sc0, cols, catalog, poke_instead=(j, moved, ref["full_after"][j][moved]), explore=explore)
            for k in range(t + 1, min(t + CLOSURE_STEPS, sc0["steps"]) + 1):
                eq = same(ref["state"][k], twin["state"][k])
                if not eq.all() or not same(ref["obs"][k - 1], twin["obs"][k - 1]).all():
                    what = "after step %d (%d after the call): %s" % (k - 1, k - t, [labels[c] for c in np.nonzero(~eq)[0][:4]] or "obs")
                    break
        closed.append(int(not what)); why.append(what)
        if explore:
            print("  %-3d %-12s %2d %-30s success %s moved %-3d closed %d %s" % (
                t, o["comp"], o["unit"], o["action"], ref["ops"][j, 6], len(moved), closed[-1], what), flush=True)
    ref["op_closed"] = np.array(closed, dtype=np.int8)
    ref["op_why"] = why


def check(sc, ref, catalog):
    """what keeps the fixture from being vacuous (tests/test_turbine_maintenance_fixtures.py re-asserts it on the committed files)"""
    ops, b, a = ref["ops"], ref["op_before"], ref["op_after"]
    assert len(ops) == len(sc["ops"])
    for j, o in enumerate(sc["ops"]):
        changed = ~same(b[j], a[j])
        if o["expect"] is not None and ops[j, 3] < len(catalog):
            assert changed.any() == bool(o["expect"]), "%s op %d %r: columns changed %s" % (sc["name"], j, o, list(ref["op_labels"][changed]))
        if ops[j, 3] < len(catalog):
            kind, name = catalog[int(ops[j, 3])]
            want = 0 <= ops[j, 2] < UNITS[kind] and not (name == "thrust_bearing_adjustment" and ops[j, 2] != THRUST)
            assert ops[j, 6] == float(want), (j, o)
            assert ref["op_closed"][j] == 1, "%s op %d %r is not closed: %s" % (sc["name"], j, o, ref["op_why"][j])
            if not want:
                assert not changed.any(), (j, o)
        elif (o["comp"], o["action"]) not in CANDIDATES:
            assert ops[j, 6] == 0.0 and not changed.any(), (j, o)
    assert not ref["done"].any(), "the plant trips in this scenario"
    assert max(o["step"] for o in sc["ops"]) + CLOSURE_STEPS <= sc["steps"]


def main(argv):
    from nuclear_sim_amd.schema import SCHEMA
    from nuclear_sim_amd import _lib
    from oracle.ref_harness import trace
    global ALL_CANDIDATES
    explore = "--explore" in argv
    ALL_CANDIDATES = "--all-candidates" in argv
    assert explore or not ALL_CANDIDATES
    names = [a for a in argv if not a.startswith("--")]
    catalog = list(getattr(_lib, "TURBINE_ACTIONS", CANDIDATES))
    cols = SCHEMA.columns()
    os.makedirs(OUT, exist_ok=True)
    seen = set()
    failed = {}          # candidate -> the first difference a call of it showed
    results = []
    for sc in scenarios():
        if names and sc["name"] not in names:
            continue
        if explore:
            print(sc["name"], flush=True)
        sc0 = sc
        ref, _sim, sc = run(sc0, cols, catalog, explore=explore)
        ref["op_expect_change"] = np.array([int(bool(o["expect"])) if o["expect"] is not None else
                                            int((~same(ref["op_before"][j], ref["op_after"][j])).any()) for j, o in enumerate(sc["ops"])], dtype=np.int8)
        closure(sc0, ref, cols, catalog, explore)
        seen |= {int(r[3]) for r in ref["ops"] if r[3] < len(catalog)}
        for j, o in enumerate(sc["ops"]):
            if not ref["op_closed"][j] and (o["comp"], o["action"]) in CANDIDATES:
                failed.setdefault("%s:%s" % (o["comp"], o["action"]), "%s call %d: %s" % (sc["name"], j, ref["op_why"][j]))
        if explore:
            print("  done:", int(ref["done"].sum()), "expect mismatches:",
                  [j for j, o in enumerate(sc["ops"]) if o["expect"] is not None and (~same(ref["op_before"][j], ref["op_after"][j])).any() != bool(o["expect"])])
            continue
        check(sc, ref, catalog)
        t = _sim.secondary_physics.turbine      # the ids the maintenance log names the objects by, from the live objects
        ref["component_ids"] = dict(turbine=[t.config.system_id], bearing=list(t.rotor_dynamics.bearings), lubrication=[t.bearing_lubrication_system.config.system_id],
                                    stage=list(t.stage_system.stages), thrust=[k for k, b in t.rotor_dynamics.bearings.items() if b.config.bearing_type == "thrust"],
                                    lubrication_components=list(t.bearing_lubrication_system.component_wear),
                                    oil_level=float(t.bearing_lubrication_system.oil_level), oil_cooling_effectiveness=float(t.bearing_lubrication_system.oil_cooling_effectiveness))
        results.append((sc, ref))
    if explore:
        print("not closed:", json.dumps(failed, indent=1))
        return
    offered = set(catalog)
    assert not [k for k in failed if tuple(k.split(":")) in offered], "catalogued handlers that are not closed: %s" % failed
    for sc, ref in results:
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
        meta["ops"] = [dict(step=o["step"], component=o["comp"], unit=o["unit"], action=o["action"]) for o in sc["ops"]]
        meta["closure_steps"] = CLOSURE_STEPS
        meta["refused"] = failed
        meta["component_ids"] = ref["component_ids"]
        path = os.path.join(OUT, sc["name"] + ".npz")
        np.savez_compressed(path, action=ref["action"], magnitude=ref["magnitude"], setpoint=ref["setpoint"], cooling=ref["cooling"],
                            noise_z=ref["noise_z"], obs=ref["obs"], reward=ref["reward"], done=ref["done"], info=ref["info"],
                            state_steps=np.array(steps), sec_keys=ref["sec_keys"], sec=ref["sec"], rc_keys=ref["rc_keys"], rc=ref["rc"],
                            state=ref["state"][steps], labels=np.array([c[2] for c in cols]), kinds=np.array([c[0] for c in cols]),
                            paths=np.array([c[3] for c in cols]), meta=json.dumps(meta), ops=ref["ops"], op_before=ref["op_before"],
                            op_after=ref["op_after"], op_labels=ref["op_labels"], op_expect_change=ref["op_expect_change"],
                            op_closed=ref["op_closed"])
        print(sc["name"], "steps", T, "ops", len(ref["ops"]), "successful", int(np.nansum(ref["ops"][:, 6])), "closed", int(ref["op_closed"].sum()),
              os.path.getsize(path), "bytes ->", os.path.relpath(path, ROOT))
    if not names:
        missing = [catalog[k] for k in range(len(catalog)) if k not in seen]
        assert not missing, "catalog actions no fixture calls: %s" % missing
        assert set(failed) == {"%s:%s" % k for k in getattr(_lib, "TURBINE_ACTIONS_NOT_OFFERED", {})}, failed


if __name__ == "__main__":
    main(sys.argv[1:])
