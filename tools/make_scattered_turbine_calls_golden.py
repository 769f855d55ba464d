"""Reference fixtures of scattered operator calls on the turbine: tests/golden/operator_calls/turbine/sc_turbine_*.npz.

The method of tools/make_scattered_calls_golden.py (whose Section / run_calls / pack this generator uses), for the catalog of
npb_perform_turbine_maintenance: ONE live reference simulator, stepped a few times, and for each call of a long list every real member
of turb and tstg is poked with a seeded draw, then the members the call is ABOUT are poked to the values its `set` names; the members
are read back (before), perform_maintenance(type) is called on the turbine, a bearing, the lubrication system or a stage (success,
after), and the same again from the float32-rounded values (after32).  Nothing is stepped between calls.

Written-out cases beside the drawn ones: every min / max of the handlers with its member exactly on the cap, just below and just above;
the protection test with and without an active trip; the thrust adjustment on every bearing; a NaN in a member a handler reads; the
vibration monitor's displacement on both sides of the knee of vibration_analysis' min(5.0, 0.3 v) (the reduction moves bearing attributes
the state does not carry, and reads the previous step's result, not a carried member: the carried thermal bow follows the factor 0.7 wherever
the vibration stands); stages and bearings that need nothing.

The files live in a sub-directory of their own: tests/test_scattered_calls_fixtures.py holds tests/golden/operator_calls/*.npz to the
component and pump files.

  calls[K, 8]: (turbine kind called, unit, catalog index (_lib.TURBINE_ACTIONS), 0, success, explicit, 0, 0)

    python tools/make_scattered_turbine_calls_golden.py            writes the files
    python tools/make_scattered_turbine_calls_golden.py --check    regenerates and compares with the committed files bit for bit
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_scattered_calls_golden as base      # noqa: E402
from make_turbine_maintenance_golden import KINDS, THRUST, UNITS, install_mask_poke, target_of      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "operator_calls", "turbine")
N_RANDOM = 150
PER_FILE = 120
NAN = float("nan")
TURBINE_SECTIONS = ("turb.", "tstg.")
# (label suffix, lo, hi): the ranges of _scrambled in tests/test_turbine_maintenance_gpu.py, and the protection timers
TURBINE_RANGES = (("turb.bearing_wear_factor", 0.7, 1.0), ("turb.bearing_metal_temp", 75.0, 110.0), ("turb.lub_oil_temperature", 40.0, 70.0),
                  ("turb.lub_oil_contamination", 0.5, 15.0), ("turb.lub_oil_moisture", 0.01, 0.08), ("turb.lub_oil_acidity", 0.02, 0.6),
                  ("turb.lub_effectiveness", 0.4, 1.0), ("turb.thermal_bow", 0.0, 0.05), ("turb.lub_wear", 0.0, 25.0),
                  ("tstg.stage_deposit_thickness", 0.0, 0.4), ("tstg.stage_blade_wear_factor", 0.8, 1.0),
                  ("tstg.stage_efficiency_degradation", 0.0, 0.05), ("turb.timer_overspeed", 0.0, 600.0), ("turb.timer_vibration", 0.0, 600.0),
                  ("turb.timer_bearing_temp", 0.0, 600.0))
READ_ONLY = (("turbine", "turbine_performance_test"), ("turbine", "thermal_stress_analysis"), ("bearing", "turbine_bearing_inspection"),
             ("bearing", "bearing_clearance_check"), ("bearing", "bearing_alignment"))


def tc(comp, unit, action, expect, **set_):
    return dict(comp=comp, unit=unit, action=action, expect=expect, set=set_, explicit=1)


def explicit_calls():
    tb, br, lu, st = KINDS
    T = lambda b: "turb.bearing_metal_temp[%d]" % b
    W = lambda b: "turb.bearing_wear_factor[%d]" % b
    C = []
    # the turbine's routine maintenance: max(80, T - 0.5) with a bearing exactly on the floor's edge, below, above; all four at or below 80
    C.append(tc(tb, 0, "routine_maintenance", True, **{T(0): 80.5, T(1): 80.0, T(2): 79.0, T(3): 120.0}))
    C.append(tc(tb, 0, "routine_maintenance", True, **{T(0): 80.4, T(1): 80.6, T(2): 80.5, T(3): 80.0}))
    C.append(tc(tb, 0, "routine_maintenance", False, **{T(0): 80.0, T(1): 80.0, T(2): 80.0, T(3): 80.0}))
    C.append(tc(tb, 0, "routine_maintenance", True, **{T(1): NAN}))          # max(80.0, nan) is 80.0
    # system optimisation: min(1, e + 0.05) on the cap, below, above
    for e in (0.95, 0.9, 0.99, 1.0):
        C.append(tc(tb, 0, "turbine_system_optimization", e != 1.0, **{"turb.lub_effectiveness": e}))
    # the protection test with and without an active trip
    C.append(tc(tb, 0, "turbine_protection_test", True, **{"turb.trip_active": 1, "turb.trip_latched_mask": 6}))
    C.append(tc(tb, 0, "turbine_protection_test", False, **{"turb.trip_active": 0, "turb.trip_latched_mask": 6}))
    C.append(tc(tb, 0, "turbine_protection_test", True, **{"turb.trip_active": 1, "turb.trip_latched_mask": 0}))
    C.append(tc(tb, 0, "turbine_protection_test", True, **{"turb.trip_active": 1, "turb.trip_latched_mask": 63, "turb.timer_overspeed": 0.0,
                                                            "turb.timer_vibration": 0.0, "turb.timer_bearing_temp": 0.0}))
    # the vibration analysis on both sides of the knee of min(5.0, 0.3 v) (v = 50 / 3), and with a rotor that is not bowed
    for v in (10.0, 16.0, 17.0, 30.0):
        C.append(tc(tb, 0, "vibration_analysis", True, **{"turb.vibration_displacement": v, "turb.thermal_bow": 0.03}))
    C.append(tc(tb, 0, "vibration_analysis", False, **{"turb.thermal_bow": 0.0}))
    C.append(tc(tb, 0, "vibration_analysis", False, **{"turb.thermal_bow": NAN}))
    # a bearing's replacement: min(T, 90) on the cap, below, above; one that needs nothing; a NaN temperature stays NaN
    for b, t in enumerate((90.0, 89.9, 90.1, 75.0)):
        C.append(tc(br, b, "turbine_bearing_replacement", True, **{T(b): t, W(b): 0.8}))
    C.append(tc(br, 1, "turbine_bearing_replacement", False, **{T(1): 85.0, W(1): 1.0}))
    C.append(tc(br, 3, "turbine_bearing_replacement", True, **{T(3): NAN, W(3): 0.9}))
    # the thrust adjustment: the thrust bearing with max(80, T - 5) on the edge, below, above; every journal bearing is refused
    for t in (85.0, 84.0, 86.0, 80.0, 70.0, NAN):
        C.append(tc(br, THRUST, "thrust_bearing_adjustment", t != 80.0, **{T(THRUST): t}))
    for b in (0, 1, 3):
        C.append(tc(br, b, "thrust_bearing_adjustment", False, **{T(b): 100.0}))
    # a bearing's oil change (max(80, T - 2)) and routine maintenance (max(80, T - 1))
    for b, t in enumerate((82.0, 81.9, 82.1, 80.0)):
        C.append(tc(br, b, "turbine_oil_change", t != 80.0, **{T(b): t}))
    for b, t in enumerate((81.0, 80.9, 81.1, 80.0)):
        C.append(tc(br, b, "routine_maintenance", t != 80.0, **{T(b): t}))
    for b in range(4):
        for a in ("turbine_bearing_inspection", "bearing_clearance_check", "bearing_alignment"):
            C.append(tc(br, b, a, False))
    # the oil change of the lubrication system: min(1, e + 0.15) and max(45, T - 5) on the edges; NaN members
    for e, t in ((0.85, 50.0), (0.84, 49.9), (0.86, 50.1), (1.0, 45.0), (0.5, 40.0)):
        C.append(tc(lu, 0, "turbine_oil_change", True, **{"turb.lub_effectiveness": e, "turb.lub_oil_temperature": t}))
    C.append(tc(lu, 0, "turbine_oil_change", True, **{"turb.lub_effectiveness": NAN, "turb.lub_oil_temperature": NAN}))
    C.append(tc(lu, 0, "turbine_oil_change", False, **{"turb.lub_effectiveness": 1.0, "turb.lub_oil_temperature": 45.0, "turb.lub_oil_contamination": 1.0,
                                                        "turb.lub_oil_acidity": 0.05, "turb.lub_oil_moisture": 0.01}))
    # the top-off at an oil level of 100: max(1, c) and max(0.05, a) from both sides, and on the floors
    for c, a, e in ((8.0, 0.3, False), (1.0, 0.05, False), (0.9, 0.3, True), (8.0, 0.04, True), (0.5, 0.01, True), (NAN, 0.3, True)):
        C.append(tc(lu, 0, "turbine_oil_top_off", e, **{"turb.lub_oil_contamination": c, "turb.lub_oil_acidity": a}))
    # the filter replacement: min(5, 0.6 c) around c = 25 / 3, the floor max(1, c) around c = 2.5; min(1, e + 0.05)
    for c, e in ((8.0, 0.95), (9.0, 0.94), (25.0 / 3.0, 0.96), (2.5, 0.5), (2.4, 0.5), (2.6, 0.5), (1.0, 1.0), (0.5, 0.7), (NAN, 0.7), (20.0, NAN)):
        C.append(tc(lu, 0, "oil_filter_replacement", True if c != 1.0 else False, **{"turb.lub_oil_contamination": c, "turb.lub_effectiveness": e}))
    # the oil-cooler cleaning: max(0, w - 5) of the fifth component and max(45, T - 0)
    for w, t, e in ((5.0, 50.0, True), (4.9, 50.0, True), (5.1, 45.0, True), (0.0, 50.0, False), (0.0, 44.0, True), (0.0, 45.0, False), (NAN, 50.0, True)):
        C.append(tc(lu, 0, "oil_cooler_cleaning", e, **{"turb.lub_wear[4]": w, "turb.lub_oil_temperature": t}))
    # the system test: min(1, e + 0.1)
    for e in (0.9, 0.89, 0.91, 1.0):
        C.append(tc(lu, 0, "lubrication_system_test", e != 1.0, **{"turb.lub_effectiveness": e}))
    # routine maintenance: every floor on its edge, and a system that needs nothing
    C.append(tc(lu, 0, "routine_maintenance", True, **{"turb.lub_effectiveness": 0.98, "turb.lub_oil_contamination": 1.5, "turb.lub_oil_temperature": 46.0,
                                                        "turb.lub_wear[0]": 0.5, "turb.lub_wear[1]": 0.4, "turb.lub_wear[2]": 0.6, "turb.lub_wear[3]": 0.0}))
    C.append(tc(lu, 0, "routine_maintenance", True, **{"turb.lub_effectiveness": 0.97, "turb.lub_oil_contamination": 1.4, "turb.lub_oil_temperature": 45.9}))
    C.append(tc(lu, 0, "routine_maintenance", True, **{"turb.lub_effectiveness": 0.99, "turb.lub_oil_contamination": 1.6, "turb.lub_oil_temperature": 46.1}))
    C.append(tc(lu, 0, "routine_maintenance", False, **dict({"turb.lub_effectiveness": 1.0, "turb.lub_oil_contamination": 1.0, "turb.lub_oil_temperature": 45.0},
                                                             **{"turb.lub_wear[%d]" % k: 0.0 for k in range(5)})))
    C.append(tc(lu, 0, "routine_maintenance", True, **{"turb.lub_wear[2]": NAN, "turb.lub_oil_contamination": NAN}))
    # the stages: both types on every stage; a stage that needs nothing; NaN members
    for k in range(14):
        C.append(tc(st, k, "blade_replacement", True))
        C.append(tc(st, (k + 5) % 14, "overhaul", True))
    S = lambda k, m: "tstg.stage_%s[%d]" % (m, k)
    C.append(tc(st, 4, "blade_replacement", False, **{S(4, "blade_wear_factor"): 1.0}))
    C.append(tc(st, 9, "overhaul", False, **{S(9, "blade_wear_factor"): 1.0, S(9, "deposit_thickness"): 0.0, S(9, "efficiency_degradation"): 0.0}))
    C.append(tc(st, 2, "overhaul", True, **{S(2, "blade_wear_factor"): NAN, S(2, "deposit_thickness"): NAN, S(2, "efficiency_degradation"): NAN}))
    C.append(tc(st, 11, "blade_replacement", True, **{S(11, "blade_wear_factor"): NAN, S(11, "deposit_thickness"): NAN}))
    return C


def random_calls(catalog):
    rng = np.random.default_rng([base.SEED, 31])
    C = []
    for _ in range(N_RANDOM):
        kind, action = catalog[int(rng.integers(0, len(catalog)))]
        C.append(dict(comp=kind, unit=int(rng.integers(0, UNITS[kind])), action=action, expect=None, set={}, explicit=0))
    return C


def generate():
    from nuclear_sim_amd.schema import SCHEMA
    from nuclear_sim_amd._lib import TURBINE_ACTIONS
    from oracle.ref_harness import refsim
    refsim.setup()
    install_mask_poke()
    from systems.primary import ControlAction
    sim = refsim.make_sim(dt=5.0)
    with refsim.quiet():
        for _ in range(base.STEPS_BEFORE):
            sim.step(ControlAction(8), magnitude=1.0)
    catalog = list(TURBINE_ACTIONS)
    S = base.Section(sim, SCHEMA.columns(), lambda lab: lab.startswith(TURBINE_SECTIONS), TURBINE_RANGES)

    def call(c, before, j):
        res = target_of(sim, c).perform_maintenance(c["action"])
        return res if c["comp"] != "stage" else {"success": bool(res)}      # a stage's handler returns no success flag
    calls = explicit_calls() + random_calls(catalog)
    kept, dropped = base.run_calls(lambda c: S, calls, call, 30)
    assert not dropped, dropped
    rows, expect = [], []
    for c, before, after, _b32, _a32, ok, _j in kept:
        changed = bool((~base.same(before, after)).any())
        if c["expect"] is not None:
            assert changed == bool(c["expect"]), (c, [S.labels[q] for q in np.nonzero(~base.same(before, after))[0]])
        if (c["comp"], c["action"]) in READ_ONLY:
            assert not changed, c
        assert ok == (not (c["action"] == "thrust_bearing_adjustment" and c["unit"] != THRUST)), c
        assert ok or not changed, c
        rows.append((KINDS.index(c["comp"]), c["unit"], catalog.index((c["comp"], c["action"])), 0, float(ok), c["explicit"], 0, 0))
        expect.append(int(changed))
    common = dict(seed=base.SEED, steps_before=base.STEPS_BEFORE, dt=5.0, else_within=base.ELSE_WITHIN,
                  note="draws: uniform in the range of a member's name, other real members base * (1 +- else_within), integer members kept")
    files = {}
    for part, lo in enumerate(range(0, len(kept), PER_FILE)):
        sl = slice(lo, lo + PER_FILE)
        meta = dict(common, kind="turbine", part=part, ranges=[list(r) for r in TURBINE_RANGES], not_poked=S.not_poked, dropped=dropped,
                    calls=[base.jsonable(k[0]) for k in kept[sl]])
        files["sc_turbine_%02d" % part] = base.pack(S, kept[sl], rows[sl], expect[sl], meta)
    return files


def main(argv):
    files = generate()
    if "--check" in argv:
        names = sorted(os.path.splitext(f)[0] for f in os.listdir(OUT) if f.endswith(".npz"))
        assert names == sorted(files), (names, sorted(files))
        for name, new in files.items():
            old = np.load(os.path.join(OUT, name + ".npz"), allow_pickle=False)
            assert sorted(old.files) == sorted(new), (name, old.files)
            for k, v in new.items():
                a, b = old[k], np.asarray(v)
                if a.dtype.kind == "f":
                    assert a.shape == b.shape and base.same(a, b).all(), "%s: %s differs from the committed file" % (name, k)
                else:
                    assert a.shape == b.shape and np.array_equal(a, b), "%s: %s differs from the committed file" % (name, k)
            print(name, "reproduced bit for bit:", len(new["calls"]), "calls")
        return
    os.makedirs(OUT, exist_ok=True)
    for name, arrays in files.items():
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        meta = json.loads(arrays["meta"])
        print(name, "calls", len(arrays["calls"]), "successful", int(arrays["calls"][:, 4].sum()), "changing", int(arrays["expect_change"].sum()),
              "not poked", meta["not_poked"], os.path.getsize(path), "bytes ->", os.path.relpath(path, ROOT))


if __name__ == "__main__":
    main(sys.argv[1:])
