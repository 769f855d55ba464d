"""What NuclearPlantSimulator.reset() leaves in the thirteen quantities the diagnostics build carries from step to step
(include/npb.h NPB_DIAG_CARRIED): tests/golden/diag_carry/reference_reset.json.

Drives a REFERENCE simulator (oracle/ref_harness/refsim; needs a machine with the reference): a run that moves the quantities -- those
the quiet run leaves at rest are poked to a value no reset would produce -- then ``sim.reset()``, each quantity read by attribute before
and after.  Per row the file records "kept" (the reset left the moved value) or the value it was reset to, with the attribute read and
both readings.  A quantity with no attribute to read would be recorded with "rule": "legacy" and the reason.  npb_reset_reference
(nuclear_sim_amd/csrc/npb_api.hip, diag_reference_reset_values) restates the file; tests/test_diagnostics_carry_gpu.py holds it to it.

    python tools/make_diag_reset_golden.py [steps]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "diag_carry", "reference_reset.json")


def find(root, want, name="sim.secondary_physics", limit=200000):
    """[(path, object)] of the objects under `root` that `want(obj)` accepts, in discovery order (breadth first over attributes, dict
    values and list items of the reference's own classes)"""
    seen, out, queue = set(), [], [(name, root)]
    while queue and limit > 0:
        path, obj = queue.pop(0)
        limit -= 1
        if id(obj) in seen:
            continue
        seen.add(id(obj))
        try:
            if want(obj):
                out.append((path, obj))
        except Exception:
            pass
        if isinstance(obj, dict):
            queue.extend(("%s[%r]" % (path, k), v) for k, v in obj.items() if hasattr(v, "__dict__") or isinstance(v, (dict, list)))
        elif isinstance(obj, (list, tuple)):
            queue.extend(("%s[%d]" % (path, k), v) for k, v in enumerate(obj) if hasattr(v, "__dict__") or isinstance(v, (dict, list)))
        elif hasattr(obj, "__dict__") and type(obj).__module__.split(".")[0] in ("systems", "simulator"):
            queue.extend(("%s.%s" % (path, k), v) for k, v in vars(obj).items() if hasattr(v, "__dict__") or isinstance(v, (dict, list)))
    return out


def quantities(sim):
    """[(row, name, getter, setter, path)] in the table order of include/npb.h NPB_DIAG_CARRIED"""
    sec = sim.secondary_physics
    bearing_ids = ["TB-001", "TB-002", "TB-003", "TB-004"]
    bearings = {getattr(o.config, "bearing_id", None): (p, o) for p, o in
                find(sec, lambda o: hasattr(o, "clearance_increase") and hasattr(getattr(o, "config", None), "bearing_id"))}
    (rotor_path, rotor), = find(sec, lambda o: hasattr(o, "overspeed_events"))[:1]
    (stages_path, stages), = find(sec, lambda o: hasattr(o, "system_efficiency") and hasattr(o, "overall_efficiency"))[:1]
    (prot_path, prot), = find(sec, lambda o: hasattr(o, "valid_trip_count") and hasattr(o, "emergency_actions"))[:1]
    ejectors = {getattr(o.config, "ejector_id", None): (p, o) for p, o in
                find(sec, lambda o: hasattr(o, "compression_ratio_actual") and hasattr(getattr(o, "config", None), "ejector_id"))}
    out = []

    def attr(row, name, path, obj, a):
        out.append((row, name, lambda: float(getattr(obj, a)), lambda v: setattr(obj, a, type(getattr(obj, a))(v)), "%s.%s" % (path, a)))

    def item(row, name, path, obj, a, k):      # read through the owner at every reading: a reset may replace the dict
        out.append((row, name, lambda: float(getattr(obj, a)[k]), lambda v: getattr(obj, a).__setitem__(k, bool(v)), "%s.%s[%r]" % (path, a, k)))
    for q, b in enumerate(bearing_ids):
        attr(124 + q, "%s_clearance_increase" % b, bearings[b][0], bearings[b][1], "clearance_increase")
    attr(128, "overspeed_events", rotor_path, rotor, "overspeed_events")
    attr(133, "stage_system.system_efficiency", stages_path, stages, "system_efficiency")
    attr(141, "protection_valid_trip_count", prot_path, prot, "valid_trip_count")
    item(142, "protection_emergency_feedwater", prot_path, prot, "emergency_actions", "emergency_feedwater_activated")
    item(143, "protection_steam_dump", prot_path, prot, "emergency_actions", "steam_dump_activated")
    for e, sje in enumerate(("SJE-001", "SJE-002")):
        attr(164 + e, "%s_compression_ratio" % sje, ejectors[sje][0], ejectors[sje][1], "compression_ratio_actual")
    for e, sje in enumerate(("SJE-001", "SJE-002")):
        attr(166 + e, "%s_operating_hours" % sje, ejectors[sje][0], ejectors[sje][1], "operating_hours")
    return out


# values a reset could not produce by itself, for the quantities the quiet run leaves at their construction value
POKES = {133: 0.875, 141: 3.0, 142: 1.0, 143: 1.0, 165: 9.25, 167: 2.5}


def main(argv):
    from oracle.ref_harness import refsim
    steps = int(argv[1]) if len(argv) > 1 else 24
    sim = refsim.make_sim(dt=1.0)
    Q = quantities(sim)
    fresh = [get() for _row, _name, get, _set, _path in Q]
    with refsim.quiet():
        for _ in range(steps):
            sim.step()
    moved = {}
    for (row, _name, get, put, _path), f in zip(Q, fresh):
        if get() == f and row in POKES:
            put(POKES[row]); moved[row] = "poke"
        else:
            moved[row] = "run" if get() != f else "not moved"
    before = [get() for _row, _name, get, _set, _path in Q]
    with refsim.quiet():
        sim.reset()
    after = [get() for _row, _name, get, _set, _path in quantities(sim)]      # found again: a reset may replace an object
    rows = []
    for (row, name, _get, _put, path), f, b, a in zip(Q, fresh, before, after):
        assert b != f, (row, name, "the quantity was not moved: the reset's effect on it cannot be seen")
        rows.append({"row": row, "quantity": name, "attribute": path, "fresh": f, "moved_by": moved[row], "before_reset": b, "after_reset": a,
                     "rule": "kept" if a == b else "reset", "reset_to": None if a == b else a})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump({"what": "NuclearPlantSimulator.reset() on the carried diagnostics quantities, read off the live reference by attribute "
                           "(tools/make_diag_reset_golden.py)", "steps_before_reset": steps, "rows": rows}, fh, indent=1)
        fh.write("\n")
    for r in rows:
        print(r["row"], r["quantity"], r["moved_by"], r["before_reset"], "->", r["after_reset"], r["rule"])


if __name__ == "__main__":
    main(sys.argv)
