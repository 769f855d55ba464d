"""Reference work-order fixtures: tests/golden/wo_<scenario>.json.

Re-runs a handful of the committed maintenance scenarios on the REFERENCE (oracle/ref_harness: make_golden.scenarios,
trace.run_reference; needs a machine with the reference) and writes what its WorkOrderManager holds after the run: the open and the
completed orders on FWP-* components, with the fields the data-gen runner exports.  Orders on other components are counted, not
listed: they take numbers from the same counter, so where there are any the reference's WO-%06d numbering and the device's (one
counter per plant, FWP orders only) diverge, and the fixture's meta says so.  Before writing, every re-run is checked against the
scenario's committed .npz (observations and the maintenance counters at every recorded state).

    python tools/make_work_order_golden.py [scenario ...]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCENARIOS = ("m1_oil_top_off_staggered", "m2_oil_top_off_simultaneous", "m8_handlers_inspection_overhaul_promotion",
             "m10_motor_bearing_replacement_seed1", "m13b_oil_analysis", "m13e_bearing_inspection", "z21_fuzzed_maintenance",
             "z22_fuzzed_maintenance")


def _order(wo):
    md = getattr(wo, "metadata", None) or {}
    return {"work_order_id": wo.work_order_id, "component_id": wo.component_id, "work_order_type": wo.work_order_type.value,
            "priority": wo.priority.name, "status": wo.status.value, "title": wo.title, "created_date": wo.created_date,
            "planned_start_date": wo.planned_start_date, "actual_start_date": wo.actual_start_date,
            "actual_completion_date": wo.actual_completion_date,
            "action_types": [a.action_type for a in wo.maintenance_actions],
            "extracted_component_id": md.get("extracted_component_id")}


def _check_against_npz(name, ref):
    from golden_util import Golden
    g = Golden(name)
    steps = [int(s) for s in g.state_steps]
    np.testing.assert_array_equal(ref["obs"], g.obs, err_msg="%s: the re-run's observations are not the committed fixture's" % name)
    labels = [c[2] for c in g.cols]
    from nuclear_sim_amd.schema import SCHEMA
    cols = SCHEMA.columns()
    for lab in ("maint.work_orders_created", "maint.maintenance_actions_performed"):
        j = [c[2] for c in cols].index(lab)
        np.testing.assert_array_equal(ref["state"][steps, j], g.state[:, labels.index(lab)], err_msg="%s: %s" % (name, lab))


def main(names):
    from oracle.ref_harness import make_golden, trace
    from nuclear_sim_amd.schema import SCHEMA
    cols = SCHEMA.columns()
    by_name = {sc["name"]: sc for sc in make_golden.scenarios()}
    for name in names:
        sc = by_name[name]
        ref, sim = trace.run_reference(sc, cols)
        _check_against_npz(name, ref)
        wom = sim.maintenance_system.work_order_manager
        orders = list(wom.work_orders.values()) + list(wom.completed_work_orders)
        fwp = sorted((o for o in orders if str(o.component_id).startswith("FWP-")), key=lambda o: (o.created_date, o.work_order_id))
        other = [o for o in orders if not str(o.component_id).startswith("FWP-")]
        out = {"meta": {"scenario": name, "steps": sc["steps"], "dt": sc.get("dt", 1.0),
                        "orders_on_other_components": len(other),
                        "numbering_matches_device": len(other) == 0,
                        "note": "the reference's WorkOrderManager after the run: open (work_orders) and completed (completed_work_orders) "
                                "orders on FWP-* components; orders on other components take numbers from the same counter and are "
                                "only counted, so with any of them the WO numbers differ from the device's per-plant FWP numbering"},
               "orders": [_order(o) for o in fwp]}
        path = os.path.join(ROOT, "tests", "golden", "wo_%s.json" % name)
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
        print(name, len(fwp), "FWP orders,", len(other), "on other components ->", os.path.relpath(path, ROOT))


if __name__ == "__main__":
    main(sys.argv[1:] or SCENARIOS)
