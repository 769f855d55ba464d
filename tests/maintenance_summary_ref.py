"""The per-plant work-order summary computed directly from the reference's recorded work orders (tests/golden/wo_<name>.json,
tools/make_work_order_golden.py): per key the first creation time, the first completion time and the counts -- what
nuclear_sim_amd.maintlog.summarize and the device (npb_set_maintenance_summary) must give for a plant that ran the fixture.  Shared by
tests/test_maintenance_summary_cpu.py and tests/test_maintenance_summary_gpu.py."""
import numpy as np

from work_order_events import reference_orders

WO_FIXTURES = ("m1_oil_top_off_staggered", "m2_oil_top_off_simultaneous", "m8_handlers_inspection_overhaul_promotion",
               "m10_motor_bearing_replacement_seed1", "m13b_oil_analysis", "m13e_bearing_inspection", "z21_fuzzed_maintenance",
               "z22_fuzzed_maintenance")
NACT = 18


def feedwater_keys():
    """every feedwater action with a wildcard unit and with a specific one (oil_top_off with each of the four), any action per unit
    and any action on any unit: 44 keys, as (catalog, action, unit) triples of names and None"""
    from nuclear_sim_amd._lib import MAINT_ACTION_NAMES as A
    assert len(A) == NACT
    keys = [("feedwater", a, None) for a in A]
    keys += [("feedwater", "oil_top_off", u) for u in range(4)]
    keys += [("feedwater", a, j % 4) for j, a in enumerate(A) if a != "oil_top_off"]
    keys += [("feedwater", None, None)] + [("feedwater", None, u) for u in range(4)]
    return keys


def groups(keys, size=16):
    return [keys[j:j + size] for j in range(0, len(keys), size)]


def reference_summary(name, keys, since_minutes=0.0):
    """[n_keys] arrays first_created / first_completed (float64, +inf = never) / n_created / n_completed (int32) of one plant, from the
    reference's WorkOrderManager after the run: an order counts as created if its created_date >= since_minutes, as completed if it has
    an actual_completion_date >= since_minutes"""
    ref = reference_orders(name)
    assert ref is not None and ref["meta"]["orders_on_other_components"] == 0, name
    out = {"first_created": np.full(len(keys), np.inf), "first_completed": np.full(len(keys), np.inf),
           "n_created": np.zeros(len(keys), dtype=np.int32), "n_completed": np.zeros(len(keys), dtype=np.int32)}
    for j, (catalog, action, unit) in enumerate(keys):
        assert catalog == "feedwater"
        for o in ref["orders"]:
            (a,) = o["action_types"]
            u = int(o["component_id"].split("-")[1]) - 1
            if (action is not None and a != action) or (unit is not None and u != unit):
                continue
            if o["created_date"] >= since_minutes:
                out["n_created"][j] += 1
                out["first_created"][j] = min(out["first_created"][j], float(o["created_date"]))
            done = o["actual_completion_date"]
            if done is not None and done >= since_minutes:
                out["n_completed"][j] += 1
                out["first_completed"][j] = min(out["first_completed"][j], float(done))
    return out


def records_from_orders(name, plant=0):
    """the reference's orders as event records (maintlog.EVENT_DTYPE): a creation at created_date and, for a completed order, a
    completion at actual_completion_date -- for the fixtures whose state is not recorded at every step, where
    work_order_events.events_from_golden cannot tell when between two recorded states an order came or went"""
    from nuclear_sim_amd._lib import MAINT_ACTION_NAMES as A
    from nuclear_sim_amd.maintlog import COMPLETED, CREATED, EVENT_DTYPE
    out = []
    for o in reference_orders(name)["orders"]:
        (a,) = o["action_types"]
        u, n = int(o["component_id"].split("-")[1]) - 1, int(o["work_order_id"].split("-")[1])
        out.append((o["created_date"], o["created_date"], o["planned_start_date"], plant, n, 0, u, A.index(a), CREATED, 0, 0, 0))
        if o["actual_completion_date"] is not None:
            out.append((o["actual_completion_date"], o["created_date"], o["planned_start_date"], plant, n, 0, u, A.index(a), COMPLETED, 0, 0, 0))
    return np.array(out, dtype=EVENT_DTYPE)


def assert_same_tables(got, want, where, plants=None):
    """exact: integers equal, times bit-equal; ``want`` may be one plant's [n_keys] arrays, compared against the columns ``plants``"""
    for k in ("first_created", "first_completed", "n_created", "n_completed"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if plants is not None:
            g = g[:, plants]
            if w.ndim == 1:
                w = np.repeat(w[:, None], g.shape[1], axis=1)
        assert g.dtype == w.dtype and g.shape == w.shape, (where, k, g.dtype, w.dtype, g.shape, w.shape)
        gb, wb = (g.view(np.uint64), w.view(np.uint64)) if g.dtype == np.float64 else (g, w)
        bad = np.argwhere(gb != wb)
        assert len(bad) == 0, "%s: %s differs at (key, plant) %s: got %r, want %r" % (where, k, bad[:6].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
