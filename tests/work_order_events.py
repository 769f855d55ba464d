"""Work orders created and completed, derived from a golden fixture's per-step maintenance state: the events the device's
maintenance log (npb_set_maintenance_log) must report for that run.

Between state s - 1 and state s (step s - 1; state 0 = the initial state), for each pump k and action a:
  - mpump[k].wo_order[a] goes from n > 0 to anything else: order n completed (maint.executed[a] rises by one per completion);
  - mpump[k].wo_order[a] becomes a new n > 0: order n created, stamped mpump[k].last_trigger_time[a];
the fixtures leave prim.sim_time unrecorded, so the clock of state s is s * dt, which every creation stamp must equal.  The trigger
mask is the rows whose last_violation_time moved; the priority the highest of their table rows (the batched event's)."""
import numpy as np

from nuclear_sim_amd.maintlog import EVENT_DTYPE, CREATED, COMPLETED

PRIORITY = {"LOW": 1, "MEDIUM": 2, "HIGH": 3, "CRITICAL": 4, "EMERGENCY": 5}
NPUMP, NPARAM, NACT = 4, 16, 18
BEARING_REPLACEMENT = 7


def table_priorities(g, params):
    """per catalog parameter: the priority of its row in the run's threshold table (0 = no row)"""
    import json
    import os
    from golden_util import GOLDEN_DIR
    if g.meta.get("maint_thresholds"):
        rows = dict((nm, c) for nm, c in g.meta["maint_thresholds"])
    else:
        rows = {r["name"]: r for r in json.load(open(os.path.join(GOLDEN_DIR, "maint_table.json")))["thresholds"]}
    return np.array([PRIORITY[str(rows[p]["priority"]).upper()] if p in rows else 0 for p in params], dtype=np.int64)


def events_from_golden(g, params, plant=0):
    """the fixture's events as npb_maint_event_t records (maintlog.EVENT_DTYPE), in state order; the states must be recorded at
    consecutive steps (g.state_steps[j + 1] == g.state_steps[j] + 1) between the pairs compared"""
    labels = [c[2] for c in g.cols]
    col = {lab: j for j, lab in enumerate(labels)}
    S = g.state
    steps = [int(s) for s in g.state_steps]
    dt = float(g.meta.get("dt", 1.0))
    prio = table_priorities(g, params)

    def v(j, lab):
        return S[j, col[lab]]
    out = []
    for j in range(1, len(steps)):
        if steps[j] != steps[j - 1] + 1:
            raise ValueError("%s: states %d and %d are not one step apart" % (g.name, steps[j - 1], steps[j]))
        s = steps[j]
        clock = s * dt
        completions = np.zeros(NACT, dtype=np.int64)
        for k in range(NPUMP):
            for a in range(NACT):
                old = v(j - 1, "mpump[%d].wo_order[%d]" % (k, a)); new = v(j, "mpump[%d].wo_order[%d]" % (k, a))
                if old > 0 and new != old:
                    completions[a] += 1
                    out.append((clock, v(j - 1, "mpump[%d].last_trigger_time[%d]" % (k, a)), v(j - 1, "mpump[%d].wo_planned_start[%d]" % (k, a)),
                                plant, int(old), 0, k, a, COMPLETED, 0,
                                int(v(j - 1, "mpump[%d].wo_bearing" % k)) if a == BEARING_REPLACEMENT else 0, 0))
                if new > 0 and new != old:
                    stamp = v(j, "mpump[%d].last_trigger_time[%d]" % (k, a))
                    if stamp != clock:
                        raise AssertionError("%s: order %d created at %r, but the clock of state %d is %r" % (g.name, int(new), stamp, s, clock))
                    trig = 0
                    for q in range(NPARAM):
                        if v(j, "mpump[%d].last_violation_time[%d]" % (k, q)) != v(j - 1, "mpump[%d].last_violation_time[%d]" % (k, q)):
                            trig |= 1 << q
                    p = max([int(prio[q]) for q in range(NPARAM) if (trig >> q) & 1] or [0])
                    out.append((clock, stamp, v(j, "mpump[%d].wo_planned_start[%d]" % (k, a)), plant, int(new), trig, k, a, CREATED, p,
                                int(v(j, "mpump[%d].wo_bearing" % k)) if a == BEARING_REPLACEMENT else 0, 0))
        executed = np.array([v(j, "maint.executed[%d]" % a) - v(j - 1, "maint.executed[%d]" % a) for a in range(NACT)])
        if not np.array_equal(executed, completions):
            raise AssertionError("%s: step %d executed %s, orders closed %s" % (g.name, s - 1, executed, completions))
    return np.array(out, dtype=EVENT_DTYPE)


def per_step(g):
    """the fixture records its state at every step"""
    return len(g.state_steps) == g.T + 1 and all(int(s) == j for j, s in enumerate(g.state_steps))


def windows(g, params, plant=0):
    """sparse-state fixtures: per window between two recorded states, the counts of creations and completions the counters
    say happened ((created_before, created_after, performed_before, performed_after) per window, by time)"""
    labels = [c[2] for c in g.cols]
    col = {lab: j for j, lab in enumerate(labels)}
    steps = [int(s) for s in g.state_steps]
    dt = float(g.meta.get("dt", 1.0))
    out = []
    for j in range(1, len(steps)):
        out.append((steps[j - 1] * dt, steps[j] * dt,
                    int(g.state[j, col["maint.work_orders_created"]] - g.state[j - 1, col["maint.work_orders_created"]]),
                    int(g.state[j, col["maint.maintenance_actions_performed"]] - g.state[j - 1, col["maint.maintenance_actions_performed"]])))
    return out


def make_env(g=None, n=1, **kw):
    """a batch set up as a fixture's run was (the heat source, noise, maintenance parameters and thresholds its meta records)"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    if g is not None:
        m = g.meta
        kw.setdefault("dt", m.get("dt", 1.0))
        kw.setdefault("heat_source", m.get("heat_source", "constant"))
        kw.setdefault("noise_enabled", bool(m.get("noise")))
        kw.setdefault("noise_std_percent", m.get("noise_std_percent", 0.1))
        kw.setdefault("maintenance", bool(m.get("runner") or m.get("state_management")))
        if m.get("maint_params"):
            kw.setdefault("params", dict(m["maint_params"]))
        kw.setdefault("mode", "full" if m.get("enable_secondary", True) else "primary")
        kw.setdefault("reactivity_components", g.rc is not None)
        if m.get("maint_thresholds"):
            kw.setdefault("maintenance_thresholds", dict((nm, c) for nm, c in m["maint_thresholds"]))
    return BatchedPlantEnv(n, **kw)


def host_state(env):
    f, i = env.state_arrays()
    return f.cpu().numpy(), i.cpu().numpy()


def reference_orders(name):
    """tests/golden/wo_<name>.json (tools/make_work_order_golden.py): the reference's FWP work orders after the run, or None"""
    import json
    import os
    from golden_util import GOLDEN_DIR
    path = os.path.join(GOLDEN_DIR, "wo_%s.json" % name)
    if not os.path.exists(path):
        return None
    return json.load(open(path))


def orders_from_columns(cols):
    """maintlog.columns of one plant -> one dict per work order, as the reference's fixture lists them (created / completed
    records joined by work_order_id)"""
    out = {}
    for j in range(len(cols["work_order_id"])):
        wid = cols["work_order_id"][j]
        o = out.setdefault(wid, {"work_order_id": wid, "actual_completion_date": None})
        o["component_id"] = cols["component_id"][j]
        o["title"] = cols["title"][j]
        o["action_types"] = [cols["action_type"][j]]
        if cols["event_type"][j] == "work_order_created":
            o["priority"] = cols["priority"][j]
            o["work_order_type"] = cols["work_order_type"][j]
        else:
            o["actual_completion_date"] = float(cols["actual_completion_date"][j])
        o["created_date"] = float(cols["created_date"][j])
        o["planned_start_date"] = float(cols["planned_start_date"][j])
    return out


def assert_orders_match(cols, ref, where):
    """the log's orders (one plant) against the reference's: id, component, type, priority, title, action, created, planned start,
    completion; the reference's open orders are the log's orders without a completion"""
    mine = orders_from_columns(cols)
    assert ref["meta"]["numbering_matches_device"], ref["meta"]
    theirs = {o["work_order_id"]: o for o in ref["orders"]}
    assert sorted(mine) == sorted(theirs), "%s: orders %s, the reference's %s" % (where, sorted(mine), sorted(theirs))
    for wid, o in theirs.items():
        m = mine[wid]
        for k in ("component_id", "work_order_type", "priority", "title", "action_types", "created_date", "planned_start_date",
                  "actual_completion_date"):
            assert m.get(k) == o[k], "%s %s: %s is %r, the reference's %r" % (where, wid, k, m.get(k), o[k])
