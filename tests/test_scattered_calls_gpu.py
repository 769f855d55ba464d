"""GPU: the two operator-maintenance kernels (npb_operator_component_maint_kernel, npb_operator_maint_kernel) with one reference call per
LANE.  Every call of the replay fixtures (tests/golden/operator_components/, tests/golden/operator/) and of the scattered-call fixtures
(tests/golden/operator_calls/: a seeded draw of every member the handlers read, the branch inputs pinned from both sides) gets a lane of
its own in ONE launch, beside lanes that order nothing that exists; neighbours differ in kind, unit, option, pump, bearing and target.
Every lane is checked in every schema column: what the call may touch against the reference's values after the call, everything else
against its own bits before the launch.

Tolerances.  fp64 storage: integers exact; carried real members 1e-12 relative (the bound test_operator_top_off_is_the_automatic_top_off
holds two compilations of the same expressions to; measured here against the reference: see WORST_MEASURED), the cancellation columns
at the contract's RTOL with golden_util's floor; output members, which the arena stores as float, at the contract's RTOL.  fp32
storage: the reference's own result from the float32-rounded inputs, so what is left is the rounding of the store -- one float32 ulp."""
import numpy as np
import pytest

from golden_util import ATOL_SMALL, CANCELLATION_COLUMNS, CANCELLATION_FLOOR, RTOL
from component_maintenance_golden import ACTIONS, UNITS, ComponentGolden
from operator_maintenance_golden import ACTIONS as PUMP_ACTIONS, OperatorGolden
from scattered_calls_golden import ScatteredCalls
from work_order_events import host_state
from nuclear_sim_amd.schema import SCHEMA

pytestmark = pytest.mark.gpu

OPERATOR_COMPONENT = 3
# carried real members outside the cancellation columns under fp64 storage, over every lane of the launches below, against the reference
# (MI355X): component kernel 4.4e-16, pump kernel 3.7e-16 (output members 6.1e-8: float in the arena; cancellation columns 2.6e-15)
WORST_MEASURED = 4.4e-16
CARRIED_RTOL = 1e-12
_CACHE = {}


def _cached(key, make):
    """loaded once, shared, never written to"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _columns():
    def make():
        cols = SCHEMA.columns()
        by_label = {lab: (kind, slot) for kind, slot, lab, _p in cols}
        floor = np.full(SCHEMA.total_f64, ATOL_SMALL); cancel = np.zeros(SCHEMA.total_f64, dtype=bool); narrow = np.zeros(SCHEMA.total_f64, dtype=bool)
        names = [None] * SCHEMA.total_f64
        for kind, slot, lab, _p in cols:
            if kind != "f64":
                continue
            names[slot] = lab
            sec, _, rest = lab.partition(".")
            narrow[slot] = SCHEMA.is_output(sec.split("[")[0] + "." + rest.split("[")[0])
            if lab.endswith(CANCELLATION_COLUMNS):
                floor[slot] = CANCELLATION_FLOOR; cancel[slot] = True
        return by_label, floor, cancel, narrow, names
    return _cached("columns", make)


class Lane:
    """one plant of the launch: the order's columns, the reference's success, and its members (kind, slot) before / after the call
    (valid = the reference has the member: a NaN in a replay fixture is "no such leaf", in a scattered call a value)"""

    def __init__(self, order, success, slots, before, after, valid, default, what):
        self.order, self.success, self.slots, self.before, self.after, self.valid = order, bool(success), slots, before, after, valid
        self.default, self.what = default, what


def _load(env, lanes, extra=None):
    """every lane's `before` into a copy of the batch's state; returns what the device then holds"""
    f0, i0 = host_state(env)
    for p, lane in enumerate(lanes):
        for (kind, slot), v, ok in zip(lane.slots, lane.before, lane.valid):
            if ok:
                if kind == "f64":
                    f0[slot, p] = v
                else:
                    i0[slot, p] = int(v)
    if extra is not None:
        extra(f0, i0)
    env.load_state_arrays(f0, i0)
    return host_state(env)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def _check(env, lanes, ordered, pre, f32, where):
    """every column of every lane after the launch; ordered[p] = lane p's order was in the launch.  Returns the worst relative deviation
    per class of real column."""
    by_label, floor, cancel, narrow, names = _columns()
    n = len(lanes)
    post_f, post_i = host_state(env)
    pre_f, pre_i = pre
    want_f = np.zeros((SCHEMA.total_f64, n)); chk_f = np.zeros((SCHEMA.total_f64, n), dtype=bool)
    want_i = np.zeros((SCHEMA.total_i32, n), dtype=np.int64); chk_i = np.zeros((SCHEMA.total_i32, n), dtype=bool)
    for p, lane in enumerate(lanes):
        if not ordered[p]:
            continue
        for (kind, slot), v, ok in zip(lane.slots, lane.after, lane.valid):
            if ok and kind == "f64":
                want_f[slot, p] = v; chk_f[slot, p] = True
            elif ok:
                want_i[slot, p] = int(v); chk_i[slot, p] = True
    # outside the fixture's members, and on every lane that ordered nothing: the bits before the launch
    keep_f = ~chk_f & (_bits(post_f) != _bits(pre_f)); keep_i = ~chk_i & (post_i != pre_i)
    assert not keep_f.any() and not keep_i.any(), "%s: columns no call may touch moved, first (column, lane): %s" % (
        where, [(names[s], p, lanes[p].what) for s, p in zip(*np.nonzero(keep_f))][:5] + [("i32 slot %d" % s, p, lanes[p].what) for s, p in zip(*np.nonzero(keep_i))][:5])
    bad_i = chk_i & (post_i != want_i)
    assert not bad_i.any(), "%s: integer members, first (slot, lane, got, want): %s" % (
        where, [(s, p, lanes[p].what, int(post_i[s, p]), int(want_i[s, p])) for s, p in zip(*np.nonzero(bad_i))][:5])
    nan_w = chk_f & np.isnan(want_f); nan_g = chk_f & np.isnan(post_f)
    assert np.array_equal(nan_w, nan_g), "%s: NaN positions differ, first: %s" % (
        where, [(names[s], p, lanes[p].what, post_f[s, p], want_f[s, p]) for s, p in zip(*np.nonzero(nan_w != nan_g))][:5])
    fin = chk_f & ~nan_w
    err = np.where(fin, np.abs(post_f - np.where(fin, want_f, 0.0)), 0.0)
    if f32:
        tol = 2.0 ** -23 * np.abs(want_f) + 2.0 ** -149
    else:
        rtol = np.where((cancel | narrow), RTOL, CARRIED_RTOL)[:, None]
        tol = rtol * np.abs(want_f) + floor[:, None]
    bad = fin & ~(err <= tol)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(fin & (err > 0), err / np.abs(want_f), 0.0)
    worst = {"carried": float(rel[~(cancel | narrow)].max()), "output members (float in the arena)": float(rel[narrow & ~cancel].max()),
             "cancellation columns": float(rel[cancel].max())}
    print("%s: %d lanes, %d ordered, %d real and %d integer members held to the reference; worst relative deviation %s" % (
        where, n, int(np.sum(ordered)), int(fin.sum()), int(chk_i.sum()), ", ".join("%s %.3e" % kv for kv in worst.items())))
    assert not bad.any(), "%s: %d members off, first (column, lane, got, want): %s" % (
        where, int(bad.sum()), [(names[s], p, lanes[p].what, post_f[s, p], want_f[s, p]) for s, p in zip(*np.nonzero(bad))][:5])
    return worst


def _permuted(lanes, seed):
    order = np.random.default_rng(seed).permutation(len(lanes))
    return [lanes[q] for q in order]


# ---------------------------------------------------------------------------------------------------------------- the component kernel
NOOP_ORDERS = (dict(action=-1, unit=0), dict(action=len(ACTIONS), unit=0), dict(action=1000, unit=1),
               dict(action=ACTIONS.index(("steam_generator", "tsp_chemical_cleaning")), unit=3),
               dict(action=ACTIONS.index(("steam_generator", "scale_removal")), unit=-1),
               dict(action=ACTIONS.index(("ejector", "general")), unit=2))


def _component_lanes(replays=True):
    """the lanes of the component launch, in a fixed permutation; system and condenser lanes carry junk units, lanes that name a cleaning
    method no handler knows carry one of four spellings of it"""
    def make():
        by_label = _columns()[0]
        sc = ScatteredCalls("components")
        sc_slots = sc.slots()
        lanes = []
        junk_units, other_methods = (7, -2), (5, 6, 1000, -1)
        if replays:
            for name in ("oc1_steam_generators", "oc2_condenser", "oc3_long_run"):
                g = ComponentGolden(name)
                slots = [by_label[m] for m in g.op_labels]
                for j, o in enumerate(g.ops):
                    lanes.append(Lane(dict(action=o.action, unit=o.unit, option=o.cleaning), o.success, slots, g.op_before[j], g.op_after[j],
                                      ~np.isnan(g.op_before[j]), o.unit == 0 and o.cleaning == 0, "%s call %d %r" % (name, j, o)))
        for j, c in enumerate(sc.calls):
            lanes.append(Lane(dict(action=c.action, unit=c.unit, option=c.cleaning), c.success, sc_slots, (sc.before, sc.before32), (sc.after, sc.after32),
                              np.ones(len(sc_slots), dtype=bool), c.unit == 0 and c.cleaning == 0, "scattered call %d %r" % (j, c)))
            lanes[-1].row = j
        k = 0
        while k < len(NOOP_ORDERS) or len(lanes) % 64 in (0, 63) or len(lanes) <= 192:      # never a whole number of waves
            o = NOOP_ORDERS[k % len(NOOP_ORDERS)]
            row = (17 * k + 3) % len(sc)
            lanes.append(Lane(dict(action=o["action"], unit=o["unit"], option=k % 6), False, sc_slots, (sc.before, sc.before32), (sc.before, sc.before32),
                              np.ones(len(sc_slots), dtype=bool), False, "no-op lane %r" % (o,)))
            lanes[-1].row = row; lanes[-1].noop = True
            k += 1
        lanes = _permuted(lanes, 2718)
        for p, lane in enumerate(lanes):
            a = lane.order["action"]
            kind = ACTIONS[a][0] if 0 <= a < len(ACTIONS) else None
            lane.unit_sent = junk_units[p % 2] if kind in ("steam_generator_system", "condenser") else lane.order["unit"]
            lane.option_sent = other_methods[p % 4] if lane.order["option"] == 5 else lane.order["option"]
        return lanes
    return _cached(("component lanes", replays), make)


def _resolved(lanes, f32):
    """the lanes with the scattered rows' arrays picked for the storage type (shared arrays, never written to)"""
    out = []
    for lane in lanes:
        if isinstance(lane.before, tuple):
            r = Lane(lane.order, lane.success, lane.slots, lane.before[f32][lane.row], lane.after[f32][lane.row], lane.valid, lane.default, lane.what)
        else:
            r = Lane(lane.order, lane.success, lane.slots, lane.before, lane.after, lane.valid, lane.default, lane.what)
        r.__dict__.update({k: v for k, v in lane.__dict__.items() if k not in r.__dict__})
        out.append(r)
    return out


def _component_launch(storage, defaults=False, log=False):
    from nuclear_sim_amd.env import BatchedPlantEnv
    f32 = storage == "f32"
    lanes = _resolved(_component_lanes(replays=not f32), int(f32))
    n = len(lanes)
    assert n > 192 and n % 64 != 0
    env = BatchedPlantEnv(n, dt=5.0, storage=storage, maintenance=log)
    if log:
        env.enable_maintenance_log(8192)
    env.step()
    clock = 5.0 * (1 + np.arange(n) % 7)

    def clocks(f0, i0):
        if log:
            f0[SCHEMA.slot("prim.sim_time")[1], :] = clock
    pre = _load(env, lanes, clocks)
    ordered = np.array([(lane.default if defaults else True) and not getattr(lane, "noop", False) for lane in lanes])
    action = np.array([lane.order["action"] if (ordered[p] or (not defaults)) else -1 for p, lane in enumerate(lanes)], dtype=np.int32)
    unit = None if defaults else np.array([lane.unit_sent for lane in lanes], dtype=np.int32)
    option = None if defaults else np.array([lane.option_sent for lane in lanes], dtype=np.int32)
    ok = env.perform_component_maintenance("condenser", action, unit=unit, cleaning_type=option).cpu().numpy()
    want = np.array([lane.success and ordered[p] for p, lane in enumerate(lanes)], dtype=np.uint8)
    assert np.array_equal(ok, want), "success: first lanes off %s" % [(p, lanes[p].what, int(ok[p])) for p in np.nonzero(ok != want)[0][:5]]
    assert want.sum() > 0.6 * ordered.sum() > 0
    # neighbours differ: no wave is of one kind
    if not defaults:
        for w in range(0, n, 64):
            kinds = {ACTIONS[a][0] for a in action[w:w + 64] if 0 <= a < len(ACTIONS)}
            assert len(kinds) >= 3 or n - w < 16, (w, kinds)
    worst = _check(env, lanes, ordered, pre, f32, "component kernel, %s storage%s" % (storage, ", optional columns NULL" if defaults else ""))
    return env, lanes, want, clock, worst


def test_component_kernel_every_call_a_lane_fp64():
    env, lanes, want, _clock, worst = _component_launch("f64")
    replays = sum("scattered" not in lane.what and "no-op" not in lane.what for lane in lanes)
    assert replays == 67 and sum("scattered" in lane.what for lane in lanes) >= 160 + 80 and sum("no-op" in lane.what for lane in lanes) >= 6
    assert worst["carried"] < CARRIED_RTOL
    env.close()


def test_component_kernel_every_call_a_lane_fp32_storage():
    env, lanes, _want, _clock, _worst = _component_launch("f32")
    assert sum("scattered" in lane.what for lane in lanes) >= 160 + 80 and sum("no-op" in lane.what for lane in lanes) >= 6
    env.close()


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_component_kernel_optional_columns_null(storage):
    """unit and option NULL: unit 0, the handlers' default cleaning type.  Only the calls recorded with those arguments are ordered"""
    env, lanes, want, _clock, _worst = _component_launch(storage, defaults=True)
    assert 20 < want.sum() < len(lanes) // 2
    env.close()


def test_component_kernel_logs_exactly_the_successful_lanes():
    env, lanes, want, clock, _worst = _component_launch("f64", log=True)
    rec = env.maintenance_log_records()
    rec = rec[rec["kind"] == OPERATOR_COMPONENT]
    got = sorted(zip(rec["plant"].tolist(), rec["action"].tolist(), rec["pump"].tolist()))
    wanted = sorted((p, lane.order["action"], lane.order["unit"] if UNITS[ACTIONS[lane.order["action"]][0]] > 1 else 0)
                    for p, lane in enumerate(lanes) if want[p])
    assert got == wanted and len(got) == int(want.sum())
    assert np.array_equal(rec["time"], clock[rec["plant"]]) and np.array_equal(rec["created"], rec["time"]) and np.all(rec["order"] == 0)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- the pump kernel
PUMP_NOOP_ORDERS = (dict(action=-1, pump=0), dict(action=len(PUMP_ACTIONS), pump=1), dict(action=PUMP_ACTIONS.index("oil_change"), pump=4),
                    dict(action=PUMP_ACTIONS.index("component_overhaul"), pump=-1), dict(action=PUMP_ACTIONS.index("npsh_analysis"), pump=2))


def _pump_lanes(replays=True):
    def make():
        by_label = _columns()[0]
        sc = ScatteredCalls("pumps")
        slots_of = [sc.slots(k) for k in range(4)]
        lanes = []
        if replays:
            for name in ("om1_every_handler", "om2_with_automatic_maintenance"):
                g = OperatorGolden(name)
                for j, o in enumerate(g.ops):
                    lanes.append(Lane(dict(action=o.action, pump=o.pump, bearing=o.bearing, target=o.target_level), o.success, g.pump_slots(o.pump),
                                      g.op_before[j], g.op_after[j], ~np.isnan(g.op_before[j]), o.bearing == 0 and np.isnan(o.target_level),
                                      "%s call %d %r" % (name, j, o)))
        for j, c in enumerate(sc.calls):
            lanes.append(Lane(dict(action=c.action, pump=c.pump, bearing=c.bearing, target=c.target_level, target_is_level=c.target_is_level), c.success,
                              slots_of[c.pump], (sc.before, sc.before32), (sc.after, sc.after32), np.ones(len(sc.labels), dtype=bool),
                              c.bearing == 0 and np.isnan(c.target_level), "scattered call %d %r" % (j, c)))
            lanes[-1].row = j
        k = 0
        while k < len(PUMP_NOOP_ORDERS) or len(lanes) % 64 in (0, 63) or len(lanes) <= 192:
            o = PUMP_NOOP_ORDERS[k % len(PUMP_NOOP_ORDERS)]
            lanes.append(Lane(dict(action=o["action"], pump=o["pump"], bearing=k % 4, target=70.0 + k), False, slots_of[k % 4], (sc.before, sc.before32),
                              (sc.before, sc.before32), np.ones(len(sc.labels), dtype=bool), False, "no-op lane %r" % (o,)))
            lanes[-1].row = (29 * k + 5) % len(sc); lanes[-1].noop = True
            k += 1
        lanes = _permuted(lanes, 3141)
        # the plant's other three pumps hold scattered values of their own
        rng = np.random.default_rng(1618)
        for lane in lanes:
            lane.others = [(slots_of[k], int(rng.integers(0, len(sc)))) for k in range(4) if k != lane.order["pump"] or lane.order["pump"] not in range(4)]
        return lanes, sc
    return _cached(("pump lanes", replays), make)


def _pump_launch(storage, defaults=False):
    from nuclear_sim_amd.env import BatchedPlantEnv
    f32 = storage == "f32"
    shared, sc = _pump_lanes(replays=not f32)
    lanes = _resolved(shared, int(f32))
    n = len(lanes)
    assert n > 192 and n % 64 != 0
    env = BatchedPlantEnv(n, dt=5.0, storage=storage)
    env.step()
    rows = (sc.before, sc.before32)[f32]

    def other_pumps(f0, i0):
        for p, lane in enumerate(lanes):
            mine = {s for s in lane.slots} if lane.order["pump"] in range(4) else set()
            for slots, row in lane.others:
                for (kind, slot), v in zip(slots, rows[row]):
                    if (kind, slot) in mine:
                        continue
                    if kind == "f64":
                        f0[slot, p] = v
                    else:
                        i0[slot, p] = int(v)
    pre = _load(env, lanes, other_pumps)
    ordered = np.array([(lane.default if defaults else True) and not getattr(lane, "noop", False) for lane in lanes])
    action = np.array([lane.order["action"] if (ordered[p] or not defaults) else -1 for p, lane in enumerate(lanes)], dtype=np.int32)
    pump = np.array([lane.order["pump"] for lane in lanes], dtype=np.int32)
    bearing = target = None
    if not defaults:
        bearing = np.array([lane.order["bearing"] for lane in lanes], dtype=np.int32)
        # a target "equal to the current level" is the level this storage type holds
        level = SCHEMA.slot("pump.oil_level", 0)[1], SCHEMA.slot("pump.oil_level", 1)[1] - SCHEMA.slot("pump.oil_level", 0)[1]
        target = np.array([95.0 if np.isnan(lane.order["target"]) else
                           pre[0][level[0] + level[1] * lane.order["pump"], p] if lane.order.get("target_is_level") else lane.order["target"]
                           for p, lane in enumerate(lanes)])
    ok = env.perform_maintenance(action, pump, bearing=bearing, target_level=target).cpu().numpy()
    want = np.array([lane.success and ordered[p] for p, lane in enumerate(lanes)], dtype=np.uint8)
    assert np.array_equal(ok, want), "success: first lanes off %s" % [(p, lanes[p].what, int(ok[p])) for p in np.nonzero(ok != want)[0][:5]]
    assert want.sum() > 0.6 * ordered.sum() > 0
    worst = _check(env, lanes, ordered, pre, f32, "pump kernel, %s storage%s" % (storage, ", optional columns NULL" if defaults else ""))
    return env, lanes, want, worst


def test_pump_kernel_every_call_a_lane_fp64():
    env, lanes, want, worst = _pump_launch("f64")
    assert sum("om" in lane.what.split()[0] for lane in lanes) >= 45 and sum("scattered" in lane.what for lane in lanes) >= 130 + 60
    assert {lane.order["bearing"] for lane in lanes if lane.order["action"] == PUMP_ACTIONS.index("bearing_replacement")} >= {-1, 0, 1, 2, 3, 4}
    assert worst["carried"] < CARRIED_RTOL
    env.close()


def test_pump_kernel_every_call_a_lane_fp32_storage():
    env, lanes, _want, _worst = _pump_launch("f32")
    assert sum("scattered" in lane.what for lane in lanes) >= 130 + 60
    env.close()


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_pump_kernel_optional_columns_null(storage):
    """bearing and target_level NULL: every bearing, a target of 95.0.  Only the calls recorded with those arguments are ordered"""
    env, lanes, want, _worst = _pump_launch(storage, defaults=True)
    assert 20 < want.sum() < len(lanes) // 2
    env.close()
