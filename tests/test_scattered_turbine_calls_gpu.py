"""GPU: the turbine's operator-maintenance kernel (npb_operator_turbine_maint_kernel) with one reference call per LANE.  Every call of the
replay fixtures (tests/golden/operator_turbine/ot1-ot4) and of the scattered-call fixtures (tests/golden/operator_calls/turbine/: a seeded
draw of every real member of turb and tstg, the handlers' caps and floors pinned on the edge and from both sides, NaN members) gets a lane
of its own in ONE launch, in a fixed permutation and never whole waves, beside lanes that order nothing that exists; neighbours differ in
kind, unit and action, and lanes of the turbine and the lubrication system carry junk units.  Every lane is checked in every schema
column: turb and tstg against the reference's values after the call, everything else against its own bits before the launch.

The machinery (Lane, _load, _check) and the tolerances are those of tests/test_scattered_calls_gpu.py: fp64 storage -- integers, NaN
positions and success exact, carried real members 1e-12 relative, the members the arena keeps as float at the contract's 1e-6; fp32
storage -- the reference's own result from the float32-rounded inputs within one float32 ulp."""
import numpy as np
import pytest

from test_scattered_calls_gpu import CARRIED_RTOL, Lane, _cached, _check, _columns, _load, _permuted, _resolved
from turbine_maintenance_golden import ACTIONS, REPLAYED, UNITS, ScatteredTurbineCalls, TurbineGolden
from nuclear_sim_amd.schema import SCHEMA

pytestmark = pytest.mark.gpu

OPERATOR_TURBINE = 4
A = lambda kind, name: ACTIONS.index((kind, name))
NOOP_ORDERS = (dict(action=-1, unit=0), dict(action=len(ACTIONS), unit=0), dict(action=1000, unit=1),
               dict(action=A("bearing", "turbine_bearing_replacement"), unit=4), dict(action=A("stage", "overhaul"), unit=14),
               dict(action=A("stage", "blade_replacement"), unit=-1), dict(action=A("bearing", "thrust_bearing_adjustment"), unit=3),
               dict(action=A("bearing", "routine_maintenance"), unit=-3))


def _turbine_lanes(replays=True):
    def make():
        by_label = _columns()[0]
        sc = ScatteredTurbineCalls()
        lanes = []
        if replays:
            for name in REPLAYED:
                g = TurbineGolden(name)
                slots = [by_label[m] for m in g.op_labels]
                for j, o in enumerate(g.ops):
                    lanes.append(Lane(dict(action=o.action, unit=o.unit), o.success, slots, g.op_before[j], g.op_after[j], ~np.isnan(g.op_before[j]),
                                      o.unit == 0, "%s call %d %r" % (name, j, o)))
        for j, c in enumerate(sc.calls):
            lanes.append(Lane(dict(action=c.action, unit=c.unit), c.success, sc.slots, (sc.before, sc.before32), (sc.after, sc.after32),
                              np.ones(len(sc.slots), dtype=bool), c.unit == 0, "scattered call %d %r" % (j, c)))
            lanes[-1].row = j
        k = 0
        while k < len(NOOP_ORDERS) or len(lanes) % 64 in (0, 63) or len(lanes) <= 192:      # never a whole number of waves
            o = NOOP_ORDERS[k % len(NOOP_ORDERS)]
            lanes.append(Lane(dict(action=o["action"], unit=o["unit"]), False, sc.slots, (sc.before, sc.before32), (sc.before, sc.before32),
                              np.ones(len(sc.slots), dtype=bool), False, "no-op lane %r" % (o,)))
            lanes[-1].row = (17 * k + 3) % len(sc); lanes[-1].noop = True
            k += 1
        lanes = _permuted(lanes, 31415)
        junk_units = (7, -2, 100)
        for p, lane in enumerate(lanes):
            a = lane.order["action"]
            kind = ACTIONS[a][0] if 0 <= a < len(ACTIONS) else None
            lane.unit_sent = junk_units[p % 3] if kind in ("turbine", "lubrication") else lane.order["unit"]
        return lanes
    return _cached(("turbine lanes", replays), make)


def _turbine_launch(storage, defaults=False, log=False):
    from nuclear_sim_amd.env import BatchedPlantEnv
    f32 = storage == "f32"
    lanes = _resolved(_turbine_lanes(replays=not f32), int(f32))
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
    ok = env.perform_turbine_maintenance("turbine", action, unit=unit).cpu().numpy()
    want = np.array([lane.success and ordered[p] for p, lane in enumerate(lanes)], dtype=np.uint8)
    assert np.array_equal(ok, want), "success: first lanes off %s" % [(p, lanes[p].what, int(ok[p])) for p in np.nonzero(ok != want)[0][:5]]
    assert want.sum() > 0.6 * ordered.sum() > 0
    if not defaults:      # neighbours differ: no wave is of one kind
        for w in range(0, n, 64):
            kinds = {ACTIONS[a][0] for a in action[w:w + 64] if 0 <= a < len(ACTIONS)}
            assert len(kinds) >= 3 or n - w < 16, (w, kinds)
    worst = _check(env, lanes, ordered, pre, f32, "turbine kernel, %s storage%s" % (storage, ", unit NULL" if defaults else ""))
    return env, lanes, want, clock, worst


def test_turbine_kernel_every_call_a_lane_fp64():
    env, lanes, want, _clock, worst = _turbine_launch("f64")
    replays = sum("scattered" not in lane.what and "no-op" not in lane.what for lane in lanes)
    assert replays >= 100 and sum("scattered" in lane.what for lane in lanes) >= 250 and sum("no-op" in lane.what for lane in lanes) >= len(NOOP_ORDERS)
    assert worst["carried"] < CARRIED_RTOL
    env.close()


def test_turbine_kernel_every_call_a_lane_fp32_storage():
    env, lanes, _want, _clock, _worst = _turbine_launch("f32")
    assert sum("scattered" in lane.what for lane in lanes) >= 250 and sum("no-op" in lane.what for lane in lanes) >= len(NOOP_ORDERS)
    env.close()


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_turbine_kernel_unit_null(storage):
    """a second launch with the unit column NULL: unit 0.  Only the calls recorded on unit 0 are ordered"""
    env, lanes, want, _clock, _worst = _turbine_launch(storage, defaults=True)
    assert 20 < want.sum() < len(lanes)
    env.close()


def test_turbine_kernel_logs_exactly_the_successful_lanes():
    env, lanes, want, clock, _worst = _turbine_launch("f64", log=True)
    rec = env.maintenance_log_records()
    rec = rec[rec["kind"] == OPERATOR_TURBINE]
    got = sorted(zip(rec["plant"].tolist(), rec["action"].tolist(), rec["pump"].tolist()))
    wanted = sorted((p, lane.order["action"], lane.order["unit"] if UNITS[ACTIONS[lane.order["action"]][0]] > 1 else 0)
                    for p, lane in enumerate(lanes) if want[p])
    assert got == wanted and len(got) == int(want.sum())
    assert np.array_equal(rec["time"], clock[rec["plant"]]) and np.array_equal(rec["created"], rec["time"]) and np.all(rec["order"] == 0)
    env.close()
