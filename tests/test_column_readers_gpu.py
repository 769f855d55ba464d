"""GPU: the three consumers of a per-plant column -- the column statistics' fold, the event windows and the task -- read it through one
reader (npd_column_read) and must see the same bits for the same column, for every kind of descriptor: a carried fp64 member, an output
member stored as float, an int32 member, an info column with its plant stride, an obs column, the reward, and for the task the int32 and
uint8 sides.  The reference is env.task_samples(), which gathers through npb_get_field and tensor indexing and not through the reader.

The run: BatchedPlantEnv.action_test("oil_top_off", seeds=range(n), dt=5.0), two steps, every plant with a setpoint of its own.  The work
counter is set to plant + 1 and the steam temperature (obs 5) to 285 + plant / 10 before the first step, and a few plants get a fuel
temperature of 1500 before the second (they scram on it), so that no column is the same in every plant.  The windows' one trigger is
the plant clock passing a value between its first and second sample: every plant captures one one-row window on the second step."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 5.0
SHARED = [("pump.oil_level", 1),                          # a carried fp64 member
          ("sg.tube_wall_temp", 0),                       # an OUTPUT member: the arena stores it as float
          "maint.maintenance_actions_performed",          # an int32 member
          ("info", "electrical_power"),                   # a side row with a plant stride
          ("obs", 5), "reward"]
TASK_ONLY = ["flags", "done"]                             # an int32 and a uint8 side
SCRAMS = [5, 66, 130]                                     # plants past the batch are left out


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("n, segment", [(70, 0), (192, 64)])      # a full wave and a ragged one; three segments inside one block of the fold's grid
def test_the_three_consumers_see_the_same_bits(monkeypatch, n, segment, storage):
    from nuclear_sim_amd.env import BatchedPlantEnv
    monkeypatch.setenv("NPB_ARENA_SEGMENT", str(segment))
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, storage=storage)
    assert int(env.L.npb_state_arena_segment(env._h)) == segment
    env.set_field("maint.maintenance_actions_performed", np.arange(1, n + 1, dtype=np.int32))
    env.set_field("prim.steam_temperature", 285.0 + 0.1 * np.arange(n))      # obs 5 is this over 300; it relaxes towards the coolant's by half per step
    start = _np(env.get_field("prim.sim_time"))
    limit = float(start.max()) + 1.5 * env.dt      # (the clock advances by dt with every step)
    env.set_task(reward=[(c, 1.0) for c in SHARED + TASK_ONLY], keep_terms=True)      # a value term of weight 1: the sample itself
    env.enable_column_stats(SHARED, stats=("last",))
    env.enable_event_windows(SHARED, triggers=[("prim.sim_time", ">", limit)], pre=0, post=0)
    clocks = []
    for t in range(2):
        if t == 1:
            plants = [p for p in SCRAMS if p < n]
            fuel = _np(env.get_field("prim.fuel_temperature")); fuel[plants] = 1500.0
            env.set_field("prim.fuel_temperature", fuel)
        obs, rew, done, info = env.step(power_setpoint=90.0 + 8.0 * np.sin(2.0 * np.pi * t / (20.0 + np.arange(n) % 7)))
        clocks.append(_np(env.get_field("prim.sim_time")))
    assert np.all(clocks[0] < limit) and np.all(clocks[1] > limit)      # the trigger's edge lies on the second step, for every plant
    want = _np(env.task_samples())
    assert want.shape == (len(SHARED) + len(TASK_ONLY), n)
    for row, col in zip(want, SHARED + TASK_ONLY):
        assert len(np.unique(row)) > 1, "the column %r is the same in every plant: a reader on the wrong plant would pass" % (col,)
    shared = _bits(want[:len(SHARED)])
    terms = _bits(_np(info["task_terms"]))
    last = _bits(_np(env.column_stats()["last"]))
    win = env.event_windows()
    assert len(win["plant"]) == n and np.array_equal(win["plant"], np.arange(n)) and np.all(win["step"] == 1)      # (an empty drain cannot pass)
    assert win["values"].shape == (n, 1, len(SHARED))
    windows = _bits(win["values"][:, 0, :].T)
    assert np.array_equal(terms, _bits(want)), np.argwhere(terms != _bits(want))[:4]
    assert np.array_equal(last, shared), np.argwhere(last != shared)[:4]
    assert np.array_equal(windows, shared), np.argwhere(windows != shared)[:4]
    env.close()
