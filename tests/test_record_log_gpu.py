"""GPU: the slot hand-out the three record logs share (csrc/npd_record_log.h), seen as the RAW slots on the device, before a drain sorts
them: the maintenance event log, the episode records and the event windows.

70 plants: one full wave and one of six lanes.  The wanting plants are 1, 5, 63 of the first wave -- its lane 0 does not want -- and 64, 69
of the second: its lane 0 and its last live lane.  Each log gets one record per wanting plant: the maintenance log by a masked operator
order, the episode records and the event windows by the low-flow poke of tests/test_event_windows_gpu.py, which makes a plant scram, and
with autoreset end its episode and its capture, on the next step.  What the hand-out promises: the cursor counts every wanting lane; the
plants are exactly the wanting set; the slots of one wave are adjacent and rise with the plant.  Which wave comes first is not defined.
Past the capacity the cursor goes on counting and nothing is written."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, WAVE = 70, 64
WANT = [1, 5, 63, 64, 69]
SENTINEL = 0xAB


def _np(t):
    return t.detach().cpu().numpy().copy()


def _assert_hand_out(cursor, plants, where):
    """plants: the raw plant column up to the cursor"""
    assert cursor == len(WANT), (where, cursor)
    plants = [int(p) for p in plants]
    assert sorted(plants) == WANT, (where, plants)
    for wave in range((N + WAVE - 1) // WAVE):
        slots = [k for k, p in enumerate(plants) if p // WAVE == wave]
        mine = [plants[k] for k in slots]
        assert slots == list(range(slots[0], slots[0] + len(slots))) and mine == sorted(mine), (where, wave, plants)


def _operator_orders(env, capacity):
    """a log of the test's own behind `capacity`, 8 records of sentinel bytes; one masked order; (cursor, the 8 raw records, their bytes)"""
    from nuclear_sim_amd import _lib, maintlog
    nb = maintlog.EVENT_DTYPE.itemsize
    buf = torch.full((8 * nb,), SENTINEL, dtype=torch.uint8, device=env.device)
    cursor = torch.zeros(1, dtype=torch.int32, device=env.device)
    _lib.check(env.L.npb_set_maintenance_log(env._h, ctypes.c_void_p(buf.data_ptr()), capacity, ctypes.c_void_p(cursor.data_ptr())), env._h)
    mask = np.zeros(N, dtype=np.uint8); mask[WANT] = 1
    ok = env.perform_maintenance("oil_top_off", 0, mask=mask)
    assert np.flatnonzero(_np(ok)).tolist() == WANT
    raw = _np(buf)
    _lib.check(env.L.npb_set_maintenance_log(env._h, None, 0, None), env._h)
    return int(_np(cursor)[0]), raw.view(maintlog.EVENT_DTYPE), raw.reshape(8, nb)


def test_maintenance_log_raw_slots_and_capacity():
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv(N, dt=5.0, maintenance=True)
    cursor, rec, raw = _operator_orders(env, 8)
    assert np.all(rec["kind"][:5] == 2) and np.all(rec["action"][:5] == _lib.maint_action_index("oil_top_off")) and np.all(rec["pump"][:5] == 0)
    _assert_hand_out(cursor, rec["plant"][:cursor], "maintenance log")
    assert np.all(raw[5:] == SENTINEL)
    # capacity 2: all five are counted, the two lowest slots are written -- the first two plants of the wave that came first --, no byte behind them
    cursor, rec, raw = _operator_orders(env, 2)
    assert cursor == len(WANT)
    assert rec["plant"][:2].tolist() in ([1, 5], [64, 69]) and np.all(rec["kind"][:2] == 2)
    assert np.all(raw[2:] == SENTINEL), "a record was written past the capacity"
    env.close()


def test_episode_records_and_event_windows_raw_slots():
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(N), dt=5.0, autoreset=True, max_episode_steps=12)
    env.enable_episode_records(16)
    env.enable_event_windows([("pump.oil_level", 0)], [("trip", 0xFFFFFFFF)], 1, 1, capacity=16)
    sp = np.full(N, 90.0)
    for t in range(3):
        if t == 2:      # the ring holds two samples: the trigger is primed
            v = _np(env.get_field("prim.coolant_flow_rate"))
            v[WANT] = 4000.0
            env.set_field("prim.coolant_flow_rate", v)
        _obs, _rew, done, _info = env.step(power_setpoint=sp)
    assert np.flatnonzero(_np(done)).tolist() == WANT
    for name, log in (("episode records", env._erec), ("event windows", env._ewin)):
        cursor = int(_np(log["cursor"])[0])
        _assert_hand_out(cursor, _np(log["dev"]["plant"])[:cursor], name)
        assert np.all(_np(log["dev"]["step"])[:cursor] == 2)
    # the drains sort what the waves left in either order
    assert env.episode_records()["plant"].tolist() == WANT and env.event_windows()["plant"].tolist() == WANT
    env.close()
