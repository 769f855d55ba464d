"""GPU: automatic maintenance of the steam generators and the condenser in one work-order queue with the feedwater pumps
(npb_set_component_maintenance; BatchedPlantEnv(component_maintenance=True)).

The reference's runs of tests/golden/auto_components/ (tools/make_auto_component_golden.py) replayed as ONE lane of a 70-plant batch of
as-built plants: every schema column at every step under golden_util's rule, the drained log against the reference's work orders field by
field -- the WO numbers included: pumps and components count from one counter --, the side state's stamps against
StateManager.threshold_last_violation_times; the other lanes equal to a run without the fixture lane.  Then: the committed pump
fixtures still pass with the feature on; every shipped step kernel, by name, in front of the rule kernel; fp32 storage; checkpoints,
snapshot / restore, masked resets; and with the feature off nothing moves."""
import glob
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN_DIR, Golden, compare_state, fixture_names
from work_order_events import host_state, make_env

pytestmark = pytest.mark.gpu

N, LANE = 70, 67      # the fixture's lane sits in the second wave, which is mostly padding
AC = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "auto_components", "ac*.npz")))
F32_OBS_RTOL = 1e-4     # the bar of tests/test_gpu_parity.py for fp32 storage against the reference's fixtures, on observations
PLAIN_KERNEL_OF_VARIANT = {1: "npb_step_kernel", 2: "npb_step2_wide_kernel", 5: "npb_step4_kernel"}


class Fixture:
    def __init__(self, name):
        self.g = Golden("auto_components/" + name)
        z = np.load(os.path.join(GOLDEN_DIR, "auto_components", name + ".npz"), allow_pickle=False)
        self.stamps = z["stamps"]
        self.side = json.load(open(os.path.join(GOLDEN_DIR, "auto_components", name + ".json")))
        # the run's table as component_thresholds takes it: the reference's dicts, in their order
        self.thresholds = {kind: dict((n, c) for n, c in self.side["table"][kind]) for kind in ("steam_generator", "condenser")}


def _env(fx, n=N, component_maintenance=True, **kw):
    env = make_env(fx.g, n=n, component_maintenance=component_maintenance,
                   component_thresholds=fx.thresholds if component_maintenance else None, **kw)
    env.log_naming = "composed"      # the fixtures' plants are the data-gen composer's: its provider ids
    return env


def _place(env, g, lane):
    """the fixture's initial state into one lane; the others stay as built"""
    f0, i0 = host_state(env)
    f, i, fm, im = g.split_state(g.state[0])
    f0[fm, lane] = f[fm]; i0[im, lane] = i[im]
    env.load_state_arrays(f0, i0)


def _step(env, g, t, lane):
    for label, v in g.pokes.get(t, []) if lane is not None else []:      # lane None: the pokes reach nobody; "all": every plant
        kind, slot = g.label_slot(label)
        col = env._get_slot(kind, slot)
        if lane == "all":
            col[:] = v
        else:
            col[lane] = v
        env._set_slot(kind, slot, col)
    sp = None if np.isnan(g.setpoint[t]) else g.setpoint[t]
    cw = None if np.isnan(g.cooling[t]) else g.cooling[t]
    return env.step(action=int(g.action[t]), magnitude=float(g.magnitude[t]), power_setpoint=sp, cooling_water_temp=cw, noise_z=float(g.noise_z[t]))


def _run(fx, lane=LANE, storage="f64", variant=0, steps=None, check=True, log=True, env=None, t0=0):
    """replay on a 70-plant batch; lane None = no fixture lane (the pokes then reach nobody).  Returns the env"""
    g = fx.g
    if env is None:
        env = _env(fx, storage=storage)
        env.set_step_kernel(variant)
        if log:
            env.enable_maintenance_log(4096)
        if lane is not None:
            _place(env, g, lane)
    for t in range(t0, g.T if steps is None else steps):
        obs, rew, done, _info = _step(env, g, t, lane)
        if variant:
            assert env.last_step_kernel() == PLAIN_KERNEL_OF_VARIANT[variant], env.last_step_kernel()
        if check and lane is not None:
            if storage == "f64":
                np.testing.assert_allclose(obs[lane].cpu().numpy(), g.obs[t], rtol=1e-6, atol=1e-12, err_msg="%s obs step %d" % (g.name, t))
                f, i = host_state(env)
                compare_state(g, f[:, lane], i[:, lane], g.state[t + 1], "state after step %d" % t)
            else:
                np.testing.assert_allclose(obs[lane].cpu().numpy(), g.obs[t], rtol=F32_OBS_RTOL, atol=1e-7, err_msg="%s obs step %d" % (g.name, t))
            side = env.component_maintenance_state().cpu().numpy()
            assert np.array_equal(side[:12, lane], fx.stamps[t + 1]), "%s: stamps after step %d: %s, the reference's %s" % (
                g.name, t, side[:12, lane], fx.stamps[t + 1])
    return env


def _orders_of(env, lane):
    """the drained log of one lane, joined by work order id"""
    cols = env.maintenance_log()
    out = {}
    for j in np.nonzero(cols["plant"] == lane)[0]:
        o = out.setdefault(cols["work_order_id"][j], {"completed": None, "success": None})
        created = cols["event_type"][j] == "work_order_created"
        for k, c in (("component_id", "component_id"), ("action", "action_type"), ("priority", "priority"), ("title", "title"),
                     ("work_order_type", "work_order_type")):
            if created or k not in o:
                o[k] = cols[c][j]
            elif cols[c][j] != "":      # a pump's completion record carries no priority: what it does carry must agree with the creation
                assert o[k] == cols[c][j], (cols["work_order_id"][j], k, o[k], cols[c][j])
        for k, c in (("created", "created_date"), ("planned", "planned_start_date")):
            v = float(cols[c][j])
            assert o.setdefault(k, v) == v, (cols["work_order_id"][j], k)
        if not created:
            o["completed"] = float(cols["actual_completion_date"][j]); o["success"] = bool(cols["success"][j])
    return out


def _assert_orders(env, fx, lane, exact_times=True):
    mine, theirs = _orders_of(env, lane), {o["work_order_id"]: o for o in fx.side["orders"]}
    assert sorted(mine) == sorted(theirs), "%s: orders %s, the reference's %s" % (fx.g.name, sorted(mine), sorted(theirs))
    for wid, o in theirs.items():
        for k in ("component_id", "action", "priority", "created", "planned", "completed", "success", "work_order_type", "title"):
            assert mine[wid][k] == o[k], "%s %s: %s is %r, the reference's %r" % (fx.g.name, wid, k, mine[wid][k], o[k])


@pytest.mark.parametrize("name", AC)
def test_fixture_replays_as_one_lane(name):
    """fails on a build without the feature: the generators are not cleaned, the orders and their numbers differ"""
    fx = Fixture(name)
    env = _run(fx)
    _assert_orders(env, fx, LANE)
    created = int(env.get_field("maint.work_orders_created")[LANE].item())
    performed = int(env.get_field("maint.maintenance_actions_performed")[LANE].item())
    assert {"work_orders_created": created, "maintenance_actions_performed": performed} == fx.side["counters"]
    # the other lanes: bit for bit what the same batch gives without the fixture lane
    f, i = host_state(env)
    side = env.component_maintenance_state().cpu().numpy()
    obs = env.get_observation().cpu().numpy().copy()
    plain = _run(fx, lane=None, log=False)
    pf, pi = host_state(plain)
    others = np.arange(N) != LANE
    assert np.array_equal(f[:, others].view(np.int64), pf[:, others].view(np.int64)) and np.array_equal(i[:, others], pi[:, others])
    assert np.array_equal(side[:, others], plain.component_maintenance_state().cpu().numpy()[:, others])
    assert np.array_equal(obs[others], plain.get_observation().cpu().numpy()[others])
    env.close(); plain.close()


def _pump_fixtures():
    out = []
    for n in fixture_names():
        if not (n.startswith("m") and n[1].isdigit()) and n[:3] not in ("z21", "z22", "z23", "z24", "z25", "z26"):
            continue
        g = Golden(n)
        if (g.meta.get("runner") or g.meta.get("state_management")) and not g.meta.get("feedwater_thresholds_only") and not g.resets:
            out.append(n)
    return out


@pytest.mark.parametrize("name", _pump_fixtures())
def test_pump_fixtures_pass_with_the_feature_on(name):
    """the committed maintenance fixtures were recorded with the reference's full table: with the components scanned too they replay
    as before, m6 / m7 now with their maint.* counters compared"""
    g = Golden(name)
    g.meta = dict(g.meta, maint_unchecked=False)
    env = make_env(g, n=64, component_maintenance=True)
    f0, i0 = host_state(env)
    f, i, fm, im = g.split_state(g.state[0])
    f0[fm, :] = f[fm, None]; i0[im, :] = i[im, None]
    env.load_state_arrays(f0, i0)
    steps = {int(s): j for j, s in enumerate(g.state_steps)}
    for t in range(g.T):
        obs, _rew, done, _info = _step(env, g, t, "all")
        np.testing.assert_allclose(obs[63].cpu().numpy(), g.obs[t], rtol=1e-6, atol=1e-12, err_msg="%s obs step %d" % (name, t))
        if t + 1 in steps:
            fs, is_ = host_state(env)
            compare_state(g, fs[:, 63], is_[:, 63], g.state[steps[t + 1]], "state after step %d (component maintenance on)" % t)
    env.close()


def test_pump_fixture_list_is_not_empty():
    names = _pump_fixtures()
    assert any(n.startswith("m6_") for n in names) and any(n.startswith("m7_") for n in names) and any(n.startswith("z2") for n in names), names


@pytest.mark.parametrize("variant", [1, 2, 5])
def test_same_result_behind_every_step_kernel(variant):
    fx = Fixture("ac1_shared_queue")
    env = _run(fx, variant=variant)
    _assert_orders(env, fx, LANE)
    env.close()


def test_fp32_storage():
    """observations at the fp32 bar; event steps, stamps and order numbers exact"""
    fx = Fixture("ac1_shared_queue")
    env = _run(fx, storage="f32")
    _assert_orders(env, fx, LANE)
    env.close()


def _bits(env):
    f, i = host_state(env)
    return f.view(np.int64), i, env.component_maintenance_state().cpu().numpy().view(np.int64)


def _same(a, b, where):
    for x, y, what in zip(a, b, ("f64", "i32", "side state")):
        assert np.array_equal(x, y), "%s: %s differs" % (where, what)


def test_checkpoint_and_snapshot_resume_identically():
    fx = Fixture("ac1_shared_queue")
    whole = _bits(_run(fx, check=False, log=False))
    # (a) state_arrays() + the side state into a fresh handle
    first = _run(fx, steps=30, check=False, log=False)
    f, i = first.state_arrays()
    side = first.component_maintenance_state()
    assert (side[:12] >= 0).any(), "no stamp at the checkpoint: the side state would not matter"
    fresh = _env(fx)
    fresh.load_state_arrays(f, i)
    fresh.load_component_maintenance_state(side)
    _same(_bits(_run(fx, env=fresh, t0=30, check=False)), whole, "checkpoint at step 30")
    # ... and without the side state the run differs (what ADVICE.md's first finding is about)
    bare = _env(fx)
    bare.load_state_arrays(f, i)
    assert not np.array_equal(_bits(_run(fx, env=bare, t0=30, check=False))[0], whole[0])
    # (b) snapshot(), step on, restore()
    first.snapshot()
    _run(fx, env=first, t0=30, steps=45, check=False)
    first.restore()
    _same(_bits(_run(fx, env=first, t0=30, check=False)), whole, "snapshot at step 30")
    for e in (first, fresh, bare):
        e.close()


def test_masked_reset_clears_the_masked_plants_side_state():
    fx = Fixture("ac1_shared_queue")
    env = _env(fx)
    for lane in (3, LANE):
        _place(env, fx.g, lane)
    for t in range(4):
        _step(env, fx.g, t, LANE)
    before = env.component_maintenance_state().cpu().numpy()
    assert (before[12:24, 3] > 0).any() and np.array_equal(before[:, 3], before[:, LANE])
    mask = np.zeros(N, dtype=np.uint8); mask[3] = 1
    env.reset(mask=mask)
    after = env.component_maintenance_state().cpu().numpy()
    fresh = np.concatenate([np.full(12, -1.0), np.zeros(48), np.full(12, -1.0)])
    assert np.array_equal(after[:, 3], fresh)
    others = np.arange(N) != 3
    assert np.array_equal(after[:, others], before[:, others])
    env.close()


def test_off_means_off():
    """a handle that had the feature switched on -- it owns a side buffer -- and off again (NULL) before the first step gives, over 40 steps
    of a 65-plant heterogeneous batch, to the bit what a handle gives on which the feature was never mentioned; the rule stays inside the step
    kernels, and the fixture lane still matches m1 as it did"""
    from nuclear_sim_amd import _lib
    g = Golden("m1_oil_top_off_staggered")
    rng = np.random.default_rng(11)
    levels = rng.uniform(57.0, 60.0, (4, 65))
    z = rng.standard_normal((40, 65))
    steps = {int(s): j for j, s in enumerate(g.state_steps)}
    out = []
    for had_it_on in (False, True):
        env = make_env(g, n=65, component_maintenance=had_it_on)
        if had_it_on:
            assert env.component_maintenance_state().shape == (_lib.CMAINT_SIDE_DOUBLES, 65)
            _lib.check(env.L.npb_set_component_maintenance(env._h, None), env._h)
        f0, i0 = host_state(env)
        f, i, fm, im = g.split_state(g.state[0])
        f0[fm, 64] = f[fm]; i0[im, 64] = i[im]
        env.load_state_arrays(f0, i0)
        for k in range(4):
            col = env.get_field("pump.oil_level", instance=k)
            col[:64] = env._col(levels[k], col.dtype)[:64]
            env.set_field("pump.oil_level", col, instance=k)
        for t in range(40):
            noise = z[t].copy(); noise[64] = g.noise_z[t]
            sp = np.full(65, 90.0); sp[64] = g.setpoint[t]
            obs, _r, _d, _info = env.step(power_setpoint=sp, noise_z=noise)
            assert env.last_step_kernel().endswith("_maint_kernel")      # the rule inside the step kernels, as before
            np.testing.assert_allclose(obs[64].cpu().numpy(), g.obs[t], rtol=1e-6, atol=1e-12)
            if t + 1 in steps:
                fs, is_ = host_state(env)
                compare_state(g, fs[:, 64], is_[:, 64], g.state[steps[t + 1]], "m1 lane after step %d" % t)
        fs, is_ = host_state(env)
        assert int(is_.max()) > 0 and int(env.get_field("maint.work_orders_created").sum().item()) > 0      # the pump rule did work in this batch
        out.append((fs.view(np.int64), is_))
        env.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_refusals_by_name():
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    with pytest.raises(ValueError, match="maintenance=True"):
        BatchedPlantEnv(4, component_maintenance=True)
    with pytest.raises(_lib.NpbError, match="unknown steam_generator threshold parameter"):
        BatchedPlantEnv(4, dt=5.0, maintenance=True, component_maintenance=True, component_thresholds={"steam_generator": {"bogus": {"threshold": 1.0, "action": "scale_removal"}}})
    with pytest.raises(_lib.NpbError, match="not in the component catalog"):
        BatchedPlantEnv(4, dt=5.0, maintenance=True, component_maintenance=True,
                        component_thresholds={"steam_generator": {"steam_quality": {"threshold": 1.0, "action": "condenser_tube_plugging"}}})
    bank = BatchedPlantEnv(8, dt=5.0, maintenance=True)
    env = BatchedPlantEnv(8, dt=5.0, maintenance=True, component_maintenance=True)
    with pytest.raises(_lib.NpbError, match="the bank handle has not"):
        env.set_start_bank(bank)
    bank.close(); env.close()


def test_autoreset_and_bank_restore_the_side_state():
    """a truncated episode restarts from the snapshot, the side state with it: steps 6..11 repeat steps 0..5 to the bit; the same from a
    start bank copied from a batch that has the feature on"""
    import torch
    fx = Fixture("ac1_shared_queue")
    g = fx.g
    for bank in (False, True):
        env = _env(fx)
        _place(env, g, LANE)
        env.snapshot()
        env._enable_autoreset(6)
        if bank:
            env.set_start_bank(env)      # entry p = plant p's start state, the side state beside it
        seen = []
        for t in range(12):
            sp = g.setpoint[t % 6]
            obs, _r, _d, info = env.step(power_setpoint=sp, noise_z=float(g.noise_z[t % 6]))
            seen.append((obs.cpu().numpy().copy(), info["truncated"].cpu().numpy().copy()))
            if t in (4, 10):
                before_reset = _bits(env)
        assert seen[5][1].all() and seen[11][1].all() and not seen[4][1].any()
        side = env.component_maintenance_state().cpu().numpy()
        assert (before_reset[2][:12, LANE].view(np.float64) >= 0).any() and (side[:, LANE][:12] == -1.0).all()      # stamped, then back to the start's
        for t in range(5):
            assert np.array_equal(seen[t][0], seen[t + 6][0]), "step %d of the second episode (bank %s)" % (t, bank)
        env.close()


def test_switching_off_and_on_keeps_the_pump_rule_right():
    """the feature switched off in mid-run hands the rule back to the step kernels (whose cooldown cache is rebuilt): m1 replays as it
    does on a handle that never had it on -- no component of m1 crosses anything"""
    from nuclear_sim_amd import _lib
    import ctypes
    g = Golden("m1_oil_top_off_staggered")
    env = make_env(g, n=64, component_maintenance=True)
    f0, i0 = host_state(env)
    f, i, fm, im = g.split_state(g.state[0])
    f0[fm, :] = f[fm, None]; i0[im, :] = i[im, None]
    env.load_state_arrays(f0, i0)
    table = _lib.NpbComponentMaintTable()
    env.L.npb_default_component_maintenance_table(ctypes.byref(table))
    steps = {int(s): j for j, s in enumerate(g.state_steps)}
    for t in range(g.T):
        if t % 7 == 3:
            on = (t // 7) % 2 == 1
            _lib.check(env.L.npb_set_component_maintenance(env._h, ctypes.byref(table) if on else None), env._h)
        _step(env, g, t, "all")
        if t + 1 in steps:
            fs, is_ = host_state(env)
            compare_state(g, fs[:, 5], is_[:, 5], g.state[steps[t + 1]], "state after step %d" % t)
    env.close()
