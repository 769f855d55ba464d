"""GPU: operator-ordered maintenance (npb_perform_maintenance, BatchedPlantEnv.perform_maintenance).  The handlers a caller orders
between two steps do to the plant what the reference's pump.perform_maintenance does (fixtures tests/golden/operator/, every step
kernel, full and ragged batches); an operator top-off is the automatic one; nothing ordered changes nothing; the result does not depend
on the arena's layout; the event log reports the orders; an autoreset takes them away with the episode."""
import json
import os

import numpy as np
import pytest

from golden_util import ATOL_SMALL, GOLDEN_DIR, RTOL, Golden, compare_state
from operator_maintenance_golden import OperatorGolden
from work_order_events import events_from_golden, host_state, make_env

pytestmark = pytest.mark.gpu

# which kernel npb_step launches for a forced variant at a batch of <= 32 768 plants in full mode (tests/test_gpu_parity.py)
KERNEL_OF_VARIANT = {0: "npb_step4_kernel", 1: "npb_step_kernel", 2: "npb_step2_wide_kernel", 3: "npb_step2_kernel", 4: "npb_step_nt_kernel",
                     5: "npb_step4_kernel"}
BEARING_REPLACEMENT = 7
OPERATOR = 2


def _want_kernel(env, variant):
    k = KERNEL_OF_VARIANT[variant]
    return k.replace("_kernel", "_maint_kernel") if env.params.maint_enabled else k


def _start(g, n, storage="f64", **kw):
    env = make_env(g, n=n, storage=storage, **kw)
    f0, i0 = host_state(env)
    f, i, fm, im = g.split_state(g.state[0])
    f0[fm, :] = f[fm, None]; i0[im, :] = i[im, None]
    env.load_state_arrays(f0, i0)
    return env


def _order(env, j, o, mask=None):
    """the fixture's call j through the Python surface, spelt differently from call to call (name / index, FWP-n / number)"""
    kw = {}
    if o.action_name == "bearing_replacement":
        kw["bearing"] = {0: None if j % 2 else "all", 1: "motor_bearings", 2: "pump_bearings", 3: 3}[o.bearing]
    if not np.isnan(o.target_level):
        kw["target_level"] = o.target_level
    return env.perform_maintenance(o.action_name if j % 2 == 0 else o.action, "FWP-%d" % (o.pump + 1) if j % 3 == 0 else o.pump, mask=mask, **kw)


def _compare_pump(g, env, pump, want, lanes, where):
    """the section of one pump against a fixture row of its members: the parity contract (tests/test_gpu_parity.py: reals within RTOL
    with the absolute floor, integer members exact)"""
    bad = []
    for (kind, slot), m, v in zip(g.pump_slots(pump), g.op_labels, want):
        if np.isnan(v):
            continue
        col = env._get_slot(kind, slot).cpu().numpy()
        for lane in lanes:
            mine = col[lane]
            if kind == "i32":
                if int(mine) != int(v):
                    bad.append((m, lane, int(mine), int(v)))
            elif not (abs(float(mine) - v) <= RTOL * abs(v) + ATOL_SMALL):
                bad.append((m, lane, float(mine), float(v)))
    assert not bad, "%s %s: %d mismatching members, first: %s" % (g.name, where, len(bad), bad[:5])


def _replay(name, variant, storage="f64", n=64, ordered=None, log=None, check=True):
    """the fixture on n lanes with its operator calls; ordered = the lanes that receive them (None = all).  Checks (lanes = the first
    and the last ordered one): success, the pump section after every call, obs / reward / done at every step, every schema column at
    every recorded step.  Returns (env, per-step maintenance_event_count of the first checked lane)."""
    import torch
    g = OperatorGolden(name)
    env = _start(g, n, storage)
    env.set_step_kernel(variant)
    if log:
        env.enable_maintenance_log(log)
    lanes = np.arange(n) if ordered is None else np.asarray(ordered)
    mask = None
    if ordered is not None:
        mask = torch.zeros(n, dtype=torch.uint8, device=env.device)
        mask[torch.as_tensor(lanes, device=env.device)] = 1
    probe = (int(lanes[0]), int(lanes[-1]))
    sampled = {int(s): k for k, s in enumerate(g.state_steps)}
    counts = []
    for t in range(g.T):
        for j, o in g.ops_at(t):
            ok = _order(env, j, o, mask).cpu().numpy()
            want = np.zeros(n, dtype=np.uint8); want[lanes] = int(o.success)
            assert np.array_equal(ok, want), "%s call %d %r: success %s" % (name, j, o, ok[:8])
            if check:
                _compare_pump(g, env, o.pump, g.op_after[j], probe, "after call %d %r (variant %d)" % (j, o, variant))
        sp = None if np.isnan(g.setpoint[t]) else g.setpoint[t]
        cw = None if np.isnan(g.cooling[t]) else g.cooling[t]
        obs, rew, done, info = env.step(action=int(g.action[t]), magnitude=float(g.magnitude[t]), power_setpoint=sp, cooling_water_temp=cw,
                                        noise_z=float(g.noise_z[t]))
        assert env.last_step_kernel() == _want_kernel(env, variant), env.last_step_kernel()
        if "maintenance_event_count" in info:
            counts.append(int(info["maintenance_event_count"][probe[0]].item()))
        if not check:
            continue
        obs = obs.cpu().numpy(); rew = rew.cpu().numpy(); done = done.cpu().numpy()
        for lane in probe:
            np.testing.assert_allclose(obs[lane], g.obs[t], rtol=RTOL, atol=1e-12, err_msg="%s obs step %d lane %d" % (name, t, lane))
            np.testing.assert_allclose(rew[lane], g.reward[t], rtol=RTOL, atol=1e-9, err_msg="%s reward step %d" % (name, t))
            assert int(done[lane]) == int(g.done[t]), "%s done step %d" % (name, t)
        if t + 1 in sampled:
            fs, is_ = host_state(env)
            for lane in probe:
                compare_state(g, fs[:, lane], is_[:, lane], g.state[sampled[t + 1]], "after step %d (lane %d, variant %d)" % (t, lane, variant))
    return env, g, counts


# ---------------------------------------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", ["om1_every_handler", "om2_with_automatic_maintenance"])
def test_operator_calls_replay_the_reference_on_every_step_kernel(name, variant):
    """64 copies of the fixture's plant; the op kernel is the same for every variant, the state it hands on is read by each step kernel"""
    env, g, _ = _replay(name, variant)
    assert sum(o.success for o in g.ops) >= 2
    env.close()


def test_ragged_batch_only_odd_lanes_ordered():
    """100 lanes (a full wave and a ragged one), the calls masked to the odd lanes: those follow the reference, the even lanes are a
    run without any call, bit for bit"""
    import torch
    name = "om1_every_handler"
    n = 100
    odd = np.arange(1, n, 2)
    env, g, _ = _replay(name, 0, n=n, ordered=odd)
    fa, ia = env.state_arrays()
    plain = _start(g, n)
    for t in range(g.T):
        sp = None if np.isnan(g.setpoint[t]) else g.setpoint[t]
        cw = None if np.isnan(g.cooling[t]) else g.cooling[t]
        plain.step(action=int(g.action[t]), magnitude=float(g.magnitude[t]), power_setpoint=sp, cooling_water_temp=cw, noise_z=float(g.noise_z[t]))
    fb, ib = plain.state_arrays()
    assert torch.equal(fa[:, 0::2].contiguous().view(torch.int64), fb[:, 0::2].contiguous().view(torch.int64)) and torch.equal(ia[:, 0::2], ib[:, 0::2])
    assert not torch.equal(fa[:, 1::2].contiguous().view(torch.int64), fb[:, 1::2].contiguous().view(torch.int64))
    env.close(); plain.close()


def test_fp32_storage_follows_the_calls():
    """fp32 storage has no reference counterpart (values rounded to float once per store): success is the reference's, the ordered
    plants' observations stay within the fp32 mode's 1e-4 of the fixture (tests/test_gpu_parity.py), an unordered lane equals a run
    without calls bit for bit"""
    import torch
    name = "om1_every_handler"
    g = OperatorGolden(name)
    n = 100
    envs = [_start(g, n, "f32"), _start(g, n, "f32")]
    mask = torch.zeros(n, dtype=torch.uint8, device=envs[0].device); mask[1::2] = 1
    for t in range(g.T):
        for j, o in g.ops_at(t):
            ok = _order(envs[0], j, o, mask).cpu().numpy()
            assert np.array_equal(ok[1::2], np.full(n // 2, int(o.success))) and not ok[0::2].any()
        sp = None if np.isnan(g.setpoint[t]) else g.setpoint[t]
        for e in envs:
            obs, _, _, _ = e.step(action=int(g.action[t]), magnitude=float(g.magnitude[t]), power_setpoint=sp, noise_z=float(g.noise_z[t]))
        np.testing.assert_allclose(envs[0]._obs[99].cpu().numpy(), g.obs[t], rtol=1e-4, atol=1e-7, err_msg="fp32 obs step %d" % t)
    (fa, ia), (fb, ib) = envs[0].state_arrays(), envs[1].state_arrays()
    assert torch.equal(fa[:, 0::2].contiguous().view(torch.int64), fb[:, 0::2].contiguous().view(torch.int64)) and torch.equal(ia[:, 0::2], ib[:, 0::2])
    for e in envs:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 2. automatic = operator
@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_operator_top_off_is_the_automatic_top_off(storage):
    """Fixture m1's plant twice.  X: the automatic maintenance as the fixture ran it, with the event log on.  Y: the same table without
    its oil_level row (a table set explicitly is taken as given, so the two maint_oil_level_* params do not put the row back), and an
    operator oil_top_off with target params.maint_top_off_target right after every step in which X's log reports a completion for the
    pump.  The automatic rule runs after the physics inside the step launch, the operator's kernel after the launch: the plants must
    agree in every pump.*, fw.*, sg.*, turb.*, cond.*, prim.* column and in the observations at every step, by the criterion
    test_the_two_step_kernels_agree (tests/test_gpu_parity.py) uses for two compilations of the same device functions: integers exact,
    reals 1e-12 relative."""
    from nuclear_sim_amd import _lib
    g = Golden("m1_oil_top_off_staggered")
    n = 64
    rows = json.load(open(os.path.join(GOLDEN_DIR, "maint_table.json")))["thresholds"]
    without = {r["name"]: r for r in rows if r["name"] != "oil_level"}
    assert len(without) == len(rows) - 1
    X = _start(g, n, storage)
    Y = _start(g, n, storage, maintenance_thresholds=without)
    X.enable_maintenance_log(4096)
    target = float(X.params.maint_top_off_target)
    top_off = _lib.MAINT_ACTIONS.index("oil_top_off")
    labels = [c[2] for c in g.cols]
    watched = np.array([lab.startswith(("pump[", "fw.", "sg[", "turb.", "cond.", "prim.")) for lab in labels])
    assert watched.sum() > 400
    fsel = np.array([slot for (kind, slot, lab, _p), w in zip(g.cols, watched) if w and kind == "f64"])
    isel = np.array([slot for (kind, slot, lab, _p), w in zip(g.cols, watched) if w and kind == "i32"])
    completions = 0
    worst = 0.0
    for t in range(g.T):
        sp = None if np.isnan(g.setpoint[t]) else g.setpoint[t]
        kw = dict(action=int(g.action[t]), magnitude=float(g.magnitude[t]), power_setpoint=sp, noise_z=float(g.noise_z[t]))
        ox = X.step(**kw)[0].cpu().numpy()
        oy = Y.step(**kw)[0].cpu().numpy()
        rec = X.maintenance_log_records()
        done = rec[rec["kind"] == 1]
        assert np.all(done["action"] == top_off), "a completion of X that is not an oil top-off: %s" % done
        for k in sorted(set(done["pump"][done["plant"] == 0].tolist())):
            assert np.array_equal(np.sort(done["plant"][done["pump"] == k]), np.arange(n))       # every lane runs the same plant
            ok = Y.perform_maintenance("oil_top_off", int(k), target_level=target)
            assert bool(ok.all().item())
            completions += 1
        (fx, ix), (fy, iy) = host_state(X), host_state(Y)
        assert np.array_equal(ix[isel], iy[isel]), "step %d: integer members differ" % t
        a, b = fx[fsel], fy[fsel]
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(a == b, 0.0, np.abs(a - b) / np.maximum(np.abs(a), np.abs(b)))
        worst = max(worst, float(np.nanmax(rel)))
        np.testing.assert_allclose(b, a, rtol=1e-12, atol=1e-300, equal_nan=True, err_msg="step %d" % t)
        np.testing.assert_allclose(oy, ox, rtol=1e-12, atol=1e-300, err_msg="obs step %d" % t)
    print("automatic = operator (%s): %d top-offs, worst relative difference %.3e" % (storage, completions, worst))
    assert completions == 3, completions
    X.close(); Y.close()


# ---------------------------------------------------------------------------------------------------------------- 3. nothing ordered
def _scrambled_pumps(env, seed):
    """heterogeneous pump sections: wear, oil state, leakage, vibration, additives of every pump of every plant"""
    rng = np.random.default_rng(seed)
    n = env.n
    for k in range(4):
        for name, lo, hi in (("pump.oil_level", 40.0, 100.0), ("pump.oil_contamination", 5.0, 18.0), ("pump.oil_acidity", 0.5, 2.0),
                             ("pump.oil_moisture", 0.02, 0.1), ("pump.wear_impeller", 0.0, 9.0), ("pump.wear_motor_bearings", 0.0, 9.0),
                             ("pump.wear_pump_bearings", 0.0, 9.0), ("pump.wear_thrust_bearing", 0.0, 6.0), ("pump.wear_mechanical_seals", 0.0, 17.0),
                             ("pump.wear_coupling_system", 0.0, 4.0), ("pump.seal_leakage_rate", 0.0, 0.2), ("pump.vibration_increase", 0.0, 2.0),
                             ("pump.antioxidant_level", 5.0, 100.0), ("pump.anti_wear_level", 5.0, 100.0), ("pump.corrosion_inhibitor_level", 5.0, 100.0)):
            env.set_field(name, rng.uniform(lo, hi, n), instance=k)


def _bits(env):
    import torch
    f, i = env.state_arrays()
    return f.view(torch.int64), i


@pytest.mark.parametrize("n", [50000, 100])
@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_nothing_ordered_changes_nothing(storage, n):
    """action -1, an action the dispatcher has no handler for, one outside the catalog, a pump that does not exist, a bearing that does
    not exist: the whole arena keeps its bits (50 000 plants: a segmented arena) and success is 0 everywhere"""
    import torch
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv(n, dt=5.0, storage=storage)
    assert (env.L.npb_state_arena_segment(env._h) > 0) == (n == 50000)
    _scrambled_pumps(env, 7)
    for t in range(3):
        env.step()
    f0, i0 = _bits(env)
    rng = np.random.default_rng(1)
    pumps = torch.as_tensor(rng.integers(0, 4, n).astype(np.int32), device=env.device)
    A = _lib.MAINT_ACTIONS
    cases = [(-1, pumps, None), ("npsh_analysis", pumps, None), (A.index("routine_maintenance"), 2, None), (len(A), pumps, None), (1000, 0, None),
             ("oil_change", 4, None), ("oil_change", -1, None), ("component_overhaul", np.full(n, 7, dtype=np.int32), None),
             ("bearing_replacement", pumps, 4), ("bearing_replacement", 1, -1)]
    for action, pump, bearing in cases:
        ok = env.perform_maintenance(action, pump, bearing=bearing)
        assert not bool(ok.any().item()), (action, bearing)
        f1, i1 = _bits(env)
        assert torch.equal(f0, f1) and torch.equal(i0, i1), (action, bearing)
    # and an order that does act is seen by the same comparison
    ok = env.perform_maintenance("oil_change", pumps)
    assert bool(ok.all().item())
    f1, i1 = _bits(env)
    assert not torch.equal(f0, f1)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4. layout independence
@pytest.mark.parametrize("segment", [None, "0"])
def test_orders_do_not_depend_on_the_arena_layout(monkeypatch, segment):
    """50 000 plants (a segmented arena; with NPB_ARENA_SEGMENT=0, read at npb_create, one block), orders for a pseudo-random 3 % of
    them -- mixed pumps, actions, bearings and targets within a wave -- against the same plants gathered into a small one-block handle
    given the same orders: every column of the ordered plants bit for bit, every other plant untouched"""
    import torch
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    if segment is None:
        monkeypatch.delenv("NPB_ARENA_SEGMENT", raising=False)
    else:
        monkeypatch.setenv("NPB_ARENA_SEGMENT", segment)
    n = 50000
    big = BatchedPlantEnv(n, dt=5.0)
    assert (big.L.npb_state_arena_segment(big._h) > 0) == (segment is None)
    _scrambled_pumps(big, 11)
    for t in range(2):
        big.step()
    rng = np.random.default_rng(2025)
    chosen = np.sort(rng.choice(n, size=n * 3 // 100, replace=False))
    m = len(chosen)
    action = rng.integers(0, len(_lib.MAINT_ACTIONS), m).astype(np.int32)
    pump = rng.integers(0, 4, m).astype(np.int32)
    bearing = rng.integers(0, 4, m).astype(np.int32)
    target = rng.uniform(60.0, 110.0, m)
    f0, i0 = big.state_arrays()
    monkeypatch.delenv("NPB_ARENA_SEGMENT", raising=False)
    small = BatchedPlantEnv(m, dt=5.0)
    assert small.L.npb_state_arena_segment(small._h) == 0
    idx = torch.as_tensor(chosen, device=big.device)
    small.load_state_arrays(f0[:, idx].contiguous(), i0[:, idx].contiguous())
    ok_small = small.perform_maintenance(action, pump, bearing=bearing, target_level=target).clone()
    A = np.full(n, -1, dtype=np.int32); A[chosen] = action
    K = np.zeros(n, dtype=np.int32); K[chosen] = pump
    B = np.zeros(n, dtype=np.int32); B[chosen] = bearing
    T = np.full(n, 95.0); T[chosen] = target
    ok_big = big.perform_maintenance(A, K, bearing=B, target_level=T)
    handlers = np.array([int(big.L.npb_maint_action_has_handler(int(a))) for a in action], dtype=np.uint8)
    assert np.array_equal(ok_small.cpu().numpy(), handlers) and handlers.sum() > m // 2 and handlers.sum() < m
    assert torch.equal(ok_big[idx], ok_small) and int(ok_big.sum().item()) == int(handlers.sum())
    f1, i1 = big.state_arrays()
    fs, is_ = small.state_arrays()
    assert torch.equal(f1[:, idx].contiguous().view(torch.int64), fs.view(torch.int64)) and torch.equal(i1[:, idx].contiguous(), is_)
    rest = torch.ones(n, dtype=torch.bool, device=big.device); rest[idx] = False
    assert torch.equal(f1[:, rest].contiguous().view(torch.int64), f0[:, rest].contiguous().view(torch.int64)) and torch.equal(i1[:, rest], i0[:, rest])
    changed = (f1[:, idx] != f0[:, idx]).any(dim=0).cpu().numpy()
    assert changed.sum() > m // 3 and not changed[handlers == 0].any()
    big.close(); small.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the event log
def test_log_reports_the_operator_calls_beside_the_automatic_events():
    """om2 with the log on: the operator records are exactly the fixture's successful calls, the created / completed records exactly
    the events the fixture's per-step reference state implies, info["maintenance_event_count"] the reference's
    maintenance_actions_performed at every step (the operator's calls move none of it)"""
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.maintlog import sort_events
    name = "om2_with_automatic_maintenance"
    n = 64
    env, g, counts = _replay(name, 0, n=n, log=8192)
    rec = env.maintenance_log_records()
    dt = float(g.meta["dt"])
    labels = [c[2] for c in g.cols]
    performed = g.state[:, labels.index("maint.maintenance_actions_performed")]
    assert counts == [int(v) for v in performed[1:]], (counts, performed)
    want_ops = [(o.step * dt, o.pump, o.action, o.bearing if o.action == BEARING_REPLACEMENT else 0) for o in g.ops if o.success]
    assert want_ops
    ops = rec[rec["kind"] == OPERATOR]
    for lane in range(n):
        r = ops[ops["plant"] == lane]
        got = sorted(zip(r["time"].tolist(), r["pump"].tolist(), r["action"].tolist(), r["bearing"].tolist()))
        assert got == sorted(want_ops), (lane, got)
        assert np.all(r["order"] == 0) and np.array_equal(r["created"], r["time"]) and np.array_equal(r["planned_start"], r["time"])
        assert np.all(r["trigger"] == 0) and np.all(r["priority"] == 0)
    auto = rec[rec["kind"] != OPERATOR]
    ev = events_from_golden(g, _lib.MAINT_PARAMS)
    assert len(ev) > 0
    fields = ("time", "created", "planned_start", "plant", "order", "trigger", "pump", "action", "kind", "priority", "bearing")
    for lane in (0, n - 1):
        want = ev.copy(); want["plant"] = lane
        a, b = sort_events(auto[auto["plant"] == lane]), sort_events(want)
        assert len(a) == len(b), (lane, a, b)
        for f in fields:
            assert np.array_equal(a[f], b[f]), (lane, f, a[f], b[f])
    env.close()


def test_formatted_log_names_the_operators_bearing_replacement():
    """a masked bearing replacement on three plants of a ragged batch, through the formatter (env.maintenance_log); an order without a
    handler leaves no record"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 130
    env = BatchedPlantEnv(n, dt=5.0, maintenance=True)
    env.enable_maintenance_log(1024)
    env.step()
    mask = np.zeros(n, dtype=np.uint8); mask[[0, 64, 129]] = 1
    env.perform_maintenance("bearing_replacement", "FWP-3", mask=mask, bearing="thrust_bearing")
    env.perform_maintenance("cavitation_analysis", 1)           # no handler: no record
    cols = env.maintenance_log()
    sel = cols["event_type"] == "operator_maintenance"
    assert list(cols["plant"][sel]) == [0, 64, 129] and list(cols["component_id"][sel]) == ["FWP-3"] * 3
    assert list(cols["bearing"][sel]) == ["thrust"] * 3 and list(cols["action_type"][sel]) == ["bearing_replacement"] * 3
    assert list(cols["timestamp_minutes"][sel]) == [5.0] * 3
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 6. episodes
def test_autoreset_takes_the_operators_work_with_the_episode():
    """autoreset with a time limit of 6 steps: an oil change ordered in the first episode is gone after the restore (the state equals
    the snapshot's, bit for bit), and calls issued in the same loop as the stepping, with no synchronisation in between, act on the
    state the autoreset left"""
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    n, K = 200, 6
    env = BatchedPlantEnv(n, dt=5.0)
    for k in range(4):
        env.set_field("pump.oil_level", np.full(n, 70.0), instance=k)
        env.set_field("pump.oil_contamination", np.full(n, 12.0), instance=k)
    env.snapshot()
    env._enable_autoreset(K)
    f0, i0 = _bits(env)
    odd = torch.zeros(n, dtype=torch.uint8, device=env.device); odd[1::2] = 1
    for t in range(K):
        obs, rew, done, info = env.step()
        if t == 2:
            ok = env.perform_maintenance("oil_change", 1, mask=odd)
            assert torch.equal(ok, odd)
            level = env.get_field("pump.oil_level", instance=1)
            assert bool((level[1::2] == 100.0).all().item()) and bool((level[0::2] < 71.0).all().item())
    assert bool(info["truncated"].all().item())
    f1, i1 = _bits(env)
    assert torch.equal(f0, f1) and torch.equal(i0, i1), "the restored state is not the snapshot's"
    # a policy loop: step, order, step, order ... across the next restore, nothing read back in between
    for t in range(K):
        env.step()
        env.perform_maintenance("oil_top_off", 1, mask=odd, target_level=90.0)
    level = env.get_field("pump.oil_level", instance=1).cpu().numpy()
    assert np.all(level[1::2] == 90.0), level[:4]          # ordered after the restoring step, on the snapshot's 70 %
    assert np.all(level[0::2] == 70.0), level[:4]
    f2, i2 = _bits(env)
    assert not torch.equal(f0, f2)
    env.close()


def test_missing_columns_are_refused_with_a_message():
    import ctypes
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv(64)
    col = torch.zeros(64, dtype=torch.int32, device=env.device)
    assert env.L.npb_perform_maintenance(env._h, None, ctypes.c_void_p(col.data_ptr()), None, None, None, None) == -1
    assert b"npb_perform_maintenance" in env.L.npb_last_error(env._h)
    assert env.L.npb_perform_maintenance(env._h, ctypes.c_void_p(col.data_ptr()), None, None, None, None, None) == -1
    # success may be NULL: the order (oil_change on FWP-1 everywhere) is carried out all the same
    env.set_field("pump.oil_level", np.full(64, 50.0), instance=0)
    assert env.L.npb_perform_maintenance(env._h, ctypes.c_void_p(col.data_ptr()), ctypes.c_void_p(col.data_ptr()), None, None, None, env._stream()) == 0
    assert bool((env.get_field("pump.oil_level", instance=0) == 100.0).all().item())
    env.close()


# ---------------------------------------------------------------------------------------------------------------- the single-plant facade
def test_facade_answers_the_references_call_paths():
    from nuclear_sim_amd.env import ConstantHeatSource, NuclearPlantSimulator
    sim = NuclearPlantSimulator(dt=5.0, heat_source=ConstantHeatSource(), enable_state_management=False)
    pumps = sim.secondary_physics.feedwater_system.pump_system.pumps
    pumps["FWP-2"].lubrication_system.oil_level = 60.0
    assert pumps["FWP-2"].perform_maintenance("oil_top_off") == {"success": True}
    assert pumps["FWP-2"].lubrication_system.oil_level == 95.0
    assert pumps["FWP-2"].lubrication_system.perform_maintenance("oil_top_off", target_level=99.0)["success"] is True
    assert pumps["FWP-2"].lubrication_system.oil_level == 99.0
    pumps["FWP-4"].lubrication_system.component_wear["thrust_bearing"] = 4.0
    pumps["FWP-4"].lubrication_system.component_wear["motor_bearings"] = 3.0
    assert pumps["FWP-4"].lubrication_system.perform_maintenance("bearing_replacement", component_id="thrust_bearing")["success"] is True
    assert pumps["FWP-4"].lubrication_system.component_wear["thrust_bearing"] == 0.0
    assert pumps["FWP-4"].lubrication_system.component_wear["motor_bearings"] == 3.0
    assert pumps["FWP-4"].perform_maintenance("bearing_replacement", component_id="wheel_bearing")["success"] is False
    assert pumps["FWP-1"].perform_maintenance("npsh_analysis")["success"] is False
    assert pumps["FWP-1"].perform_maintenance("general")["success"] is False
    with pytest.raises(AttributeError):       # the other components' maintenance is not on the device
        sim.secondary_physics.turbine.perform_maintenance
    with pytest.raises(AttributeError):
        sim.secondary_physics.feedwater_system.pump_system.perform_maintenance
    sim.step()
