"""GPU: operator-ordered maintenance of the turbine (npb_perform_turbine_maintenance, BatchedPlantEnv.perform_turbine_maintenance).  The
handlers a caller orders between two steps do to the plant what the reference's perform_maintenance of the turbine, a bearing, the
bearing-lubrication system and a stage does (fixtures tests/golden/operator_turbine/, every step kernel, full and ragged batches, both
storage types); nothing ordered changes nothing; an order moves only turb, or the stage's three columns; the result does not depend on
the arena's layout; the modes that do not step the turbine refuse every order; the event log reports the orders; an autoreset takes the
work away with the episode.

Tolerances: those of tests/test_component_maintenance_gpu.py -- the parity contract's RTOL with the absolute floor on reals (the members
the arena keeps as float included), integer members and success exact; fp32 storage at the project's 1e-4 on observations.  The
per-lane comparison at 1e-12 from exactly loaded inputs is tests/test_scattered_turbine_calls_gpu.py."""
import ctypes

import numpy as np
import pytest

from golden_util import ATOL_SMALL, RTOL, compare_state
from turbine_maintenance_golden import ACTIONS, REPLAYED, UNITS, TurbineGolden, order_succeeds
from work_order_events import host_state, make_env

pytestmark = pytest.mark.gpu

KERNEL_OF_VARIANT = {0: "npb_step4_kernel", 1: "npb_step_kernel", 2: "npb_step2_wide_kernel", 3: "npb_step2_kernel", 4: "npb_step_nt_kernel",
                     5: "npb_step4_kernel"}
OPERATOR_TURBINE = 4
BEARING_IDS = ("TB-001", "TB-002", "TB-003", "TB-004")
STAGE_IDS = tuple(["HP-%d" % k for k in range(1, 9)] + ["LP-%d" % k for k in range(1, 7)])
_GOLDENS = {}


def golden(name):
    """loaded once, shared, never written to"""
    if name not in _GOLDENS:
        _GOLDENS[name] = TurbineGolden(name)
    return _GOLDENS[name]


def _start(g, n, storage="f64", **kw):
    env = make_env(g, n=n, storage=storage, **kw)
    f0, i0 = host_state(env)
    f, i, fm, im = g.split_state(g.state[0])
    f0[fm, :] = f[fm, None]; i0[im, :] = i[im, None]
    env.load_state_arrays(f0, i0)
    return env


def _order(env, g, j, o, mask=None):
    """the fixture's call j through the Python surface, spelt differently from call to call (name / index, number / id)"""
    kind, name = g.kind_name(o)
    if kind is None:                   # a type outside the catalog: only an index can say so (a name is refused on the host)
        return env.perform_turbine_maintenance(o.called, len(ACTIONS), unit=o.unit, mask=mask)
    unit = o.unit if UNITS[kind] > 1 else (None if j % 2 else 0)
    if j % 3 == 0 and 0 <= o.unit < UNITS[kind] and UNITS[kind] > 1:
        unit = (BEARING_IDS if kind == "bearing" else STAGE_IDS)[o.unit]
    return env.perform_turbine_maintenance(kind, name if j % 2 == 0 else o.action, unit=unit, mask=mask)


def _poke(env, g, t, n):
    import torch
    from nuclear_sim_amd import _lib
    for label, v in g.pokes.get(t, []):
        kind, slot = g.label_slot(label)
        col = torch.full((n,), v, dtype=torch.float64 if kind == "f64" else torch.int32, device=env.device)
        _lib.check(env.L.npb_set_field(env._h, 0 if kind == "f64" else 1, slot, ctypes.c_void_p(col.data_ptr()), 1, env._stream()), env._h)


def _step(env, g, t):
    sp = None if np.isnan(g.setpoint[t]) else g.setpoint[t]
    cw = None if np.isnan(g.cooling[t]) else g.cooling[t]
    return env.step(action=int(g.action[t]), magnitude=float(g.magnitude[t]), power_setpoint=sp, cooling_water_temp=cw, noise_z=float(g.noise_z[t]))


def _compare_sections(g, env, want, lanes, where):
    """turb and tstg against a fixture row: reals within RTOL with the absolute floor, integer members exact"""
    fs, is_ = host_state(env)
    bad = []
    for (kind, slot), m, v in zip(g.op_slots, g.op_labels, want):
        if np.isnan(v):
            continue
        for lane in lanes:
            if kind == "i32":
                if int(is_[slot, lane]) != int(v):
                    bad.append((m, lane, int(is_[slot, lane]), int(v)))
            elif not (abs(float(fs[slot, lane]) - v) <= RTOL * abs(v) + ATOL_SMALL):
                bad.append((m, lane, float(fs[slot, lane]), float(v)))
    assert not bad, "%s %s: %d mismatching members, first: %s" % (g.name, where, len(bad), bad[:5])


def _replay(name, variant, storage="f64", n=64, ordered=None, log=None):
    """the fixture on n lanes with its pokes and operator calls; ordered = the lanes that receive the calls (None = all).  Checks (lanes =
    the first and the last ordered one): success of every call, turb and tstg after every call, obs / reward / done at every step, every
    schema column at every recorded step."""
    import torch
    g = golden(name)
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
    want_kernel = KERNEL_OF_VARIANT[variant].replace("_kernel", "_maint_kernel") if env.params.maint_enabled else KERNEL_OF_VARIANT[variant]
    for t in range(g.T):
        _poke(env, g, t, n)
        for j, o in g.ops_at(t):
            ok = _order(env, g, j, o, mask).cpu().numpy()
            want = np.zeros(n, dtype=np.uint8); want[lanes] = int(o.success)
            assert np.array_equal(ok, want), "%s call %d %r: success %s" % (name, j, o, ok[:8])
            if storage == "f64":
                _compare_sections(g, env, g.op_after[j], probe, "after call %d %r (variant %d)" % (j, o, variant))
        obs, rew, done, info = _step(env, g, t)
        assert env.last_step_kernel() == want_kernel, env.last_step_kernel()
        obs = obs.cpu().numpy(); rew = rew.cpu().numpy(); done = done.cpu().numpy()
        for lane in probe:
            if storage == "f64":
                np.testing.assert_allclose(obs[lane], g.obs[t], rtol=RTOL, atol=1e-12, err_msg="%s obs step %d lane %d" % (name, t, lane))
                np.testing.assert_allclose(rew[lane], g.reward[t], rtol=RTOL, atol=1e-9, err_msg="%s reward step %d" % (name, t))
            else:
                np.testing.assert_allclose(obs[lane], g.obs[t], rtol=1e-4, atol=1e-7, err_msg="%s fp32 obs step %d lane %d" % (name, t, lane))
            assert int(done[lane]) == int(g.done[t]), "%s done step %d" % (name, t)
        if storage == "f64" and t + 1 in sampled:
            fs, is_ = host_state(env)
            for lane in probe:
                compare_state(g, fs[:, lane], is_[:, lane], g.state[sampled[t + 1]], "after step %d (lane %d, variant %d)" % (t, lane, variant))
    return env, g


def _plain(g, n, storage="f64"):
    """the fixture's run with its pokes and without its calls"""
    env = _start(g, n, storage)
    for t in range(g.T):
        _poke(env, g, t, n)
        _step(env, g, t)
    return env


def _bits(env):
    import torch
    f, i = env.state_arrays()
    return f.view(torch.int64) if f.dtype == torch.float64 else f.view(torch.int32), i


# ---------------------------------------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", REPLAYED)
def test_turbine_calls_replay_the_reference_on_every_step_kernel(name, variant):
    """64 copies of the fixture's plant; the kernel is the same for every variant, the state it hands on is read by each step kernel"""
    env, g = _replay(name, variant)
    assert sum(o.success for o in g.ops) >= 5
    env.close()


@pytest.mark.parametrize("name", ["ot1_degraded_turbine", "ot2_stages"])
def test_ragged_batch_a_subset_of_lanes_ordered(name):
    """130 lanes (two full waves and a ragged one), the calls masked to every third lane: those follow the reference, the others are a
    run without any call, bit for bit"""
    import torch
    n = 130
    some = np.arange(2, n, 3)
    rest = np.setdiff1d(np.arange(n), some)
    env, g = _replay(name, 0, n=n, ordered=some)
    (fa, ia), plain = _bits(env), _plain(g, n)
    fb, ib = _bits(plain)
    assert torch.equal(fa[:, rest], fb[:, rest]) and torch.equal(ia[:, rest], ib[:, rest])
    assert not torch.equal(fa[:, some], fb[:, some])
    env.close(); plain.close()


@pytest.mark.parametrize("name", ["ot1_degraded_turbine", "ot2_stages"])
def test_fp32_storage_follows_the_calls(name):
    """fp32 storage has no reference trajectory (values rounded to float once per store): success is the reference's, the ordered
    plants' observations stay within the fp32 mode's 1e-4 of the fixture, an unordered lane equals a run without calls bit for bit"""
    import torch
    n = 130
    some = np.arange(1, n, 2)
    env, g = _replay(name, 0, storage="f32", n=n, ordered=some)
    (fa, ia), plain = _bits(env), _plain(g, n, "f32")
    fb, ib = _bits(plain)
    assert torch.equal(fa[:, 0::2], fb[:, 0::2]) and torch.equal(ia[:, 0::2], ib[:, 0::2])
    assert not torch.equal(fa[:, 1::2], fb[:, 1::2])
    env.close(); plain.close()


# ---------------------------------------------------------------------------------------------------------------- 2. nothing ordered; only what is touched
def _scrambled(env, seed):
    """heterogeneous bearings, oil and stages; a latched trip on some plants"""
    rng = np.random.default_rng(seed)
    n = env.n
    for k in range(4):
        env.set_field("turb.bearing_wear_factor", rng.uniform(0.7, 1.0, n), k=k)
        env.set_field("turb.bearing_metal_temp", rng.uniform(75.0, 110.0, n), k=k)
    for name, lo, hi in (("turb.lub_oil_temperature", 40.0, 70.0), ("turb.lub_oil_contamination", 0.5, 15.0), ("turb.lub_oil_moisture", 0.01, 0.08),
                         ("turb.lub_oil_acidity", 0.02, 0.6), ("turb.lub_effectiveness", 0.4, 1.0), ("turb.thermal_bow", 0.0, 0.05)):
        env.set_field(name, rng.uniform(lo, hi, n))
    for k in range(5):
        env.set_field("turb.lub_wear", rng.uniform(0.0, 25.0, n), k=k)
    for k in range(14):
        env.set_field("tstg.stage_deposit_thickness", rng.uniform(0.0, 0.4, n), k=k)
        env.set_field("tstg.stage_blade_wear_factor", rng.uniform(0.8, 1.0, n), k=k)
        env.set_field("tstg.stage_efficiency_degradation", rng.uniform(0.0, 0.05, n), k=k)
    env.set_field("turb.trip_active", rng.integers(0, 2, n).astype(np.int32))
    env.set_field("turb.trip_latched_mask", rng.integers(1, 64, n).astype(np.int32))
    env.set_field("turb.timer_vibration", rng.uniform(0.0, 600.0, n))


@pytest.mark.parametrize("n", [50000, 64])
@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_nothing_ordered_changes_nothing(storage, n):
    """every action -1, a zero mask, an index outside the catalog, a unit that does not exist, the thrust adjustment of a journal bearing:
    no byte of the arena changes (50 000 plants: a segmented arena) and success is 0 everywhere; an order that does act is seen by the
    same comparison"""
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv(n, dt=5.0, storage=storage)
    assert (env.L.npb_state_arena_segment(env._h) > 0) == (n == 50000)
    env.step()
    _scrambled(env, 7)
    f0, i0 = _bits(env)
    rng = np.random.default_rng(1)
    units = torch.as_tensor(rng.integers(0, 14, n).astype(np.int32), device=env.device)
    journal = torch.as_tensor(rng.choice([0, 1, 3], n).astype(np.int32), device=env.device)
    zero = torch.zeros(n, dtype=torch.uint8, device=env.device)
    everything = rng.integers(0, len(ACTIONS), n).astype(np.int32)
    cases = [("stage", -1, units, None), ("turbine", np.full(n, -1, dtype=np.int32), None, None),
             ("stage", "overhaul", units, zero), ("bearing", everything, units % 4, zero),
             ("lubrication", len(ACTIONS), units, None), ("turbine", 1000, 0, None),
             ("stage", "overhaul", 14, None), ("stage", "blade_replacement", -1, None),
             ("bearing", "turbine_bearing_replacement", 4, None), ("bearing", "routine_maintenance", np.full(n, 77, dtype=np.int32), None),
             ("bearing", "thrust_bearing_adjustment", journal, None)]
    for component, action, unit, mask in cases:
        ok = env.perform_turbine_maintenance(component, action, unit=unit, mask=mask)
        assert not bool(ok.any().item()), (component, action)
        f1, i1 = _bits(env)
        assert torch.equal(f0, f1) and torch.equal(i0, i1), (component, action)
    ok = env.perform_turbine_maintenance("stage", "overhaul", unit=units)
    assert bool(ok.all().item())
    assert not torch.equal(f0, _bits(env)[0])
    env.close()


def test_one_block_arena_gives_the_segmented_arenas_result(monkeypatch):
    """50 000 plants with NPB_ARENA_SEGMENT=0 (read at npb_create: one block) and as a segmented arena, orders for a pseudo-random 3 % of
    them -- mixed kinds, actions and units within a wave -- against the same plants gathered into a small one-block handle given the same
    orders: every column of the ordered plants bit for bit, every other plant untouched"""
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 50000
    rng = np.random.default_rng(2025)
    chosen = np.sort(rng.choice(n, size=n * 3 // 100, replace=False))
    m = len(chosen)
    action = rng.integers(0, len(ACTIONS) + 2, m).astype(np.int32)
    unit = rng.integers(0, 15, m).astype(np.int32)
    want = np.array([int(a < len(ACTIONS) and (UNITS[ACTIONS[a][0]] == 1 or order_succeeds(ACTIONS[a][0], ACTIONS[a][1], u))) for a, u in zip(action, unit)],
                    dtype=np.uint8)
    assert m // 4 < want.sum() < m
    A = np.full(n, -1, dtype=np.int32); A[chosen] = action
    U = np.zeros(n, dtype=np.int32); U[chosen] = unit
    results = []
    for segment in (None, "0"):
        if segment is None:
            monkeypatch.delenv("NPB_ARENA_SEGMENT", raising=False)
        else:
            monkeypatch.setenv("NPB_ARENA_SEGMENT", segment)
        big = BatchedPlantEnv(n, dt=5.0)
        assert (big.L.npb_state_arena_segment(big._h) > 0) == (segment is None)
        big.step()
        _scrambled(big, 11)
        f0, i0 = big.state_arrays()
        monkeypatch.delenv("NPB_ARENA_SEGMENT", raising=False)
        small = BatchedPlantEnv(m, dt=5.0)
        assert small.L.npb_state_arena_segment(small._h) == 0
        idx = torch.as_tensor(chosen, device=big.device)
        small.load_state_arrays(f0[:, idx].contiguous(), i0[:, idx].contiguous())
        ok_small = small.perform_turbine_maintenance("turbine", action, unit=unit).clone()
        ok_big = big.perform_turbine_maintenance("turbine", A, unit=U)
        assert np.array_equal(ok_small.cpu().numpy(), want)
        assert torch.equal(ok_big[idx], ok_small) and int(ok_big.sum().item()) == int(want.sum())
        f1, i1 = big.state_arrays()
        fs, is_ = small.state_arrays()
        assert torch.equal(f1[:, idx].contiguous().view(torch.int64), fs.view(torch.int64)) and torch.equal(i1[:, idx].contiguous(), is_)
        rest = torch.ones(n, dtype=torch.bool, device=big.device); rest[idx] = False
        assert torch.equal(f1[:, rest].contiguous().view(torch.int64), f0[:, rest].contiguous().view(torch.int64)) and torch.equal(i1[:, rest], i0[:, rest])
        changed = ((f1[:, idx] != f0[:, idx]).any(dim=0) | (i1[:, idx] != i0[:, idx]).any(dim=0)).cpu().numpy()
        assert changed.sum() > m // 4 and not changed[want == 0].any()
        results.append(f1.view(torch.int64).clone())
        big.close(); small.close()
    assert torch.equal(results[0], results[1]), "the two layouts disagree"


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_an_order_moves_only_turb_or_the_stages_three_columns(storage):
    """every catalogued action in turn, ordered for every third plant of a ragged batch of 130 with mixed units: the unordered plants keep
    their bits, and so does every column of an ordered plant outside turb (the turbine, a bearing, the lubrication system: the bearing's
    own members for a bearing) or outside the ordered stage's three columns"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    from nuclear_sim_amd.schema import SCHEMA
    n = 130
    env = BatchedPlantEnv(n, dt=5.0, storage=storage)
    env.step()
    cols = SCHEMA.columns()
    flabel = [lab for k, _s, lab, _p in cols if k == "f64"]; ilabel = [lab for k, _s, lab, _p in cols if k == "i32"]
    some = np.arange(2, n, 3)
    rest = np.setdiff1d(np.arange(n), some)
    mask = np.zeros(n, dtype=np.uint8); mask[some] = 1
    rng = np.random.default_rng(5)
    same = lambda x, y: (x == y) | (np.isnan(x) & np.isnan(y))
    acted = 0
    for a, (kind, name) in enumerate(ACTIONS):
        _scrambled(env, 100 + a)
        unit = rng.integers(0, UNITS[kind], n).astype(np.int32)
        fb, ib = host_state(env)
        ok = env.perform_turbine_maintenance(kind, name, unit=unit, mask=mask).cpu().numpy()
        want = mask * np.array([order_succeeds(kind, name, u) for u in unit], dtype=np.uint8)
        assert np.array_equal(ok, want), (kind, name)
        fa, ia = host_state(env)
        assert same(fb[:, rest], fa[:, rest]).all() and np.array_equal(ib[:, rest], ia[:, rest]), (kind, name)
        moved = [(flabel[r], lane) for r, lane in zip(*np.nonzero(~same(fb, fa)))] + [(ilabel[r], lane) for r, lane in zip(*np.nonzero(ib != ia))]
        for label, lane in moved:
            assert want[lane], (kind, name, lane, label)
            allowed = {"turbine": ("turb.",), "lubrication": ("turb.lub_",),
                       "bearing": ("turb.bearing_metal_temp[%d]" % unit[lane], "turb.bearing_wear_factor[%d]" % unit[lane]),
                       "stage": tuple("tstg.stage_%s[%d]" % (m, unit[lane]) for m in ("deposit_thickness", "blade_wear_factor", "efficiency_degradation"))}[kind]
            assert label.startswith(allowed), (kind, name, lane, label)
        acted += int(bool(moved))
    assert acted >= 14, acted
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3. modes, arguments
def test_modes_that_do_not_step_the_turbine_do_not_service_it():
    """primary only: the reference then has no secondary_physics to call; primary + steam generators: no turbine is stepped -- success 0
    for every kind, nothing stored"""
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 70
    for mode in ("primary", "primary_sg"):
        env = BatchedPlantEnv(n, dt=5.0, mode=mode)
        env.step()
        for kind, name in (("turbine", "routine_maintenance"), ("bearing", "turbine_bearing_replacement"), ("lubrication", "turbine_oil_change"),
                           ("stage", "overhaul")):
            f0, i0 = _bits(env)
            ok = env.perform_turbine_maintenance(kind, name, unit=1)
            assert not bool(ok.any().item()), (mode, kind)
            f1, i1 = _bits(env)
            assert torch.equal(f0, f1) and torch.equal(i0, i1), (mode, kind)
        env.close()


def test_missing_action_column_is_refused_and_the_optional_ones_may_be_null():
    from nuclear_sim_amd import _lib
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv(64, dt=5.0)
    assert env.L.npb_perform_turbine_maintenance(env._h, None, None, None, None) == -1
    assert b"npb_perform_turbine_maintenance" in env.L.npb_last_error(env._h)
    env.set_field("turb.thermal_bow", np.full(64, 0.1))
    env.set_field("tstg.stage_deposit_thickness", np.full(64, 0.2), k=0)
    env.set_field("tstg.stage_deposit_thickness", np.full(64, 0.2), k=1)
    a = torch.full((64,), _lib.turbine_action_index("turbine", "vibration_analysis"), dtype=torch.int32, device=env.device)
    assert env.L.npb_perform_turbine_maintenance(env._h, ctypes.c_void_p(a.data_ptr()), None, None, env._stream()) == 0
    assert bool((env.get_field("turb.thermal_bow") == 0.1 * 0.7).all().item())
    # unit NULL = 0: the first stage
    a.fill_(_lib.turbine_action_index("stage", "overhaul"))
    assert env.L.npb_perform_turbine_maintenance(env._h, ctypes.c_void_p(a.data_ptr()), None, None, env._stream()) == 0
    assert bool((env.get_field("tstg.stage_deposit_thickness", k=0) == 0.0).all().item())
    assert bool((env.get_field("tstg.stage_deposit_thickness", k=1) != 0.0).all().item())
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the event log
def test_log_reports_one_record_per_successful_order():
    """ot4 (the log needs the automatic maintenance on, which this fixture's plant has) with the log on: the kind-4 records are exactly the
    fixture's successful calls -- catalog index, unit, the plant's clock -- for every lane, beside the automatic pump maintenance's own
    created / completed records, which the calls do not disturb"""
    name = "ot4_long_run"
    n = 64
    env, g = _replay(name, 0, n=n, log=8192)
    rec = env.maintenance_log_records()
    dt = float(g.meta["dt"])
    want = sorted((o.step * dt, o.unit if UNITS[ACTIONS[o.action][0]] > 1 else 0, o.action) for o in g.ops if o.success)
    assert len(want) == 6
    ops = rec[rec["kind"] == OPERATOR_TURBINE]
    assert len(ops) == n * len(want)
    for lane in range(n):
        r = ops[ops["plant"] == lane]
        assert sorted(zip(r["time"].tolist(), r["pump"].tolist(), r["action"].tolist())) == want, lane
        assert np.all(r["order"] == 0) and np.array_equal(r["created"], r["time"]) and np.array_equal(r["planned_start"], r["time"])
        assert np.all(r["trigger"] == 0) and np.all(r["priority"] == 0) and np.all(r["bearing"] == 0)
    auto = rec[rec["kind"] != OPERATOR_TURBINE]
    labels = [c[2] for c in g.cols]
    performed = int(g.state[-1, labels.index("maint.maintenance_actions_performed")])
    created = int(g.state[-1, labels.index("maint.work_orders_created")])
    assert performed >= 1 and set(auto["kind"].tolist()) <= {0, 1}
    assert int((auto["kind"] == 1).sum()) == n * performed and int((auto["kind"] == 0).sum()) == n * created
    env.close()


def test_formatted_log_names_the_object_and_action_beside_the_other_operator_orders():
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 130
    env = BatchedPlantEnv(n, dt=5.0, maintenance=True)
    env.enable_maintenance_log(1024)
    env.step()
    mask = np.zeros(n, dtype=np.uint8); mask[[0, 64, 129]] = 1
    env.perform_turbine_maintenance("bearing", "thrust_bearing_adjustment", unit="TB-003", mask=mask)
    env.perform_turbine_maintenance("stage", "overhaul", unit="LP-2", mask=mask)
    env.perform_turbine_maintenance("bearing", "thrust_bearing_adjustment", unit=1)           # a journal bearing: no record
    env.perform_turbine_maintenance("stage", "overhaul", unit=14)                              # no such stage: no record
    env.perform_component_maintenance("steam_generator", "scale_removal", unit=1, mask=mask)
    env.perform_maintenance("oil_change", "FWP-3", mask=mask)
    cols = env.maintenance_log()
    sel = cols["event_type"] == "operator_turbine_maintenance"
    assert list(cols["plant"][sel]) == [0, 0, 64, 64, 129, 129]
    assert list(cols["component_id"][sel]) == ["TB-003", "LP-2"] * 3
    assert list(cols["action_type"][sel]) == ["thrust_bearing_adjustment", "overhaul"] * 3
    assert list(cols["timestamp_minutes"][sel]) == [5.0] * 6 and list(cols["work_order_id"][sel]) == [""] * 6
    # per plant: the pump order, the component order, then the turbine orders
    assert list(cols["event_type"][cols["plant"] == 64]) == ["operator_maintenance", "operator_component_maintenance"] + ["operator_turbine_maintenance"] * 2
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5. episodes
def test_autoreset_and_restore_take_the_operators_work_with_the_episode():
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    n, K = 200, 6
    env = BatchedPlantEnv(n, dt=5.0)
    env.set_field("tstg.stage_deposit_thickness", np.full(n, 0.3), k=9)
    env.set_field("turb.bearing_wear_factor", np.full(n, 0.8), k=1)
    env.snapshot()
    env._enable_autoreset(K)
    f0, i0 = _bits(env)
    odd = torch.zeros(n, dtype=torch.uint8, device=env.device); odd[1::2] = 1
    for t in range(K):
        obs, rew, done, info = env.step()
        if t == 2:
            assert torch.equal(env.perform_turbine_maintenance("stage", "overhaul", unit=9, mask=odd), odd)
            assert torch.equal(env.perform_turbine_maintenance("bearing", "turbine_bearing_replacement", unit=1, mask=odd), odd)
            dep = env.get_field("tstg.stage_deposit_thickness", k=9)
            assert bool((dep[1::2] == 0.0).all().item()) and bool((dep[0::2] > 0.29).all().item())
    assert bool(info["truncated"].all().item())
    f1, i1 = _bits(env)
    assert torch.equal(f0, f1) and torch.equal(i0, i1), "the restored state is not the snapshot's"
    env.step()
    env.perform_turbine_maintenance("bearing", "turbine_bearing_replacement", unit=1, mask=odd)
    wear = env.get_field("turb.bearing_wear_factor", k=1).cpu().numpy()
    assert np.all(wear[1::2] == 1.0) and np.all(wear[0::2] < 0.81), wear[:4]
    env.restore()
    f2, i2 = _bits(env)
    assert torch.equal(f0, f2) and torch.equal(i0, i2), "restore() did not take the replacement away"
    env.close()
