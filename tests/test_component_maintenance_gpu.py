"""GPU: operator-ordered maintenance of steam generators and condenser (npb_perform_component_maintenance,
BatchedPlantEnv.perform_component_maintenance).  The handlers a caller orders between two steps do to the plant what the reference's
perform_maintenance of a steam generator, the steam-generator system, the condenser and a steam-jet ejector does (fixtures
tests/golden/operator_components/, every step kernel, full and ragged batches, both storage types); nothing ordered changes nothing; an
order moves only the sections its action touches; the result does not depend on the arena's layout; the event log reports the orders;
the single-plant facade answers the reference's call paths; an autoreset takes the work away with the episode.

Tolerances: those of tests/test_operator_maintenance_gpu.py -- the parity contract's RTOL with the absolute floor on reals, integer
members exact; fp32 storage at the project's 1e-4 on observations."""
import ctypes

import numpy as np
import pytest

from golden_util import ATOL_SMALL, CANCELLATION_COLUMNS, CANCELLATION_FLOOR, RTOL, compare_state
from component_maintenance_golden import ACTIONS, CLEANING_NAMES, UNITS, ComponentGolden
from work_order_events import host_state, make_env

pytestmark = pytest.mark.gpu

KERNEL_OF_VARIANT = {0: "npb_step4_kernel", 1: "npb_step_kernel", 2: "npb_step2_wide_kernel", 3: "npb_step2_kernel", 4: "npb_step_nt_kernel",
                     5: "npb_step4_kernel"}
OPERATOR_COMPONENT = 3
FIXTURES = ("oc1_steam_generators", "oc2_condenser", "oc3_long_run")
_GOLDENS = {}


def golden(name):
    """loaded once, shared, never written to"""
    if name not in _GOLDENS:
        _GOLDENS[name] = ComponentGolden(name)
    return _GOLDENS[name]


def _start(g, n, storage="f64", **kw):
    env = make_env(g, n=n, storage=storage, **kw)
    f0, i0 = host_state(env)
    f, i, fm, im = g.split_state(g.state[0])
    f0[fm, :] = f[fm, None]; i0[im, :] = i[im, None]
    env.load_state_arrays(f0, i0)
    return env


def _order(env, g, j, o, mask=None):
    """the fixture's call j through the Python surface, spelt differently from call to call (name / index, keyword / enum)"""
    kind, name = g.kind_name(o)
    if kind is None:                   # a type outside the catalog: only an index can say so (a name is refused on the host)
        return env.perform_component_maintenance(o.called, len(ACTIONS), unit=o.unit, mask=mask)
    cleaning = (CLEANING_NAMES[o.cleaning] if j % 2 == 0 else o.cleaning) if o.cleaning else None
    unit = o.unit if UNITS[kind] > 1 else (None if j % 2 else 0)
    if kind == "ejector" and j % 3 == 0:
        unit = ("SJE-001", "SJE-002")[o.unit]
    return env.perform_component_maintenance(kind, name if j % 2 == 0 else o.action, unit=unit, mask=mask, cleaning_type=cleaning)


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
    """the sections a call may touch against a fixture row: reals within RTOL with the absolute floor, integer members exact"""
    fs, is_ = host_state(env)
    bad = []
    for (kind, slot), m, v in zip(g.op_slots, g.op_labels, want):
        if np.isnan(v):
            continue
        for lane in lanes:
            if kind == "i32":
                if int(is_[slot, lane]) != int(v):
                    bad.append((m, lane, int(is_[slot, lane]), int(v)))
            else:
                floor = CANCELLATION_FLOOR if m.endswith(CANCELLATION_COLUMNS) else ATOL_SMALL
                if not (abs(float(fs[slot, lane]) - v) <= RTOL * abs(v) + floor):
                    bad.append((m, lane, float(fs[slot, lane]), float(v)))
    assert not bad, "%s %s: %d mismatching members, first: %s" % (g.name, where, len(bad), bad[:5])


def _replay(name, variant, storage="f64", n=64, ordered=None, log=None):
    """the fixture on n lanes with its pokes and operator calls; ordered = the lanes that receive the calls (None = all).  Checks (lanes =
    the first and the last ordered one): success of every call, the touched sections after every call, obs / reward / done at every
    step, every schema column at every recorded step."""
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
@pytest.mark.parametrize("name", FIXTURES)
def test_component_calls_replay_the_reference_on_every_step_kernel(name, variant):
    """64 copies of the fixture's plant; the kernel is the same for every variant, the state it hands on is read by each step kernel"""
    env, g = _replay(name, variant)
    assert sum(o.success for o in g.ops) >= 5
    env.close()


@pytest.mark.parametrize("name", ["oc1_steam_generators", "oc2_condenser"])
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


@pytest.mark.parametrize("name", ["oc1_steam_generators", "oc2_condenser"])
def test_fp32_storage_follows_the_calls(name):
    """fp32 storage has no reference counterpart (values rounded to float once per store): success is the reference's, the ordered
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
    """heterogeneous generators, condenser and ejectors"""
    rng = np.random.default_rng(seed)
    n = env.n
    for i in range(3):
        for name, lo, hi in (("sg.tsp_magnetite", 0.0, 1.2), ("sg.tsp_copper", 0.0, 0.4), ("sg.tsp_silica", 0.0, 0.5), ("sg.tsp_biological", 0.0, 0.3)):
            for k in range(7):
                env.set_field(name, rng.uniform(lo, hi, n), instance=i, k=k)
        s = rng.uniform(0.0, 2.0, n)
        for name, share in (("sg.scale_thickness", 1.0), ("sg.scale_iron_oxide", 0.6), ("sg.scale_crud", 0.3), ("sg.scale_corrosion", 0.1)):
            env.set_field(name, s * share, instance=i)
    for name, lo, hi in (("cond.biofouling_thickness", 0.0, 1.0), ("cond.scale_thickness", 0.0, 0.8), ("cond.corrosion_product_thickness", 0.0, 0.5),
                         ("cond.time_since_cleaning", 0.0, 6000.0), ("cond.current_air_leakage", 0.05, 0.15)):
        env.set_field(name, rng.uniform(lo, hi, n))
    for k in range(2):
        for name, lo in (("cond.ej_nozzle_fouling", 0.5), ("cond.ej_diffuser_fouling", 0.6), ("cond.ej_nozzle_erosion", 0.7)):
            env.set_field(name, rng.uniform(lo, 1.0, n), instance=0, k=k)


@pytest.mark.parametrize("n", [50000, 130])
@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_nothing_ordered_changes_nothing(storage, n):
    """every action -1, a zero mask, an index outside the catalog, a unit that does not exist: no byte of the arena changes (50 000
    plants: a segmented arena) and success is 0 everywhere; an order that does act is seen by the same comparison"""
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv(n, dt=5.0, storage=storage)
    assert (env.L.npb_state_arena_segment(env._h) > 0) == (n == 50000)
    _scrambled(env, 7)
    for t in range(2):
        env.step()
    f0, i0 = _bits(env)
    rng = np.random.default_rng(1)
    units = torch.as_tensor(rng.integers(0, 3, n).astype(np.int32), device=env.device)
    zero = torch.zeros(n, dtype=torch.uint8, device=env.device)
    everything = rng.integers(0, len(ACTIONS), n).astype(np.int32)
    cases = [("steam_generator", -1, units, None), ("condenser", np.full(n, -1, dtype=np.int32), None, None),
             ("steam_generator", "tsp_chemical_cleaning", units, zero), ("condenser", everything, units % 2, zero),
             ("steam_generator", len(ACTIONS), units, None), ("ejector", 1000, 0, None),
             ("steam_generator", "tsp_chemical_cleaning", 3, None), ("steam_generator", "scale_removal", -1, None),
             ("ejector", "general", 2, None), ("ejector", "vacuum_ejector_cleaning", np.full(n, 7, dtype=np.int32), None)]
    for component, action, unit, mask in cases:
        ok = env.perform_component_maintenance(component, action, unit=unit, mask=mask)
        assert not bool(ok.any().item()), (component, action)
        f1, i1 = _bits(env)
        assert torch.equal(f0, f1) and torch.equal(i0, i1), (component, action)
    ok = env.perform_component_maintenance("steam_generator", "tsp_chemical_cleaning", unit=units)
    assert bool(ok.all().item())
    assert not torch.equal(f0, _bits(env)[0])
    env.close()


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_an_order_moves_only_the_sections_its_action_touches(storage):
    """every catalogued action in turn, ordered for every third plant of a ragged batch of 130 with mixed units: the unordered plants keep
    their bits, and so does every column of an ordered plant outside the sections the action may touch"""
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    from nuclear_sim_amd.schema import SCHEMA
    n = 130
    env = BatchedPlantEnv(n, dt=5.0, storage=storage)
    _scrambled(env, 3)
    env.step()
    cols = SCHEMA.columns()
    some = np.arange(2, n, 3)
    mask = np.zeros(n, dtype=np.uint8); mask[some] = 1
    rng = np.random.default_rng(5)
    acted = 0
    for a, (kind, name) in enumerate(ACTIONS):
        unit = rng.integers(0, UNITS[kind], n).astype(np.int32)
        fb, ib = host_state(env)
        ok = env.perform_component_maintenance(kind, name, unit=unit, mask=mask, cleaning_type="mechanical").cpu().numpy()
        assert np.array_equal(ok, mask), (kind, name)
        fa, ia = host_state(env)
        same = lambda x, y: (x == y) | (np.isnan(x) & np.isnan(y))
        rest = np.setdiff1d(np.arange(n), some)
        assert same(fb[:, rest], fa[:, rest]).all() and np.array_equal(ib[:, rest], ia[:, rest]), (kind, name)
        flabel = [lab for k, _s, lab, _p in cols if k == "f64"]; ilabel = [lab for k, _s, lab, _p in cols if k == "i32"]
        moved = [(flabel[r], lane) for r, lane in zip(*np.nonzero(~same(fb, fa)))] + [(ilabel[r], lane) for r, lane in zip(*np.nonzero(ib != ia))]
        for label, lane in moved:
            allowed = {"steam_generator": ("sg[%d]." % unit[lane],), "steam_generator_system": ("sg[", "sec."),
                       "condenser": ("cond.", "chem[1]."), "ejector": ("cond.ej_",)}[kind]
            assert label.startswith(allowed), (kind, name, lane, label)
        acted += int(not (same(fb, fa).all() and np.array_equal(ib, ia)))
    assert acted >= 15, acted
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3. layout independence
@pytest.mark.parametrize("segment", [None, "0"])
def test_orders_do_not_depend_on_the_arena_layout(monkeypatch, segment):
    """50 000 plants (a segmented arena; with NPB_ARENA_SEGMENT=0, read at npb_create, one block), orders for a pseudo-random 3 % of
    them -- mixed kinds, actions, units and cleaning types within a wave -- against the same plants gathered into a small one-block
    handle given the same orders: every column of the ordered plants bit for bit, every other plant untouched"""
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    if segment is None:
        monkeypatch.delenv("NPB_ARENA_SEGMENT", raising=False)
    else:
        monkeypatch.setenv("NPB_ARENA_SEGMENT", segment)
    n = 50000
    big = BatchedPlantEnv(n, dt=5.0)
    assert (big.L.npb_state_arena_segment(big._h) > 0) == (segment is None)
    _scrambled(big, 11)
    big.step()
    rng = np.random.default_rng(2025)
    chosen = np.sort(rng.choice(n, size=n * 3 // 100, replace=False))
    m = len(chosen)
    action = rng.integers(0, len(ACTIONS) + 2, m).astype(np.int32)
    unit = rng.integers(0, 4, m).astype(np.int32)
    option = rng.integers(0, 6, m).astype(np.int32)
    f0, i0 = big.state_arrays()
    monkeypatch.delenv("NPB_ARENA_SEGMENT", raising=False)
    small = BatchedPlantEnv(m, dt=5.0)
    assert small.L.npb_state_arena_segment(small._h) == 0
    idx = torch.as_tensor(chosen, device=big.device)
    small.load_state_arrays(f0[:, idx].contiguous(), i0[:, idx].contiguous())
    ok_small = small.perform_component_maintenance("condenser", action, unit=unit, cleaning_type=option).clone()
    A = np.full(n, -1, dtype=np.int32); A[chosen] = action
    U = np.zeros(n, dtype=np.int32); U[chosen] = unit
    C = np.zeros(n, dtype=np.int32); C[chosen] = option
    ok_big = big.perform_component_maintenance("condenser", A, unit=U, cleaning_type=C)
    want = np.array([int(a < len(ACTIONS) and (UNITS[ACTIONS[a][0]] == 1 or u < UNITS[ACTIONS[a][0]])) for a, u in zip(action, unit)], dtype=np.uint8)
    assert np.array_equal(ok_small.cpu().numpy(), want) and m // 2 < want.sum() < m
    assert torch.equal(ok_big[idx], ok_small) and int(ok_big.sum().item()) == int(want.sum())
    f1, i1 = big.state_arrays()
    fs, is_ = small.state_arrays()
    assert torch.equal(f1[:, idx].contiguous().view(torch.int64), fs.view(torch.int64)) and torch.equal(i1[:, idx].contiguous(), is_)
    rest = torch.ones(n, dtype=torch.bool, device=big.device); rest[idx] = False
    assert torch.equal(f1[:, rest].contiguous().view(torch.int64), f0[:, rest].contiguous().view(torch.int64)) and torch.equal(i1[:, rest], i0[:, rest])
    changed = (f1[:, idx] != f0[:, idx]).any(dim=0).cpu().numpy()
    assert changed.sum() > m // 4 and not changed[want == 0].any()
    big.close(); small.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the event log
def test_log_reports_one_record_per_successful_order():
    """oc3 (the log needs the automatic maintenance on, which this fixture's plant has) with the log on: the kind-3 records are exactly
    the fixture's successful calls -- catalog index, unit, the plant's clock -- for every lane, beside the automatic pump maintenance's
    own created / completed records, which the calls do not disturb"""
    name = "oc3_long_run"
    n = 64
    env, g = _replay(name, 0, n=n, log=8192)
    rec = env.maintenance_log_records()
    dt = float(g.meta["dt"])
    want = sorted((o.step * dt, o.unit if UNITS[ACTIONS[o.action][0]] > 1 else 0, o.action) for o in g.ops if o.success)
    assert len(want) == 5
    ops = rec[rec["kind"] == OPERATOR_COMPONENT]
    assert len(ops) == n * len(want)
    for lane in range(n):
        r = ops[ops["plant"] == lane]
        assert sorted(zip(r["time"].tolist(), r["pump"].tolist(), r["action"].tolist())) == want, lane
        assert np.all(r["order"] == 0) and np.array_equal(r["created"], r["time"]) and np.array_equal(r["planned_start"], r["time"])
        assert np.all(r["trigger"] == 0) and np.all(r["priority"] == 0) and np.all(r["bearing"] == 0)
    auto = rec[rec["kind"] != OPERATOR_COMPONENT]
    labels = [c[2] for c in g.cols]
    performed = int(g.state[-1, labels.index("maint.maintenance_actions_performed")])
    created = int(g.state[-1, labels.index("maint.work_orders_created")])
    assert performed >= 1 and set(auto["kind"].tolist()) <= {0, 1}
    assert int((auto["kind"] == 1).sum()) == n * performed and int((auto["kind"] == 0).sum()) == n * created
    env.close()


def test_formatted_log_names_component_and_action_beside_a_pump_order():
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 130
    env = BatchedPlantEnv(n, dt=5.0, maintenance=True)
    env.enable_maintenance_log(1024)
    env.step()
    mask = np.zeros(n, dtype=np.uint8); mask[[0, 64, 129]] = 1
    env.perform_component_maintenance("steam_generator", "tsp_mechanical_cleaning", unit=2, mask=mask)
    env.perform_component_maintenance("ejector", "vacuum_ejector_nozzle_replacement", unit="SJE-002", mask=mask)
    env.perform_component_maintenance("steam_generator", "scale_removal", unit=3)           # no such generator: no record
    env.perform_maintenance("oil_change", "FWP-3", mask=mask)
    cols = env.maintenance_log()
    sel = cols["event_type"] == "operator_component_maintenance"
    assert list(cols["plant"][sel]) == [0, 0, 64, 64, 129, 129]
    assert list(cols["component_id"][sel]) == ["SJE-002", "SG-2"] * 3 or list(cols["component_id"][sel]) == ["SG-2", "SJE-002"] * 3
    assert set(cols["action_type"][sel]) == {"tsp_mechanical_cleaning", "vacuum_ejector_nozzle_replacement"}
    assert list(cols["timestamp_minutes"][sel]) == [5.0] * 6 and list(cols["work_order_id"][sel]) == [""] * 6
    pump = cols["event_type"] == "operator_maintenance"
    assert list(cols["plant"][pump]) == [0, 64, 129] and list(cols["component_id"][pump]) == ["FWP-3"] * 3
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5. modes, arguments
def test_modes_that_do_not_step_a_component_do_not_service_it():
    """primary only: the reference then has no secondary_physics to call -- success 0 for every kind; primary + steam generators: the
    generators and their system are serviced, condenser and ejectors are not"""
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 70
    for mode, serviced in (("primary", ()), ("primary_sg", ("steam_generator", "steam_generator_system"))):
        env = BatchedPlantEnv(n, dt=5.0, mode=mode)
        env.step()
        for kind, name in (("steam_generator", "tsp_chemical_cleaning"), ("steam_generator_system", "routine_maintenance"),
                           ("condenser", "condenser_tube_cleaning"), ("ejector", "general")):
            f0, i0 = _bits(env)
            ok = env.perform_component_maintenance(kind, name, unit=1)
            assert bool(ok.all().item()) == (kind in serviced) and bool(ok.any().item()) == (kind in serviced), (mode, kind)
            if kind not in serviced:
                f1, i1 = _bits(env)
                assert torch.equal(f0, f1) and torch.equal(i0, i1), (mode, kind)
        env.close()


def test_missing_action_column_is_refused_and_the_optional_ones_may_be_null():
    from nuclear_sim_amd import _lib
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv(64, dt=5.0)
    assert env.L.npb_perform_component_maintenance(env._h, None, None, None, None, None, None) == -1
    assert b"npb_perform_component_maintenance" in env.L.npb_last_error(env._h)
    env.set_field("cond.current_air_leakage", np.full(64, 0.1))
    a = torch.full((64,), _lib.component_action_index("condenser", "vacuum_leak_detection"), dtype=torch.int32, device=env.device)
    assert env.L.npb_perform_component_maintenance(env._h, ctypes.c_void_p(a.data_ptr()), None, None, None, None, env._stream()) == 0
    assert bool((env.get_field("cond.current_air_leakage") == 0.05).all().item())
    # the amount column is accepted and read by no handler
    amount = torch.full((64,), 25.0, dtype=torch.float64, device=env.device)
    ok = env.perform_component_maintenance("condenser", "vacuum_leak_detection", tubes_to_plug=amount)
    assert bool(ok.all().item()) and bool((env.get_field("cond.current_air_leakage") == 0.025).all().item())
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 6. episodes
def test_autoreset_and_restore_take_the_operators_work_with_the_episode():
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    n, K = 200, 6
    env = BatchedPlantEnv(n, dt=5.0)
    env.set_field("cond.biofouling_thickness", np.full(n, 0.8))
    for k in range(7):
        env.set_field("sg.tsp_magnetite", np.full(n, 1.0), instance=1, k=k)
    env.snapshot()
    env._enable_autoreset(K)
    f0, i0 = _bits(env)
    odd = torch.zeros(n, dtype=torch.uint8, device=env.device); odd[1::2] = 1
    for t in range(K):
        obs, rew, done, info = env.step()
        if t == 2:
            assert torch.equal(env.perform_component_maintenance("condenser", "condenser_tube_cleaning", mask=odd), odd)
            assert torch.equal(env.perform_component_maintenance("steam_generator", "tsp_chemical_cleaning", unit=1, mask=odd), odd)
            bio = env.get_field("cond.biofouling_thickness")
            assert bool((bio[1::2] < 0.2).all().item()) and bool((bio[0::2] > 0.79).all().item())
    assert bool(info["truncated"].all().item())
    f1, i1 = _bits(env)
    assert torch.equal(f0, f1) and torch.equal(i0, i1), "the restored state is not the snapshot's"
    env.step()
    env.perform_component_maintenance("steam_generator", "tsp_chemical_cleaning", unit=1, mask=odd)
    mag = env.get_field("sg.tsp_magnetite", instance=1, k=0).cpu().numpy()
    assert np.all(mag[1::2] < 0.26) and np.all(mag[0::2] > 0.99), mag[:4]
    env.restore()
    f2, i2 = _bits(env)
    assert torch.equal(f0, f2) and torch.equal(i0, i2), "restore() did not take the cleaning away"
    env.close()


# ---------------------------------------------------------------------------------------------------------------- the single-plant facade
def test_facade_answers_the_references_call_paths_with_its_success():
    """the reference's own call paths, with the success its result carries for the same calls in the fixtures (a catalogued type: True;
    an unknown one: False, on an ejector True -- its dispatcher falls through to general maintenance; a delegated one: the generator's)"""
    from nuclear_sim_amd.env import ConstantHeatSource, NuclearPlantSimulator
    sim = NuclearPlantSimulator(dt=5.0, heat_source=ConstantHeatSource(), enable_state_management=False)
    sec = sim.secondary_physics
    sgs, cond = sec.steam_generator_system, sec.condenser
    sg1 = sgs.steam_generators[1]
    sg1.tube_interior_fouling.scale_thickness = 1.0
    assert sg1.perform_maintenance("scale_removal", cleaning_type="mechanical") == {"success": True}
    assert abs(sg1.tube_interior_fouling.scale_thickness - 0.05) < 1e-12
    sg1.steam_quality = 0.97
    assert sgs.perform_maintenance("system_steam_quality_maintenance")["success"] is True
    assert abs(sg1.steam_quality - (0.97 + (0.999 - 0.97) * 0.8)) < 1e-12
    assert sg1.perform_maintenance("bogus_maintenance")["success"] is False
    assert sgs.perform_maintenance("bogus_maintenance")["success"] is False
    assert sgs.perform_maintenance("tsp_chemical_cleaning", sg_index=1)["success"] is True
    assert sgs.perform_maintenance("tsp_chemical_cleaning", sg_index=3)["success"] is False
    assert sgs.perform_maintenance("condenser_tube_cleaning", sg_index=1)["success"] is False       # no generator knows it
    for name in ("load_balancing_maintenance", "system_coordination_maintenance", "routine_maintenance"):
        assert sgs.perform_maintenance(name)["success"] is True
    cond.fouling_model.biofouling_thickness = 1.0
    assert cond.perform_maintenance("condenser_tube_cleaning", cleaning_type="hydroblast")["success"] is True
    assert abs(cond.fouling_model.biofouling_thickness - 0.1) < 1e-12 and cond.fouling_model.time_since_cleaning == 0.0
    assert cond.perform_maintenance("bogus_maintenance")["success"] is False
    assert cond.perform_maintenance("vacuum_system_test")["success"] is True
    ej = cond.vacuum_system.ejectors["SJE-002"]
    assert ej.perform_maintenance("vacuum_ejector_inspection")["success"] is True
    assert ej.perform_maintenance("whatever_else")["success"] is True                                # general maintenance
    assert cond.vacuum_system.ejectors["SJE-001"].perform_maintenance("vacuum_ejector_cleaning", cleaning_type="replacement")["success"] is True
    with pytest.raises(ValueError, match="not offered"):
        cond.perform_maintenance("condenser_tube_plugging", tubes_to_plug=10)
    with pytest.raises(ValueError, match="not offered"):
        sgs.perform_maintenance("eddy_current_testing", sg_index=0)
    with pytest.raises(AttributeError):       # turbine maintenance is not on the device
        sec.turbine.perform_maintenance
    with pytest.raises((AttributeError, KeyError)):
        cond.vacuum_system.ejectors["SJE-003"]
    sim.step()
