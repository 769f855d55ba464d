"""GPU: the maintenance event log (npb_set_maintenance_log, BatchedPlantEnv.enable_maintenance_log / maintenance_log).  The records
the step kernels' maintenance rule appends are the work orders the reference creates and completes: equal, field for field, to the
events the golden fixtures' per-step state implies (tests/work_order_events.py) on every step kernel; consistent with the counters
at every step of config 4 and at its full size; written by npb_maint_kernel in the modes that do not step the pumps; without any
effect on the step's results; bounded by the capacity; and carried on across autoreset restores with the restored clock and counters."""
import ctypes

import numpy as np
import pytest

from golden_util import Golden, fixture_names
from work_order_events import assert_orders_match, events_from_golden, host_state, make_env, per_step, reference_orders, windows

pytestmark = pytest.mark.gpu

FIELDS = ("time", "created", "planned_start", "plant", "order", "trigger", "pump", "action", "kind", "priority", "bearing")
KERNEL_OF_VARIANT = {0: "npb_step4_maint_kernel", 1: "npb_step_maint_kernel", 2: "npb_step2_wide_maint_kernel", 3: "npb_step2_maint_kernel",
                     4: "npb_step_nt_maint_kernel", 5: "npb_step4_maint_kernel"}


def _params():
    from nuclear_sim_amd import _lib
    return _lib.MAINT_PARAMS


def _maint_fixtures():
    out = []
    for n in fixture_names():
        g = Golden(n)
        if not (g.meta.get("runner") or g.meta.get("state_management")) or g.meta.get("maint_unchecked") or g.resets:
            continue
        out.append((n, per_step(g)))
    return out


_ALL = _maint_fixtures()
PER_STEP = [n for n, dense in _ALL if dense]
SPARSE = [n for n, dense in _ALL if not dense]
EVERY_KERNEL = ("m1_oil_top_off_staggered", "m13b_oil_analysis", "z21_fuzzed_maintenance", "z22_fuzzed_maintenance", "z40_fuzzed_wide_running")


def _sorted(rec):
    from nuclear_sim_amd.maintlog import sort_events
    return sort_events(rec)


def _same_records(got, want, where):
    got, want = _sorted(got), _sorted(want)
    assert len(got) == len(want), "%s: %d records, want %d\n got %s\nwant %s" % (where, len(got), len(want), got[:8], want[:8])
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), "%s: field %s differs\n got %s\nwant %s" % (where, f, got[f][:16], want[f][:16])


def _replay(name, variant, storage="f64", n=64, states=False):
    """the fixture on n lanes with the log on; returns (records, env[, per-step host states])"""
    import torch
    g = Golden(name)
    env = make_env(g, n=n, storage=storage)
    env.set_step_kernel(variant)
    env.enable_maintenance_log(4096)
    f0, i0 = host_state(env)
    f, i, fm, im = g.split_state(g.state[0])
    f0[fm, :] = f[fm, None]; i0[im, :] = i[im, None]
    env.load_state_arrays(f0, i0)
    hist = [host_state(env)] if states else None
    for t in range(g.T):
        for label, v in g.pokes.get(t, []):
            kind, slot = g.label_slot(label)
            col = torch.full((n,), v, dtype=torch.float64 if kind == "f64" else torch.int32, device=env.device)
            env._set_slot(kind, slot, col)
        sp = None if np.isnan(g.setpoint[t]) else g.setpoint[t]
        cw = None if np.isnan(g.cooling[t]) else g.cooling[t]
        env.step(action=int(g.action[t]), magnitude=float(g.magnitude[t]), power_setpoint=sp, cooling_water_temp=cw, noise_z=float(g.noise_z[t]))
        assert env.last_step_kernel() == KERNEL_OF_VARIANT[variant], env.last_step_kernel()
        if states:
            hist.append(host_state(env))
    return env.maintenance_log_records(), env, g, hist


def _golden_for_all(g, n):
    ev = events_from_golden(g, _params())
    out = np.concatenate([ev.copy() for _ in range(n)]) if len(ev) else ev
    if len(ev):
        out["plant"] = np.repeat(np.arange(n), len(ev))
    return out


@pytest.mark.parametrize("name", PER_STEP)
def test_log_replays_golden_work_orders(name):
    """every fixture recorded at every step, all 64 lanes: the records equal the events of the reference's per-step state"""
    rec, env, g, _ = _replay(name, 0)
    _same_records(rec, _golden_for_all(g, 64), name)
    env.close()


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
@pytest.mark.parametrize("name", EVERY_KERNEL)
def test_log_replays_golden_work_orders_on_every_step_kernel(name, variant):
    rec, env, g, _ = _replay(name, variant)
    _same_records(rec, _golden_for_all(g, 64), "%s variant %d" % (name, variant))
    env.close()


@pytest.mark.parametrize("name", ("m1_oil_top_off_staggered", "m2_oil_top_off_simultaneous", "m8_handlers_inspection_overhaul_promotion",
                                  "m10_motor_bearing_replacement_seed1", "m13b_oil_analysis", "m13e_bearing_inspection",
                                  "z21_fuzzed_maintenance", "z22_fuzzed_maintenance"))
def test_log_equals_the_references_work_orders(name):
    """the drained log, formatted (env.maintenance_log()), of lanes 0 and 63 against the reference's WorkOrderManager after the same
    run (tests/golden/wo_<name>.json): ids, components, types, priorities, titles, actions, created, planned start, completion"""
    ref = reference_orders(name)
    assert ref is not None, name
    g = Golden(name)
    env = make_env(g, n=64)
    env.enable_maintenance_log(4096)
    f0, i0 = host_state(env)
    f, i, fm, im = g.split_state(g.state[0])
    f0[fm, :] = f[fm, None]; i0[im, :] = i[im, None]
    env.load_state_arrays(f0, i0)
    import torch
    for t in range(g.T):
        for label, v in g.pokes.get(t, []):
            kind, slot = g.label_slot(label)
            env._set_slot(kind, slot, torch.full((64,), v, dtype=torch.float64 if kind == "f64" else torch.int32, device=env.device))
        sp = None if np.isnan(g.setpoint[t]) else g.setpoint[t]
        cw = None if np.isnan(g.cooling[t]) else g.cooling[t]
        env.step(action=int(g.action[t]), magnitude=float(g.magnitude[t]), power_setpoint=sp, cooling_water_temp=cw, noise_z=float(g.noise_z[t]))
    cols = env.maintenance_log()
    for lane in (0, 63):
        sel = cols["plant"] == lane
        assert_orders_match({k: v[sel] for k, v in cols.items()}, ref, "%s lane %d" % (name, lane))
    env.close()


class _States:
    """a replay's per-step device states in the shape tests/work_order_events.py reads"""

    def __init__(self, g, hist, lane):
        self.name, self.meta, self.cols, self.T = g.name + " (device states)", g.meta, g.cols, g.T
        self.state_steps = np.arange(len(hist))
        rows = np.zeros((len(hist), len(g.cols)))
        for s, (f, i) in enumerate(hist):
            for j, (kind, slot, _lab, _p) in enumerate(g.cols):
                rows[s, j] = f[slot, lane] if kind == "f64" else i[slot, lane]
        self.state = rows


@pytest.mark.parametrize("name", ("m1_oil_top_off_staggered", "m13e_bearing_inspection", "z21_fuzzed_maintenance", "z24_fuzzed_maintenance"))
def test_log_follows_the_state_under_fp32_storage(name):
    """fp32 storage: the records equal the events the handle's own per-step state implies (lanes 0 and 63)"""
    rec, env, g, hist = _replay(name, 0, storage="f32", states=True)
    for lane in (0, 63):
        want = events_from_golden(_States(g, hist, lane), _params(), plant=lane)
        _same_records(rec[rec["plant"] == lane], want, "%s fp32 lane %d" % (name, lane))
    assert len(rec) > 0
    env.close()


@pytest.mark.parametrize("name", SPARSE)
def test_sparse_fixtures_agree_within_each_state_window(name):
    """fixtures recorded every few steps: per window between two recorded states, the creations and completions logged in it are
    the counters' increments, and the creations carry the order numbers the counter handed out"""
    rec, env, g, _ = _replay(name, 0, n=64)
    labels = [c[2] for c in g.cols]
    created0 = int(g.state[0, labels.index("maint.work_orders_created")])
    for plant in (0, 63):
        r = _sorted(rec[rec["plant"] == plant])
        for lo, hi, dc, dp in windows(g, _params()):
            w = r[(r["time"] > lo) & (r["time"] <= hi)]
            assert int((w["kind"] == 0).sum()) == dc and int((w["kind"] == 1).sum()) == dp, (name, plant, lo, hi)
        made = r[r["kind"] == 0]
        assert list(made["order"]) == list(range(created0 + 1, created0 + 1 + len(made))), (name, made["order"])
    env.close()


def test_counts_of_config4_every_step():
    """tests/golden/counts_c4_64seeds.npz drained after every step: each plant's cumulative creation and completion records equal the
    reference's work_orders_created and maintenance_actions_performed after that step"""
    from golden_util import Config4Counts
    from nuclear_sim_amd.env import BatchedPlantEnv
    c4 = Config4Counts()
    n = len(c4.seeds)
    env = BatchedPlantEnv.action_test("oil_top_off", c4.seeds, maintenance_log=1024)
    made = np.zeros(n, dtype=np.int64); done = np.zeros(n, dtype=np.int64)
    c0 = env.get_field("maint.work_orders_created").cpu().numpy().astype(np.int64)
    p0 = env.get_field("maint.maintenance_actions_performed").cpu().numpy().astype(np.int64)
    for t in range(c4.T):
        env.step(power_setpoint=c4.setpoint[:, t])
        r = env.maintenance_log_records()
        made += np.bincount(r["plant"][r["kind"] == 0], minlength=n)
        done += np.bincount(r["plant"][r["kind"] == 1], minlength=n)
        assert np.array_equal(c0 + made, c4.created[:, t]), t
        assert np.array_equal(p0 + done, c4.performed[:, t]), t
    assert made.sum() > 0 and done.sum() > 0
    env.close()


def _check_consistent(env, rec, c0, p0):
    """the log of a run against the arena: one record per counter increment, (plant, order, kind) unique, the orders still open in
    the log are the arena's open wo_order entries, no padding lane"""
    n = env.n
    assert rec["plant"].min(initial=0) >= 0 and rec["plant"].max(initial=0) < n, "a record names a padding lane"
    c1 = env.get_field("maint.work_orders_created").cpu().numpy().astype(np.int64)
    p1 = env.get_field("maint.maintenance_actions_performed").cpu().numpy().astype(np.int64)
    assert np.array_equal(np.bincount(rec["plant"][rec["kind"] == 0], minlength=n), c1 - c0)
    assert np.array_equal(np.bincount(rec["plant"][rec["kind"] == 1], minlength=n), p1 - p0)
    key = rec["plant"].astype(np.int64) * (1 << 33) + rec["order"].astype(np.int64) * 2 + rec["kind"]
    assert len(np.unique(key)) == len(rec), "a (plant, order, kind) is logged twice"
    made = rec[rec["kind"] == 0]; closed = rec[rec["kind"] == 1]
    open_log = set(zip(made["plant"].tolist(), made["pump"].tolist(), made["action"].tolist(), made["order"].tolist())) - \
        set(zip(closed["plant"].tolist(), closed["pump"].tolist(), closed["action"].tolist(), closed["order"].tolist()))
    open_arena = set()
    for k in range(4):
        for a in range(18):
            wo = env.get_field("mpump.wo_order", instance=k, k=a).cpu().numpy()
            for p in np.nonzero(wo > c0)[0]:      # orders created in this run and still open
                open_arena.add((int(p), k, a, int(wo[p])))
    assert open_log == open_arena


@pytest.mark.parametrize("n", [32768, 65536, 65535])
def test_config4_at_size(n):
    """config 4 for 48 steps (4 h) at 32 768, 65 536 and a ragged 65 535 plants, drained at the end"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), maintenance_log=1 << 20)
    c0 = env.get_field("maint.work_orders_created").cpu().numpy().astype(np.int64)
    p0 = env.get_field("maint.maintenance_actions_performed").cpu().numpy().astype(np.int64)
    rng = np.random.default_rng(n)
    for t in range(48):
        env.step(power_setpoint=rng.uniform(80.0, 100.0, n))
    rec = env.maintenance_log_records()
    assert len(rec) > n // 4, len(rec)
    _check_consistent(env, rec, c0, p0)
    env.close()


@pytest.mark.parametrize("mode", ["primary_sg", "primary"])
def test_maint_kernel_logs_in_modes_without_pumps(mode):
    """NPB_MODE_PRIMARY_SG / NPB_MODE_PRIMARY: npb_maint_kernel runs the rule; its records match the counters"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 200
    env = BatchedPlantEnv(n, dt=5.0, mode=mode, maintenance=True, params={"maint_start_delay_hours": 0.1})
    rng = np.random.default_rng(3)
    for k in range(4):
        env.set_field("pump.oil_level", rng.uniform(50.0, 70.0, n), instance=k)
    env.enable_maintenance_log(8192)
    c0 = env.get_field("maint.work_orders_created").cpu().numpy().astype(np.int64)
    p0 = env.get_field("maint.maintenance_actions_performed").cpu().numpy().astype(np.int64)
    for t in range(24):
        env.step()
    rec = env.maintenance_log_records()
    assert (rec["kind"] == 0).sum() > 0 and (rec["kind"] == 1).sum() > 0
    _check_consistent(env, rec, c0, p0)
    env.close()


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_log_changes_no_result(storage):
    """obs, reward, done, info and the whole arena bit-identical with the log on and off"""
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 3000

    def run(log):
        from nuclear_sim_amd import scenarios
        env = BatchedPlantEnv(n, dt=5.0, noise_enabled=True, noise_seeds=[42] * n, maintenance=True, storage=storage)
        eff = float(env.get_field("pump.lubrication_effectiveness")[0].item())
        env.set_fields(scenarios.action_test_fields("oil_top_off", range(n), eff, randomize=True))
        if log:
            env.enable_maintenance_log(1 << 16)
        rng = np.random.default_rng(5)
        outs = []
        for t in range(48):
            obs, rew, done, info = env.step(power_setpoint=rng.uniform(80.0, 100.0, n))
            outs.append([obs.clone(), rew.clone(), done.clone()] + [v.clone() for v in info.values() if torch.is_tensor(v)])
        f, i = env.state_arrays()
        rec = env.maintenance_log_records() if log else None
        env.close()
        return outs, f, i, rec
    a, fa, ia, _ = run(False)
    b, fb, ib, rec = run(True)
    assert len(rec) > 0
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert torch.equal(u.view(torch.uint8) if u.dtype == torch.float64 else u, v.view(torch.uint8) if v.dtype == torch.float64 else v)
    assert torch.equal(fa.view(torch.uint8), fb.view(torch.uint8)) and torch.equal(ia, ib)


def test_overflow_counts_and_guards():
    """capacity 4 on a run with more events: the cursor holds the true total, only the first 4 slots are written (the bytes behind
    them untouched), and the Python drain raises naming the dropped count"""
    import torch
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 256
    env = BatchedPlantEnv.action_test("oil_top_off", range(n))
    nb = int(env.L.npb_maint_event_bytes())
    buf = torch.full((64 * nb,), 0xAB, dtype=torch.uint8, device=env.device)
    cursor = torch.zeros(1, dtype=torch.int32, device=env.device)
    c0 = int(env.get_field("maint.work_orders_created").sum().item()) + int(env.get_field("maint.maintenance_actions_performed").sum().item())
    _lib.check(env.L.npb_set_maintenance_log(env._h, ctypes.c_void_p(buf.data_ptr()), 4, ctypes.c_void_p(cursor.data_ptr())), env._h)
    for t in range(24):
        env.step(power_setpoint=np.full(n, 95.0))
    c1 = int(env.get_field("maint.work_orders_created").sum().item()) + int(env.get_field("maint.maintenance_actions_performed").sum().item())
    total = int(cursor.item())
    assert total == c1 - c0 and total > 4
    head = buf[: 4 * nb].cpu().numpy()
    assert not np.all(head == 0xAB)
    assert np.all(buf[4 * nb:].cpu().numpy() == 0xAB), "a record was written past the capacity"
    env.enable_maintenance_log(4)
    for t in range(24):
        env.step(power_setpoint=np.full(n, 95.0))
    with pytest.raises(_lib.NpbError, match=r"\d+ dropped"):
        env.maintenance_log()
    rec = env.maintenance_log_records(allow_overflow=True)
    assert len(rec) == 4
    env.close()


def test_bad_arguments_are_refused():
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv(64, maintenance=True)
    L = env.L
    buf = torch.zeros(400, dtype=torch.uint8, device=env.device)
    cur = torch.zeros(1, dtype=torch.int32, device=env.device)
    assert L.npb_set_maintenance_log(env._h, ctypes.c_void_p(buf.data_ptr()), -1, ctypes.c_void_p(cur.data_ptr())) == -1
    assert L.npb_set_maintenance_log(env._h, ctypes.c_void_p(buf.data_ptr()), 10, None) == -1
    assert L.npb_set_maintenance_log(env._h, None, 10, ctypes.c_void_p(cur.data_ptr())) == -1
    assert L.npb_set_maintenance_log(env._h, ctypes.c_void_p(buf.data_ptr() + 4), 4, ctypes.c_void_p(cur.data_ptr())) == -1    # misaligned records
    assert L.npb_set_maintenance_log(env._h, None, 0, None) == 0
    with pytest.raises(ValueError):
        BatchedPlantEnv(64).enable_maintenance_log(16)
    env.close()


def test_log_off_again_writes_nothing():
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 256
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), maintenance_log=4096)
    ml = env._mlog
    env.enable_maintenance_log(None)
    for t in range(24):
        env.step(power_setpoint=np.full(n, 95.0))
    assert int(ml["cursor"].item()) == 0
    env.close()


@pytest.mark.parametrize("bank", [False, True])
def test_autoreset_records_carry_the_restored_clock_and_numbering(bank):
    """a time limit restores every plant (from its snapshot, or from the start bank): the records of the second episode carry the
    restored clock, and each plant's order numbers restart from the counter of the state it was restored to"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    n, K = 512, 20
    bank_seeds = list(range(9000, 9000 + n))
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), autoreset=True, max_episode_steps=K, maintenance_log=1 << 16,
                                      bank_seeds=bank_seeds if bank else None)
    t0 = env.get_field("prim.sim_time").cpu().numpy()
    if bank:     # default slots: plant p restarts from entry p of a bank built as action_test(bank_seeds)
        B = BatchedPlantEnv.action_test("oil_top_off", bank_seeds)
        c_restored = B.get_field("maint.work_orders_created").cpu().numpy().astype(np.int64)
        t_restored = B.get_field("prim.sim_time").cpu().numpy()
        B.close()
    else:
        c_restored = env.get_field("maint.work_orders_created").cpu().numpy().astype(np.int64)
        t_restored = t0
    for t in range(K):
        env.step(power_setpoint=np.full(n, 95.0))
    first = env.maintenance_log_records()           # episode one, up to and including the step that hit the limit
    assert len(first) > 0 and np.all(first["time"] <= t0[first["plant"]] + K * 5.0 + 1e-9)
    for t in range(K - 1):
        env.step(power_setpoint=np.full(n, 95.0))
    second = env.maintenance_log_records()          # episode two: K - 1 steps from the restored states
    assert len(second) > 0
    assert np.all(second["time"] > t_restored[second["plant"]]) and np.all(second["time"] <= t_restored[second["plant"]] + (K - 1) * 5.0 + 1e-9)
    made = second[second["kind"] == 0]
    assert len(made) > 0
    for p in np.unique(made["plant"]):
        orders = sorted(made["order"][made["plant"] == p].tolist())
        assert orders == list(range(c_restored[p] + 1, c_restored[p] + 1 + len(orders))), (p, orders, c_restored[p])
    env.close()
