"""GPU: the per-plant work-order summary folded from the maintenance event log on the device (npb_set_maintenance_summary,
BatchedPlantEnv.enable_maintenance_summary / maintenance_summary).  The tables equal, exactly, nuclear_sim_amd.maintlog.summarize over
the drained log and the reference's own recorded orders, on every step kernel and under fp32 storage; consuming the log gives the
tables keeping it gives; component and operator records are summarised under their catalogs; what the log had no room for is counted;
clear, since_minutes, restore and autoreset do what the header says; the feature changes no result; and nuclear_sim_amd.timing
answers the timing optimiser's question for a batch of probes.  Every batch has 64 to 70 plants: two waves, the second partial."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN_DIR, Golden
from maintenance_summary_ref import assert_same_tables, feedwater_keys, groups, reference_summary
from work_order_events import host_state, make_env

pytestmark = pytest.mark.gpu

N = 70
KERNEL_OF_VARIANT = {0: "npb_step4_maint_kernel", 1: "npb_step_maint_kernel", 2: "npb_step2_wide_maint_kernel", 3: "npb_step2_maint_kernel",
                     4: "npb_step_nt_maint_kernel"}
REPLAYED = ("m1_oil_top_off_staggered", "m2_oil_top_off_simultaneous", "m8_handlers_inspection_overhaul_promotion",
            "m10_motor_bearing_replacement_seed1", "z21_fuzzed_maintenance")
M2 = "m2_oil_top_off_simultaneous"


def _tables(env):
    """host copies of the summary's tables (the copy synchronises) and the dropped count"""
    s = env.maintenance_summary()
    return {k: s[k].cpu().numpy() for k in ("first_created", "first_completed", "n_created", "n_completed")}, int(s["dropped"].item()) & 0xFFFFFFFF


def _start(name, n=N, lanes=None, variant=0, storage="f64", **kw):
    """a batch set up as the fixture's run was, the fixture's initial state in ``lanes`` (None = every plant; the others stay as built)"""
    g = Golden(name)
    env = make_env(g, n=n, storage=storage, **kw)
    env.set_step_kernel(variant)
    f0, i0 = host_state(env)
    f, i, fm, im = g.split_state(g.state[0])
    sel = slice(None) if lanes is None else np.asarray(lanes)
    f0[np.ix_(fm, np.arange(n)[sel])] = f[fm, None]; i0[np.ix_(im, np.arange(n)[sel])] = i[im, None]
    env.load_state_arrays(f0, i0)
    return env, g


def _step(env, g, t, lanes=None):
    import torch
    for label, v in g.pokes.get(t, []):
        kind, slot = g.label_slot(label)
        if lanes is None:
            col = torch.full((env.n,), v, dtype=torch.float64 if kind == "f64" else torch.int32, device=env.device)
        else:
            col = env._get_slot(kind, slot)
            col[torch.as_tensor(np.asarray(lanes), device=env.device)] = v
        env._set_slot(kind, slot, col)
    sp = None if np.isnan(g.setpoint[t]) else g.setpoint[t]
    cw = None if np.isnan(g.cooling[t]) else g.cooling[t]
    return env.step(action=int(g.action[t]), magnitude=float(g.magnitude[t]), power_setpoint=sp, cooling_water_temp=cw, noise_z=float(g.noise_z[t]))


def _run(env, g, lanes=None, steps=None, each=None):
    for t in range(g.T if steps is None else steps):
        _step(env, g, t, lanes)
        if each is not None:
            each(t)


def _replay_and_compare(name, variant, storage="f64"):
    """test 4: the first sixteen keys folded step by step while the fixture runs, the other groups folded from the kept log at the end
    (one fold over every record: the strided loop over several blocks); all against summarize(drained log), lane 0 and the last lane
    against the reference's own orders"""
    from nuclear_sim_amd import maintlog
    env, g = _start(name, variant=variant, storage=storage)
    env.enable_maintenance_log(4096)
    G = groups(feedwater_keys())
    assert len(G) == 3 and all(len(k) <= 16 for k in G)
    env.enable_maintenance_summary(G[0])
    _run(env, g, each=lambda t: None if env.last_step_kernel() == KERNEL_OF_VARIANT[variant] else pytest.fail(env.last_step_kernel()))
    got = [_tables(env)]
    for keys in G[1:]:
        env.enable_maintenance_summary(keys, include_logged=True)
        got.append(_tables(env))
    rec = env.maintenance_log_records()
    assert len(rec) >= 6 * N and rec["plant"].max() == N - 1
    for keys, (tables, dropped) in zip(G, got):
        where = "%s variant %d %s" % (name, variant, storage)
        assert dropped == 0, where
        assert_same_tables(tables, maintlog.summarize(rec, keys, N), where)
        if storage == "f64":      # (under fp32 storage the device's run is its own: held to its own log, above)
            assert_same_tables(tables, reference_summary(name, keys), where + " against the reference's orders", plants=[0, N - 1])
    assert sum(int(t["n_created"].sum()) for t, _ in got) > 0
    env.close()


@pytest.mark.parametrize("name", REPLAYED)
def test_tables_equal_the_restatement_and_the_reference(name):
    """fails without the feature: there is no summary"""
    _replay_and_compare(name, 0)


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
@pytest.mark.parametrize("name", REPLAYED)
def test_tables_on_every_step_kernel(name, variant):
    _replay_and_compare(name, variant)


def test_tables_under_fp32_storage():
    _replay_and_compare("z21_fuzzed_maintenance", 0, storage="f32")


def test_m2_folds_four_creations_into_one_cell():
    """the four pumps of every plant create oil_top_off in one step: one fold, four atomic updates per cell"""
    env, g = _start(M2)
    env.enable_maintenance_summary(["oil_top_off", ("feedwater", "oil_top_off", 2)])
    _run(env, g, steps=2)
    t, dropped = _tables(env)
    assert dropped == 0
    assert np.all(t["n_created"][0] == 4) and np.all(t["n_created"][1] == 1) and np.all(t["first_created"] == 5.0)
    assert np.all(t["n_completed"] == 0) and np.all(np.isinf(t["first_completed"]))
    env.close()


def test_consume_mode_equals_keep_mode():
    """test 5: m2 in 17 lanes of 70 (68 records in one step, a log of exactly 70), consumed against kept"""
    from nuclear_sim_amd import _lib, maintlog
    lanes = 1 + 4 * np.arange(17)
    keys = groups(feedwater_keys())[1]      # oil_top_off per unit among them
    out = {}
    for mode in ("consume", "keep"):
        env, g = _start(M2, lanes=lanes)
        if mode == "keep":
            env.enable_maintenance_log(4096)
        env.enable_maintenance_summary(keys, log_capacity=N)
        assert env._msum["consume"] == (mode == "consume") and env._mlog["capacity"] == (N if mode == "consume" else 4096)
        cursors = []
        _run(env, g, lanes=lanes, each=lambda t: cursors.append(int(env._mlog["cursor"].item())))
        out[mode] = _tables(env)
        if mode == "consume":
            assert cursors == [0] * g.T, "the consumed log's cursor is 0 after every step"
            with pytest.raises(_lib.NpbError, match="keep_log=True"):
                env.maintenance_log_records()
            with pytest.raises(_lib.NpbError, match="keep_log=True"):
                env.maintenance_log()
        else:
            assert max(np.diff([0] + cursors)) == 4 * len(lanes) <= N, "the step the consumed log has to hold"
            rec = env.maintenance_log_records()
            assert_same_tables(out[mode][0], maintlog.summarize(rec, keys, N), "keep")
            assert set(rec["plant"]) == set(lanes.tolist())
        env.close()
    assert out["consume"][1] == 0 and out["keep"][1] == 0
    assert_same_tables(out["consume"][0], out["keep"][0], "consume against keep")
    assert out["keep"][0]["n_created"].sum() > 0 and out["keep"][0]["n_completed"].sum() > 0


class _AutoFixture:
    """one of the reference's runs with the automatic maintenance of generators and condenser on (tests/golden/auto_components/)"""

    def __init__(self, name):
        self.g = Golden("auto_components/" + name)
        self.side = json.load(open(os.path.join(GOLDEN_DIR, "auto_components", name + ".json")))
        self.thresholds = {kind: dict((n, c) for n, c in self.side["table"][kind]) for kind in ("steam_generator", "condenser")}


def test_components_and_operator_kinds():
    """test 6: ac1_shared_queue in one lane with component keys against the reference's orders; an operator's oil change and a turbine
    bearing alignment appear as completions at the call's clock under operator=True keys, and not under operator=False keys"""
    from nuclear_sim_amd import maintlog
    fx = _AutoFixture("ac1_shared_queue")
    g, lane = fx.g, 67
    env = make_env(g, n=N, component_maintenance=True, component_thresholds=fx.thresholds)
    f0, i0 = host_state(env)
    f, i, fm, im = g.split_state(g.state[0])
    f0[fm, lane] = f[fm]; i0[im, lane] = i[im]
    env.load_state_arrays(f0, i0)
    env.enable_maintenance_log(4096)
    chem, scale, tube = ("steam_generator", "tsp_chemical_cleaning"), ("steam_generator", "scale_removal"), ("condenser", "condenser_tube_cleaning")
    keys = [("component", chem, None), ("component", chem, 0), ("component", chem, 1), ("component", chem, 2), ("component", scale, 1),
            ("component", tube, None), ("component", None, None), ("feedwater", "oil_top_off", None), ("feedwater", "oil_change", None),
            ("turbine", ("bearing", "bearing_alignment"), None), ("turbine", None, 1)]
    env.enable_maintenance_summary(keys, operator=True)
    _run(env, g, lanes=[lane])
    t, dropped = _tables(env)
    assert dropped == 0
    # the fixture's lane against the reference's orders, reduced here
    want = {"n_created": [2, 1, 0, 1, 1, 1, 5, 1, 0, 0, 0], "n_completed": [2, 1, 0, 1, 1, 1, 5, 1, 0, 0, 0],
            "first_created": [5.0, 5.0, np.inf, 5.0, 10.0, 5.0, 5.0, 140.0, np.inf, np.inf, np.inf],
            "first_completed": [20.0, 20.0, np.inf, 35.0, 80.0, 50.0, 20.0, 155.0, np.inf, np.inf, np.inf]}
    orders = fx.side["orders"]
    assert [o["created"] for o in orders if o["action"] == "tsp_chemical_cleaning"] == [5.0, 5.0] and len(orders) == 6      # (the fixture is the one reduced above)
    for k, w in want.items():
        assert t[k][:, lane].tolist() == w, (k, t[k][:, lane].tolist(), w)
    # the operator's calls: every plant's pump 0, the fixture lane's bearing 1
    import torch
    clock = env.get_field("prim.sim_time").cpu().numpy()
    assert np.all(env.perform_maintenance("oil_change", 0).cpu().numpy() == 1)
    mask = torch.zeros(N, dtype=torch.bool, device=env.device); mask[lane] = True
    assert int(env.perform_turbine_maintenance("bearing", "bearing_alignment", unit=1, mask=mask).sum().item()) == 1
    t2, dropped = _tables(env)
    assert dropped == 0
    assert np.array_equal(t2["first_completed"][8], clock) and np.all(t2["n_completed"][8] == 1) and np.all(t2["n_created"][8] == 0)
    for j in (9, 10):
        assert t2["n_completed"][j].tolist() == [int(p == lane) for p in range(N)]
        assert t2["first_completed"][j, lane] == clock[lane] and np.isinf(np.delete(t2["first_completed"][j], lane)).all()
    for k in t:
        assert np.array_equal(t2[k][:8], t[k][:8]), k
    # the same log under work-order keys alone: the operator's records match nothing
    env.enable_maintenance_summary(keys[:9], include_logged=True)
    t3, dropped = _tables(env)
    assert dropped == 0 and np.all(t3["n_completed"][8] == 0) and np.isinf(t3["first_completed"][8]).all()
    rec = env.maintenance_log_records()
    assert {3, 4} & set(rec["kind"].tolist()) == {4} and 2 in set(rec["kind"].tolist()) and {5, 6} <= set(rec["kind"].tolist())
    assert_same_tables(t2, maintlog.summarize(rec, keys, N, operator=True), "operator keys")
    assert_same_tables(t3, maintlog.summarize(rec, keys[:9], N), "work-order keys")
    env.close()


def test_loss_is_reported():
    """test 7: a kept log of 8 records on m2 (eight events a plant): dropped is the log's own overflow count, the tables are the eight
    records that survived"""
    from nuclear_sim_amd import maintlog
    env, g = _start(M2)
    env.enable_maintenance_log(8)
    keys = ["oil_top_off", ("feedwater", None, None), ("feedwater", "oil_top_off", 3)]
    env.enable_maintenance_summary(keys)
    _run(env, g)
    t, dropped = _tables(env)
    cursor = int(env._mlog["cursor"].item())
    assert cursor == 8 * N and dropped == cursor - 8
    rec = env.maintenance_log_records(allow_overflow=True)
    assert len(rec) == 8
    assert_same_tables(t, maintlog.summarize(rec, keys, N), "the surviving records")
    assert t["n_created"][1].sum() == 8
    env.close()


def test_clear_since_restore_and_autoreset():
    """test 8"""
    import torch
    from nuclear_sim_amd import maintlog
    from nuclear_sim_amd.env import BatchedPlantEnv
    name = "m1_oil_top_off_staggered"
    keys = ["oil_top_off", ("feedwater", None, 1), ("feedwater", None, None)]
    env, g = _start(name)
    env.enable_maintenance_log(4096)
    env.snapshot()
    env.enable_maintenance_summary(keys, since_minutes=20.0)      # m1: events at 5, 15, 20 (two), 35 and 50 minutes
    _run(env, g)
    t, dropped = _tables(env)
    rec = env.maintenance_log_records(clear=False)
    assert dropped == 0 and (rec["time"] < 20.0).any() and (rec["time"] == 20.0).any()
    assert_same_tables(t, maintlog.summarize(rec, keys, N, since_minutes=20.0), "since 20")
    assert_same_tables(t, reference_summary(name, [("feedwater", "oil_top_off", None), ("feedwater", None, 1), ("feedwater", None, None)], 20.0),
                       "since 20, the reference's orders", plants=[0, N - 1])
    whole = maintlog.summarize(rec, keys, N)
    assert whole["n_created"].sum() > t["n_created"].sum() and np.all(t["first_created"][np.isfinite(t["first_created"])] >= 20.0)
    # restore: the arena goes back, the summary stays
    env.restore()
    after, _ = _tables(env)
    assert float(env.get_field("prim.sim_time").max().item()) < g.T * float(g.meta["dt"]), "the clock did not go back"
    assert_same_tables(after, t, "after restore")
    # clear(mask): exactly the masked plants
    mask = np.zeros(N, dtype=bool); mask[[3, 64, 69]] = True
    env.clear_maintenance_summary(torch.as_tensor(mask))
    cleared, _ = _tables(env)
    for k in t:
        assert np.array_equal(cleared[k][:, ~mask], t[k][:, ~mask]), k
    assert np.isinf(cleared["first_created"][:, mask]).all() and np.isinf(cleared["first_completed"][:, mask]).all()
    assert not cleared["n_created"][:, mask].any() and not cleared["n_completed"][:, mask].any() and t["n_created"][:, mask].any()
    env.clear_maintenance_summary()
    cleared, _ = _tables(env)
    assert np.isinf(cleared["first_created"]).all() and not cleared["n_completed"].any()
    env.close()
    # autoreset: the time limit restores every plant at step K; the tables go on counting across it
    K = 30
    env = BatchedPlantEnv.action_test("oil_top_off", range(N), autoreset=True, max_episode_steps=K, maintenance_log=4096)
    env.enable_maintenance_summary(["oil_top_off"])
    sp = np.full(N, 90.0)
    t0 = env.get_field("prim.sim_time").cpu().numpy()
    for _ in range(K):
        env.step(power_setpoint=sp)
    first, dropped = _tables(env)
    assert dropped == 0 and first["n_created"].sum() > 0
    assert np.array_equal(env.get_field("prim.sim_time").cpu().numpy(), t0), "the time limit did not restore every plant"
    for _ in range(K - 1):
        env.step(power_setpoint=sp)
    both, dropped = _tables(env)
    rec = env.maintenance_log_records()
    assert dropped == 0
    assert_same_tables(both, maintlog.summarize(rec, ["oil_top_off"], N), "across the autoreset")
    assert both["n_created"].sum() > first["n_created"].sum() and np.all(both["n_created"] >= first["n_created"])
    assert np.all(both["first_created"] <= first["first_created"])
    env.close()


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_summary_changes_no_result(storage):
    """test 9: obs, reward, done, info and the whole arena bit-identical with the summary on, off and on again, against a run without
    it; while it is off nothing is written to the tables it had"""
    import torch
    from nuclear_sim_amd import scenarios
    from nuclear_sim_amd.env import BatchedPlantEnv
    n, T = N, 48

    def run(summary):
        env = BatchedPlantEnv(n, dt=5.0, noise_enabled=True, noise_seeds=[42] * n, maintenance=True, storage=storage)
        eff = float(env.get_field("pump.lubrication_effectiveness")[0].item())
        env.set_fields(scenarios.action_test_fields("oil_top_off", range(n), eff, randomize=True))
        rng = np.random.default_rng(5)
        outs, held, seen = [], None, 0
        for t in range(T):
            if summary and t in (0, 32):
                env.enable_maintenance_summary(["oil_top_off", ("feedwater", None, None)])
            if summary and t == 16:
                held = env._msum      # the tables stay allocated here, so a stray write would land in them and be seen
                seen = int(held["counts"].sum().item())
                env.enable_maintenance_summary(None)
                held["times"].fill_(-7.0); held["counts"].fill_(-7); held["words"].fill_(-7)
            obs, rew, done, info = env.step(power_setpoint=rng.uniform(80.0, 100.0, n))
            outs.append([obs.clone(), rew.clone(), done.clone()] + [v.clone() for v in info.values() if torch.is_tensor(v)])
            if summary and t == 31:
                assert bool((held["times"] == -7.0).all()) and bool((held["counts"] == -7).all()) and bool((held["words"] == -7).all())
        if summary:
            assert int(env.maintenance_summary()["dropped"].item()) == 0
            seen += int(env.maintenance_summary()["n_created"].sum().item())
        f, i = env.state_arrays()
        made = int(env.get_field("maint.work_orders_created").sum().item())
        env.close()
        return outs, f, i, seen, made
    a, fa, ia, _, made = run(False)
    b, fb, ib, seen, _ = run(True)
    assert made > 0 and seen > 0, "nothing fired: the comparison would be vacuous"
    bits = lambda u: u.view(torch.uint8) if u.dtype == torch.float64 else u
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            assert torch.equal(bits(u), bits(v))
    assert torch.equal(fa.view(torch.uint8), fb.view(torch.uint8)) and torch.equal(ia, ib)


def test_refusals_with_a_handle():
    """what npb_maint_summary_check decides (tests/test_maintenance_summary_cpu.py), through the handle: its code and its message"""
    import torch
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv(N, maintenance=True)
    L = env.L
    buf = torch.zeros(4096, dtype=torch.float64, device=env.device)
    d = _lib.NpbMaintSummaryDesc()
    d.n_keys, d.consume = 1, 0
    d.keys[0].catalog, d.keys[0].action, d.keys[0].unit, d.keys[0].kinds = 0, 1, -1, 3
    d.first_created, d.first_completed, d.n_created, d.n_completed = (buf[k * 512:].data_ptr() for k in range(4))
    d.folded, d.dropped = buf[2048:].data_ptr(), buf[2049:].data_ptr()

    def refused(what):
        assert L.npb_set_maintenance_summary(env._h, ctypes.byref(d)) == -1
        assert what in L.npb_last_error(env._h).decode(), L.npb_last_error(env._h)
    refused("no maintenance log")
    assert L.npb_maint_summary_fold(env._h, None) == -1 and L.npb_maint_summary_clear(env._h, None, None) == -1
    env.enable_maintenance_log(N - 1)
    d.consume = 1
    refused("consume")
    d.consume, d.n_keys = 0, 17
    refused("n_keys")
    d.n_keys, d.keys[0].kinds = 1, 0
    refused("kinds")
    d.keys[0].kinds, d.keys[0].unit = 3, 4
    refused("unit")
    d.keys[0].unit, d.first_created = -1, buf.data_ptr() + 4
    refused("aligned")
    d.first_created = buf.data_ptr()
    assert L.npb_set_maintenance_summary(env._h, ctypes.byref(d)) == 0
    assert L.npb_maint_summary_fold(env._h, env._stream()) == 0
    assert L.npb_set_maintenance_summary(env._h, None) == 0 and L.npb_maint_summary_fold(env._h, None) == -1
    with pytest.raises(ValueError):
        BatchedPlantEnv(N).enable_maintenance_summary(["oil_top_off"])      # no automatic maintenance, no log
    env.close()


# test 10.  The oil level of pump 0 over the range of the composer's oil_top_off scenarios (scenarios.OIL_TOP_OFF_SCENARIOS: 59.2 ... 63.0),
# dt = 5 min, setpoint 90 %.  On the CPU oracle (oracle/npo.py, maintenance on, seed 7, the same 64 levels) every plant fires within 60
# steps, between 1.25 h (59.2) and 5.0 h (63.0), at 46 distinct times, non-decreasing in the level: the range needs no widening.
SEED, HOURS, DT = 7, 6.0, 5.0
LEVELS = np.linspace(63.0, 59.2, 64)
FIELD = ("pump.oil_level", 0)


@pytest.fixture(scope="module")
def trigger_run():
    """one run, shared: the summary's answer and the kept log of the same run"""
    from nuclear_sim_amd import timing
    out = timing.trigger_times("oil_top_off", [SEED] * 64, HOURS, dt=DT, fields=FIELD, values=LEVELS, unit=0, keep_log=True, return_env=True)
    env = out.pop("env")
    out["records"] = env.maintenance_log_records()
    env.close()
    return out


def test_trigger_times(trigger_run):
    from nuclear_sim_amd import maintlog, scenarios
    assert LEVELS.max() == max(s[2] for s in scenarios.OIL_TOP_OFF_SCENARIOS) and LEVELS.min() == min(s[1] for s in scenarios.OIL_TOP_OFF_SCENARIOS)
    r = trigger_run
    first = r["first_created_hours"]
    assert r["dropped"] == 0
    fired = np.isfinite(first)
    assert fired.any() and len(set(first[fired].tolist())) > 1
    assert np.all(np.diff(first[::-1][fired[::-1]]) >= 0), "first-created times must be non-decreasing in the level"
    # each equals the first creation drained from the kept log of the same run
    rec = r["records"]
    made = rec[(rec["kind"] == maintlog.CREATED) & (rec["action"] == 1) & (rec["pump"] == 0)]
    want = np.full(64, np.nan)
    for p in range(64):
        tp = made["time"][made["plant"] == p]
        if len(tp):
            want[p] = tp.min() / 60.0
    assert np.array_equal(first, want, equal_nan=True)
    done = r["first_completed_hours"]
    assert np.all(done[np.isfinite(done)] >= first[np.isfinite(done)])
    assert r["steps"] % 32 == 0 or r["steps"] == int(HOURS * 60 / DT)
    if fired.all():
        assert r["steps"] < int(HOURS * 60 / DT), "every plant had fired: the run should have stopped at the next look"


def test_sweep_finds_the_target(trigger_run):
    from nuclear_sim_amd import timing
    first = trigger_run["first_created_hours"]
    lo, hi = np.nanmin(first), np.nanmax(first)
    target, tol = 0.5 * (lo + hi), 0.1
    assert lo < target < hi
    s = timing.sweep("oil_top_off", SEED, FIELD, LEVELS.min(), LEVELS.max(), target, tol, points=64, rounds=3, dt=DT, unit=0)
    assert s["converged"] and abs(s["hours"] - target) <= tol and LEVELS.min() <= s["value"] <= LEVELS.max()
    probes = s["probes"]
    assert probes.shape[1] == 3 and len(probes) == 64 * s["rounds"]
    j = np.nanargmin(np.abs(probes[:, 2] - target))
    assert probes[j, 1] == s["value"] and probes[j, 2] == s["hours"]
