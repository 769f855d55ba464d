"""GPU: a state log with a watch list (StateLog(env, plants=...): npb_sampler_create / npb_sampler_sample, one launch per sample) gives, bit
for bit, the table the full log gives for the same plants -- members, derived columns, result keys, clock columns, diagnostics rows, done,
episodes, history windows, side columns -- under both storage types, on a segmented arena, for ragged watch sizes and with several
samplers on one handle; and the reference's own log for a watched lane of a batch.

The common construction: 200 plants (not a multiple of 64, four waves' worth of lanes) of
BatchedPlantEnv.action_test("oil_top_off", seeds=range(200), diagnostics=True), every plant different, stepped 12 times with a moving
setpoint, every log recording after every step."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, T = 200, 12
IDS = [199, 0, 63, 64, 65, 128, 7]          # given unsorted: the ends, both sides of two wave borders, a lane inside a wave
RAGGED = {1: [137], 64: list(range(3, 195, 3)), 65: list(range(70, 135)), 200: list(range(200))}


def _make(n=N, **kw):
    from nuclear_sim_amd.env import BatchedPlantEnv
    return BatchedPlantEnv.action_test("oil_top_off", seeds=range(n), diagnostics=True, **kw)


def _run(env, logs, steps=T, between=None):
    """step with a moving setpoint; after every step each log records, in the order given"""
    for t in range(steps):
        env.step(power_setpoint=97.0 - 0.9 * t)
        for k, log in enumerate(logs):
            if between is not None and k:
                between()
            log.record(t + 1, (t + 1) * env.dt)
    return logs


def _same_table(got, want, what=""):
    """column names, their order, their types and every value; float64 columns by their bit patterns (NaNs compare equal)"""
    assert got.column_names == want.column_names, what
    assert [f.type for f in got.schema] == [f.type for f in want.schema], what
    assert got.num_rows == want.num_rows, what
    for name in got.column_names:
        a, b = got[name].to_numpy(), want[name].to_numpy()
        assert a.dtype == b.dtype, (what, name)
        if a.dtype == np.float64:
            a, b = a.view(np.int64), b.view(np.int64)
        if not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0]
            raise AssertionError("%s column %s differs in %d of %d rows, first at row %d: %r vs %r" % (
                what, name, len(bad), len(a), bad[0], got[name].to_numpy()[bad[0]], want[name].to_numpy()[bad[0]]))


def _plants_differ(full):
    """any two plants differ in at least one member column: a wrong id in the watched log would show"""
    last = full.array()[-1]           # [fields, plants]
    assert len(np.unique(last.T, axis=0)) == last.shape[1]


def _full_and_watched(order, ids=IDS, **kw):
    from nuclear_sim_amd.statelog import StateLog
    n = kw.pop("n", N)
    env = _make(n=n, **kw)
    full = StateLog(env, capacity=T, diagnostics=True)
    watched = StateLog(env, capacity=T, diagnostics=True, plants=ids)
    _run(env, [full, watched] if order == "full first" else [watched, full])
    return env, full, watched


@pytest.fixture(scope="module")
def base():
    """one fp64 run of the common construction: the full log, the watch list of test 1 and the ragged ones, recorded in that order"""
    from nuclear_sim_amd.statelog import StateLog
    env = _make()
    full = StateLog(env, capacity=T, diagnostics=True)
    logs = {"full": full, "ids": StateLog(env, capacity=T, diagnostics=True, plants=IDS)}
    for k, ids in RAGGED.items():
        logs[k] = StateLog(env, capacity=T, diagnostics=True, plants=ids)
    _run(env, list(logs.values()))
    _plants_differ(full)
    yield env, logs
    for log in logs.values():
        log.close()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 1
def test_watched_table_equals_the_full_tables_rows_fp64(base):
    env, logs = base
    full, watched = logs["full"], logs["ids"]
    assert watched.plants == sorted(IDS)
    got = watched.table()
    _same_table(got, full.table(plants=sorted(IDS)), "full first")
    names = set(got.column_names)
    assert len(names) > 784 and "primary.reactor.scram_activated" in names          # the reference's columns + step, time, plant
    assert got["plant"].to_numpy()[:len(IDS)].tolist() == sorted(IDS)
    assert watched.array().shape == (T, len(watched.columns), len(IDS))
    assert np.array_equal(watched.array().view(np.int64), full.array()[:, :, sorted(IDS)].view(np.int64))
    # a subset of the watch list, in the caller's order
    _same_table(watched.table(plants=[128, 0]), full.table(plants=[128, 0]), "subset")
    # the opposite order of recording, on a second run
    env2, full2, watched2 = _full_and_watched("watched first")
    _same_table(watched2.table(), full2.table(plants=sorted(IDS)), "watched first")
    _same_table(watched2.table(), got, "the two runs")
    env2.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def test_watched_table_equals_the_full_tables_rows_fp32_storage():
    for order in ("full first", "watched first"):
        env, full, watched = _full_and_watched(order, storage="f32")
        assert env.storage == "f32"
        _plants_differ(full)
        _same_table(watched.table(), full.table(plants=sorted(IDS)), order)
        env.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_segmented_arena(monkeypatch):
    """n = 192 with NPB_ARENA_SEGMENT=64: three segments; the watched ids sit on both sides of the borders"""
    ids = [63, 64, 127, 128, 191]
    monkeypatch.setenv("NPB_ARENA_SEGMENT", "64")
    env, full, watched = _full_and_watched("full first", ids=ids, n=192)
    assert int(env.L.npb_state_arena_segment(env._h)) == 64
    _plants_differ(full)
    _same_table(watched.table(), full.table(plants=ids), "segmented: full against watched")
    monkeypatch.setenv("NPB_ARENA_SEGMENT", "0")
    env0, full0, watched0 = _full_and_watched("watched first", ids=ids, n=192)
    assert int(env0.L.npb_state_arena_segment(env0._h)) == 0
    _same_table(watched.table(), watched0.table(), "segmented against one block")
    env.close(); env0.close()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("n_watched", sorted(RAGGED))
def test_ragged_watch_sizes(base, n_watched):
    env, logs = base
    ids = RAGGED[n_watched]
    assert len(ids) == n_watched and logs[n_watched].array().shape[2] == n_watched
    want = logs["full"].table() if n_watched == N else logs["full"].table(plants=ids)
    _same_table(logs[n_watched].table(), want, "%d watched" % n_watched)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_episodes():
    """autoreset with truncation after 5 steps and carried diagnostics: episode, episode_step and the history windows, NaN rows included"""
    from nuclear_sim_amd.statelog import history_log_columns, log_column_name
    for order in ("full first", "watched first"):
        env, full, watched = _full_and_watched(order, autoreset=True, max_episode_steps=5)
        got, want = watched.table(), full.table(plants=sorted(IDS))
        _same_table(got, want, "episodes, " + order)
        assert got["episode"].type == want["episode"].type and got["episode_step"].to_numpy().dtype == np.int64
        es = got["episode_step"].to_numpy().reshape(T, len(IDS))
        assert set(np.unique(es)) <= {0, 1, 2, 3, 4} and (es == 0).any() and got["episode"].to_numpy().max() >= 2
        for name in history_log_columns():
            col = got[log_column_name(name, watched.naming)].to_numpy().reshape(T, len(IDS))
            assert np.isnan(col[es == 0]).all() and not np.isnan(col[es >= 1]).all(), name
        env.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_a_watched_lane_reproduces_the_references_log_column_by_column():
    """fixture m1 as lane 67 of a 70-plant batch of as-built plants, watch list [67]: the reference's own log of that run, all 784 columns at
    every step, under the tolerance rule of test_gpu_parity.test_state_log_reproduces_the_references_log_column_by_column"""
    from golden_util import GOLDEN_DIR, Golden, RTOL
    from test_auto_component_gpu import LANE, N as N70, _place, _step
    from test_gpu_parity import _env
    from nuclear_sim_amd import statelog
    g = Golden("m1_oil_top_off_staggered")
    z = np.load(os.path.join(GOLDEN_DIR, "log_m1_oil_top_off_staggered.npz"))
    ref_names = [str(x) for x in z["names"]]; ref = z["log"]
    assert ref.shape == (g.T, len(ref_names)) and len(ref_names) == 784
    env = _env(g, n=N70)
    _place(env, g, LANE)
    log = statelog.StateLog(env, every=1, capacity=g.T, diagnostics=True, plants=[LANE])
    for t in range(g.T):
        _step(env, g, t, LANE)
        log.record(t + 1, (t + 1) * env.dt)
    tab = log.table()
    assert tab["plant"].to_numpy().tolist() == [LANE] * g.T
    produced = [c for c in tab.column_names if c not in ("step", "time", "plant")]
    assert set(produced) <= set(ref_names)
    assert sorted(set(ref_names) - set(produced)) == [] and len(produced) == 784
    poked = set(g.pokes)
    for name in produced:
        mine = tab[name].to_numpy()
        want = ref[:, ref_names.index(name)]
        floor = 1e-6 if name.endswith("fouling_energy_penalty_mw") else 1e-9
        ok = np.abs(mine - want) <= RTOL * np.abs(want) + floor
        if "turbine" in name:
            for t in poked:
                if t < g.T:
                    ok[t] = True
        assert ok.all(), (name, int(np.argmin(ok)), mine[~ok][:3], want[~ok][:3])
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_samplers_do_not_disturb_one_another():
    """two watched logs with different lists and different fields and env.secondary_result() (the handle's remembered gather request)
    between their record() calls: each table is that of the log alone on such an env"""
    from nuclear_sim_amd.statelog import StateLog
    fields = ["pump.oil_level", "sec.electrical_power_output", "fw.running_mask"]
    make_a = lambda env: StateLog(env, capacity=T, diagnostics=True, plants=[3, 70, 199])
    make_b = lambda env: StateLog(env, fields=fields, capacity=T, plants=[64, 5])
    env = _make()
    a, b = make_a(env), make_b(env)
    assert a._sampler != b._sampler
    name = "secondary.reactor_SECONDARY-COMP-001.heat_flow_net_electrical_output"
    results = []
    _run(env, [a, b], between=lambda: results.append(env.secondary_result()["heat_flow_net_electrical_output"][[3, 70, 199]].cpu().numpy()))
    alone = []
    for make in (make_a, make_b):
        e = _make()
        alone.append(_run(e, [make(e)])[0].table())
        e.close()
    _same_table(a.table(), alone[0], "reference layout")
    _same_table(b.table(), alone[1], "chosen fields")
    import pyarrow as pa
    assert b.table()["npb.fw.running_mask"].type == pa.int32() and b.table()["plant"].to_numpy()[:2].tolist() == [5, 64]
    # the result key the first log formed from its own narrow rows is what secondary_result() gave for those plants at that step
    assert np.array_equal(a.table()[name].to_numpy().reshape(T, 3).view(np.int64), np.stack(results).view(np.int64))
    # a destroyed sampler leaves the other one working; its id is refused afterwards
    sampler = a._sampler
    a.close()
    assert env.L.npb_sampler_sample(env._h, sampler, ctypes.c_void_p(b._buf.data_ptr()), env._stream()) == -1
    assert b"unknown or destroyed sampler id" in env.L.npb_last_error(env._h)
    b.clear(); b.record(1, 1.0)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_refusals_by_message(base):
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    from nuclear_sim_amd.statelog import StateLog
    env, logs = base
    with pytest.raises(ValueError, match=r"plant id 200 .*outside \[0, 200\)"):
        StateLog(env, plants=[0, 200])
    with pytest.raises(ValueError, match="plant id 3 .*twice"):
        StateLog(env, plants=[3, 1, 3])
    with pytest.raises(ValueError, match="plant 5 is not on this log's watch list"):
        logs["ids"].table(plants=[5])
    with pytest.raises(RuntimeError, match="StateLog is full"):       # the base logs hold their 12 samples
        logs["ids"].record(T + 1, 0.0)
    small = BatchedPlantEnv(8)
    log = StateLog(small, fields=["pump.oil_level"], capacity=4, plants=[1, 6])
    small.step(power_setpoint=95.0)
    log.record(1, 1.0)
    small.close()
    with pytest.raises(_lib.NpbError, match="the env is closed"):
        log.record(2, 2.0)
    assert log.array().shape == (1, 4, 2)          # what was sampled stays readable
    log.close()


def test_the_library_refuses_a_bad_request_by_name(base):
    """npb_sampler_create validates the whole request before any device work"""
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.schema import SCHEMA
    env, _logs = base
    L, h = env.L, env._h

    def create(ids, kinds=(0,), slots=(0,), sources=()):
        desc = _lib.NpbSamplerDesc()
        desc.n_watched = len(ids); desc.plants = (ctypes.c_int32 * max(len(ids), 1))(*ids)
        desc.n_fields = len(kinds); desc.kinds = (ctypes.c_int * max(len(kinds), 1))(*kinds); desc.slots = (ctypes.c_int * max(len(slots), 1))(*slots)
        arr = (_lib.NpbSampleSource * max(len(sources), 1))()
        for k, (base_ptr, typ) in enumerate(sources):
            arr[k].base = base_ptr; arr[k].type = typ; arr[k].rows = 1; arr[k].row_stride = 0; arr[k].plant_stride = 1
        desc.n_sources = len(sources); desc.sources = arr
        sampler = ctypes.c_int(99)
        rc = L.npb_sampler_create(h, ctypes.byref(desc), ctypes.byref(sampler))
        return rc, sampler.value, L.npb_last_error(h).decode()

    done = env._done.data_ptr()
    for args, text in ((dict(ids=[]), "n_watched must be at least 1"), (dict(ids=[0, N]), "plant id 200 is outside [0, 200)"),
                       (dict(ids=[-1]), "plant id -1 is outside"), (dict(ids=[4, 9, 4]), "plant id 4 is listed twice"),
                       (dict(ids=[1], kinds=(2,)), "bad field kind or slot"), (dict(ids=[1], slots=(1 << 20,)), "bad field kind or slot"),
                       (dict(ids=[1], sources=[(None, 3)]), "side source 0 has a NULL base"),
                       (dict(ids=[1], sources=[(done, 3), (done, 4)]), "side source 1 has the unknown element type 4")):
        rc, sampler, msg = create(**args)
        assert rc == -1 and sampler == -1 and text in msg, (args, rc, sampler, msg)
    rc, sampler, _msg = create(ids=[2, 1], sources=[(done, 3)])
    assert rc == 0 and sampler >= 0
    out = torch.full((2, 2), -1.0, dtype=torch.float64, device=env.device)
    assert L.npb_sampler_sample(h, sampler, ctypes.c_void_p(out.data_ptr()), env._stream()) == 0
    first = env._get_slot("f64", 0)
    assert out[0].tolist() == [float(first[2]), float(first[1])]
    kind, slot = SCHEMA.slot("pump.oil_level")
    rc, ordered, _msg = create(ids=[2, 1, 199], kinds=(0,), slots=(slot,))
    level = env._get_slot(kind, slot)
    assert float(level[1]) != float(level[2]) and rc == 0 and ordered != sampler
    out3 = torch.full((1, 3), -1.0, dtype=torch.float64, device=env.device)
    assert L.npb_sampler_sample(h, ordered, ctypes.c_void_p(out3.data_ptr()), env._stream()) == 0
    assert out3[0].tolist() == [float(level[2]), float(level[1]), float(level[199])]          # the caller's order is kept
    assert L.npb_sampler_destroy(h, ordered) == 0
    assert out[1].tolist() == [float(env._done[2]), float(env._done[1])]
    assert L.npb_sampler_destroy(h, sampler) == 0
    assert L.npb_sampler_destroy(h, sampler) == -1 and b"unknown or destroyed sampler id" in L.npb_last_error(h)
    assert L.npb_sampler_sample(h, 12345, ctypes.c_void_p(out.data_ptr()), env._stream()) == -1


# ---------------------------------------------------------------------------------------------------------------- 9
def test_a_watched_log_holds_nothing_of_the_width_of_the_batch():
    from nuclear_sim_amd.env import BatchedPlantEnv
    from nuclear_sim_amd.statelog import StateLog
    n, capacity = 4096, 16
    ids = [0, 63, 64, 1000, 2047, 2048, 4000, 4095]
    env = BatchedPlantEnv(n, maintenance=True)
    log = StateLog(env, capacity=capacity, diagnostics=True, plants=ids)
    rows = log._request["rows"]
    assert rows == len(log._request["members"]) + 17 + 170 + 1

    def tensors(x, seen):
        if isinstance(x, torch.Tensor):
            seen.append(x)
        elif isinstance(x, dict):
            for v in x.values():
                tensors(v, seen)
        elif isinstance(x, (list, tuple)):
            for v in x:
                tensors(v, seen)
        return seen
    own = tensors({k: v for k, v in vars(log).items() if k != "env"}, [])
    assert sum(t.numel() * t.element_size() for t in own) == capacity * rows * 8 * 8
    assert all(n not in t.shape and (n + 63) // 64 * 64 not in t.shape for t in own)
    env.step(power_setpoint=95.0)
    log.record(1, env.dt)
    full = StateLog(env, capacity=1, diagnostics=True)
    full.record(1, env.dt)
    _same_table(log.table(), full.table(plants=ids), "4 096 plants")
    env.close()
