"""GPU: state windows around events captured on the device (npb_set_event_windows, BatchedPlantEnv.enable_event_windows / event_windows).

The reference is nuclear_sim_amd.eventwin.record, the numpy statement of the capture, over series the EXISTING paths return behind every
step: the sampler for all plants (npb_sampler_create / npb_sampler_sample with ids 0 .. n-1: arena members and the plant clock), and the
step's own output tensors cloned per step (an info column, an obs column, the reward, the trip flags, done, the summary's n_created row,
the episode index).  The window is copies, so every record matches by bits, NaN positions included, with no tolerance anywhere.

The run: BatchedPlantEnv.action_test("oil_top_off", seeds=range(n), dt=5.0), every plant with a setpoint of its own.  The plant clock
prim.sim_time advances by dt = 5 per step from whatever set_field put there, which makes ``("prim.sim_time", ">", X)`` a trigger whose
step is known beforehand for every plant; the low-flow poke of tests/test_episode_records_gpu.py makes a plant scram on the next step.

Episodes: the windows sample the end-of-step state BEFORE the autoreset restores an ended plant, which nothing returns after npb_step.
The arena members of that run come from a twin env without autoreset that is stepped and poked identically and restored by hand
(restore(mask)) where the env's episodes end, as in tests/test_column_stats_gpu.py; the test asserts the lockstep (reward bits) at every
step.  The terminal observation is the env's info["final_observation"]; the step's reward, info block, trip flags and done are not touched
by the restore."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, DT = 70, 5.0            # one full wave plus six lanes
KERNEL_OF_VARIANT = {0: "npb_step4_maint_kernel", 1: "npb_step_maint_kernel", 2: "npb_step2_wide_maint_kernel", 5: "npb_step4_maint_kernel"}
COLUMNS = [("pump.oil_level", 0),                 # a carried fp64 member
           ("sg.tube_wall_temp", 1),              # an OUTPUT member: the arena stores it as float
           ("info", "electrical_power"), ("obs", 5), "reward"]
MEMBERS = COLUMNS[:2]
ALL_BITS = 0xFFFFFFFF


def _np(t):
    return t.detach().cpu().numpy().copy()


def _make(n=N, **kw):
    from nuclear_sim_amd.env import BatchedPlantEnv
    return BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, **kw)


def _setpoint(t, n):
    return 90.0 + 8.0 * np.sin(2.0 * np.pi * t / (20.0 + np.arange(n) % 7))


def _poke(env, plants):
    """below the low-flow trip: the plant scrams on the next step (tests/test_episode_records_gpu.py)"""
    v = env.get_field("prim.coolant_flow_rate").cpu().numpy()
    v[list(plants)] = 4000.0
    env.set_field("prim.coolant_flow_rate", v)


class _Sampler:
    """the existing sampler path for ALL plants: ``members`` and the plant clock, one npb_sampler_sample per step into a buffer on the device"""

    def __init__(self, env, members, steps):
        from nuclear_sim_amd import _lib
        from nuclear_sim_amd.schema import SCHEMA
        keys = [SCHEMA.slot(*((m,) if isinstance(m, str) else m)) for m in members] + [SCHEMA.slot("prim.sim_time")]
        n, nm = env.n, len(keys)
        self.env, self._lib = env, _lib
        self._keep = ((ctypes.c_int32 * n)(*range(n)), (ctypes.c_int * nm)(*[0 if k == "f64" else 1 for k, _ in keys]), (ctypes.c_int * nm)(*[s for _, s in keys]))
        desc = _lib.NpbSamplerDesc(n, self._keep[0], nm, self._keep[1], self._keep[2], 0, None)
        sampler = ctypes.c_int(-1)
        _lib.check(env.L.npb_sampler_create(env._h, ctypes.byref(desc), ctypes.byref(sampler)), env._h)
        self.id = sampler.value
        self.ring = torch.zeros((steps, nm, n), dtype=torch.float64, device=env.device)

    def record(self, t):
        self._lib.check(self.env.L.npb_sampler_sample(self.env._h, self.id, ctypes.c_void_p(self.ring[t].data_ptr()), self.env._stream()), self.env._h)

    def result(self):
        """(members [steps, len(members), n], clock [steps, n])"""
        a = _np(self.ring)
        self._lib.check(self.env.L.npb_sampler_destroy(self.env._h, self.id), self.env._h)
        return a[:, :-1], a[:, -1]


def _run(env, steps, members=MEMBERS, extra=None, before=None, first=0):
    """Step with the moving setpoints.  Returns (values [steps, len(members) + 3, n] -- the members, then electrical power, obs 5 and the
    reward --, clock [steps, n], and what ``extra(obs, rew, done, info)`` gave per step, stacked: [steps, k, n]).  ``before(t)`` runs before
    step t"""
    ms = _Sampler(env, members, steps)
    sides = torch.zeros((steps, 3, env.n), dtype=torch.float64, device=env.device)
    more = []
    for t in range(steps):
        if before is not None:
            before(first + t)
        obs, rew, done, info = env.step(power_setpoint=_setpoint(first + t, env.n))
        ms.record(t)
        sides[t, 0], sides[t, 1], sides[t, 2] = info["electrical_power"], obs[:, 5], rew
        if extra is not None:
            more.append(torch.stack([x.to(torch.float64) for x in extra(obs, rew, done, info)]))
    m, clock = ms.result()
    return np.concatenate([m, _np(sides)], axis=1), clock, (_np(torch.stack(more)) if more else None)


def _stagger(env):
    """the plant clocks of test 1: 0.25 p + 5 (p % 7), every value a float too"""
    p = np.arange(env.n)
    env.set_field("prim.sim_time", 0.25 * p + 5.0 * (p % 7))


def _select(rec, keep):
    return {k: v[keep] for k, v in rec.items()}


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("variant, storage", [(1, "f64"), (2, "f64"), (5, "f64"), (0, "f32")])
def test_limit_trigger_staggered_over_the_batch(variant, storage):
    """A limit on the plant clock, crossed on a step of the plant's own; every kind of recorded column.  Fails without the feature:
    enable_event_windows does not exist"""
    from nuclear_sim_amd import eventwin
    X, pre, post, steps = 40.0, 3, 2, 12
    env = _make(storage=storage)
    env.set_step_kernel(variant)
    _stagger(env)
    env.enable_event_windows(COLUMNS, [("prim.sim_time", ">", X)], pre, post)
    values, clock, _ = _run(env, steps)
    assert env.last_step_kernel() == KERNEL_OF_VARIANT[variant], env.last_step_kernel()
    want = eventwin.record(values, clock, clock.reshape(steps, 1, N), [(">", X)], pre, post)
    # what the test is about, on the numpy statement alone
    assert len(want["plant"]) >= N // 2 and len(set(want["step"].tolist())) >= 5 and 1 in want["step"]
    assert np.sum(want["n_pre"] < pre) >= 1 and np.all(want["n_pre"][want["step"] == 1] == 1)
    assert len(set(range(N)) - set(want["plant"].tolist())) >= 1 and len(set(want["plant"].tolist())) == len(want["plant"])
    got = env.event_windows()
    eventwin.same(got, want)
    assert set(got) == set(want) and got["values"].shape == (len(want["plant"]), pre + 1 + post, len(COLUMNS))
    assert np.array_equal(got["times"][:, pre], got["time"]) and np.all(got["time"] > X) and np.all(got["time"] - DT <= X)
    assert len(env.event_windows()["plant"]) == 0                # drained
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def test_trip_and_done_triggers_with_autoreset():
    """max_episode_steps 12; triggers: rising trip bits, done, and the plant clock passing 27.5 (local step 5 of every episode, due at 8).
    Pokes before step t: plant 3 before 2 and again before 4 (its second episode: the ring holds two samples), plant 66 before 7 -- it is
    armed by the clock since 5, so the scram is a retrigger and cuts the capture short --, plant 69 before 22.  A scram ends the episode on
    the step it fires: early, n_post 0.  (A plant cannot be armed BY a poke and poked again while armed: the first scram ends the episode
    and the capture with it; the retrigger therefore comes from the clock trigger's capture.)"""
    from nuclear_sim_amd import eventwin
    L, pre, post, steps = 12, 4, 3, 30
    pokes = {2: [3], 4: [3], 7: [66], 22: [69]}
    columns = MEMBERS + ["prim.coolant_flow_rate", "reward", ("obs", 5)]
    members = MEMBERS + ["prim.coolant_flow_rate"]
    triggers = [("trip", ALL_BITS), ("done",), ("prim.sim_time", ">", 27.5)]
    env = _make(autoreset=True, max_episode_steps=L)
    twin = _make()
    twin.snapshot()
    env.enable_event_windows(columns, triggers, pre, post)
    ms = _Sampler(twin, members, steps)
    sides = torch.zeros((steps, 5, N), dtype=torch.float64, device=env.device)      # reward, obs 5, trip flags, done, episode index
    ended = torch.zeros((steps, N), dtype=torch.bool, device=env.device)
    for t in range(steps):
        if t in pokes:
            _poke(env, pokes[t]); _poke(twin, pokes[t])
        sp = _setpoint(t, N)
        obs, rew, done, info = env.step(power_setpoint=sp)
        _t_obs, t_rew, _t_done, _ = twin.step(power_setpoint=sp)
        ms.record(t)
        assert torch.equal(rew.view(torch.int64), t_rew.view(torch.int64)), "the twin left the env's path at step %d" % t
        ended[t] = (done != 0) | (info["truncated"] != 0)
        terminal = torch.where(ended[t].view(N, 1), info["final_observation"], obs)
        sides[t, 0], sides[t, 1], sides[t, 2], sides[t, 3], sides[t, 4] = rew, terminal[:, 5], info["trip_flags"], done, info["episode_index"]
        if bool(ended[t].any()):
            twin.restore(ended[t].to(torch.uint8))
    m, clock = ms.result()
    twin.close()
    s = _np(sides)
    values = np.concatenate([m, s[:, 0:2]], axis=1)
    tv = np.stack([s[:, 2], s[:, 3], clock], axis=1)
    want = eventwin.record(values, clock, tv, [("bits", ALL_BITS), ("bits", 1), (">", 27.5)], pre, post, ended=_np(ended), episode_index=s[:, 4])
    assert np.sum(want["early"]) >= 3 and np.sum(want["retriggers"] >= 1) >= 1
    early = _select(want, want["early"])
    assert sorted(early["plant"].tolist()) == [3, 3, 66, 69]
    by_poke = early["trigger"] == 0                  # armed by the scram itself: the capture is taken on the trigger step
    assert sorted(early["plant"][by_poke].tolist()) == [3, 3, 69] and np.all(early["n_post"][by_poke] == 0) and np.all(early["fired"][by_poke] == 3)
    assert early["n_pre"][early["plant"] == 3].tolist() == [2, 1] and early["episode"][early["plant"] == 3].tolist() == [0, 1]      # the restart limits n_pre
    r66 = _select(early, early["plant"] == 66)
    assert r66["trigger"].tolist() == [2] and r66["retriggers"].tolist() == [1] and r66["n_post"].tolist() == [2] and r66["step"].tolist() == [5]
    assert np.all(want["flags"][~want["early"]] == 0) and np.all(want["n_post"][~want["early"]] == post)
    got = env.event_windows()
    eventwin.same(got, want)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_work_order_trigger():
    """the summary's n_created row of the oil_top_off key going up; 40 steps"""
    from nuclear_sim_amd import eventwin
    pre, post, steps = 4, 3, 40
    env = _make(maintenance_log=16384)
    env.enable_maintenance_summary(["oil_top_off"])
    columns = [("pump.oil_level", 0), ("pump.oil_level", 1), ("pump.oil_level", 2)]
    env.enable_event_windows(columns, [("work_order", 0)], pre, post)
    created = env.maintenance_summary()["n_created"]
    values, clock, tv = _run(env, steps, members=columns, extra=lambda obs, rew, done, info: [created[0]])
    values = values[:, :3]
    want = eventwin.record(values, clock, tv, [("increase",)], pre, post)
    with_record = set(want["plant"].tolist())
    print("work-order windows: %d records of %d plants, %d plants without" % (len(want["plant"]), len(with_record), N - len(with_record)))
    assert len(with_record) * 4 >= N and (N - len(with_record)) * 4 >= N
    got = env.event_windows()
    eventwin.same(got, want)
    first_created = _np(env.maintenance_summary()["first_created"])[0]
    firsts = 0
    for i, p in enumerate(got["plant"]):
        if not np.any(got["plant"][:i] == p) and tv[0, 0, p] == 0:      # the plant's first record, and no order on the priming sample, which cannot fire
            assert got["time"][i:i + 1].view(np.int64)[0] == first_created[p:p + 1].view(np.int64)[0], (i, p)
            firsts += 1
        assert np.array_equal(got["values"][i, pre].view(np.int64), values[got["step"][i], :, p].view(np.int64))      # row `pre` is the sample of that step
    assert firsts >= N // 4
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_segmented_arena(monkeypatch):
    """n = 192 with NPB_ARENA_SEGMENT=64: a wave per segment; records of plants of all three segments, against numpy and against one segment"""
    from nuclear_sim_amd import eventwin
    X, pre, post, steps = 40.0, 3, 2, 10
    got = {}
    for seg in (64, 0):
        monkeypatch.setenv("NPB_ARENA_SEGMENT", str(seg))
        env = _make(n=192)
        assert int(env.L.npb_state_arena_segment(env._h)) == seg
        _stagger(env)
        env.enable_event_windows(COLUMNS, [("prim.sim_time", ">", X), (("pump.oil_level", 0), "<", 60.0)], pre, post)
        values, clock, _ = _run(env, steps)
        want = eventwin.record(values, clock, np.stack([clock, values[:, 0]], axis=1), [(">", X), ("<", 60.0)], pre, post)
        assert set((want["plant"] // 64).tolist()) == {0, 1, 2}
        got[seg] = env.event_windows()
        eventwin.same(got[seg], want)
        env.close()
    eventwin.same(got[64], got[0])


# ---------------------------------------------------------------------------------------------------------------- 5
def test_overflow():
    """capacity 5, all 70 plants capturing on one step; then three plants scram and their records, after the drain, are complete"""
    from nuclear_sim_amd import _lib, eventwin
    pre, post, cap = 2, 1, 5
    env = _make()
    env.enable_event_windows(COLUMNS, [("prim.sim_time", ">", 12.5), ("trip", ALL_BITS)], pre, post, capacity=cap)
    flags = lambda obs, rew, done, info: [info["trip_flags"]]
    va, ca, fa = _run(env, 4, extra=flags)
    assert int(_np(env._ewin["cursor"])[0]) == N
    with pytest.raises(_lib.NpbError, match="65 dropped"):
        env.event_windows()
    first = env.event_windows(allow_overflow=True)
    vb, cb, fb = _run(env, 3, extra=flags, before=lambda t: _poke(env, [1, 64, 69]) if t == 4 else None, first=4)
    values, clock = np.concatenate([va, vb]), np.concatenate([ca, cb])
    tv = np.stack([clock, np.concatenate([fa, fb])[:, 0]], axis=1)
    want = eventwin.record(values, clock, tv, [(">", 12.5), ("bits", ALL_BITS)], pre, post)
    one = _select(want, want["step"] == 2)
    assert one["plant"].tolist() == list(range(N)) and np.all(one["step"] + one["n_post"] == 3)
    # exactly five stored, each of a plant of its own and each the whole record of that plant (which five is not defined)
    assert len(first["plant"]) == cap and len(set(first["plant"].tolist())) == cap
    eventwin.same(first, _select(one, first["plant"]))
    later = _select(want, want["step"] > 2)
    assert later["plant"].tolist() == [1, 64, 69] and np.all(later["trigger"] == 1) and np.all(later["step"] == 4)
    assert int(_np(env._ewin["cursor"])[0]) == 3
    eventwin.same(env.event_windows(), later)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_an_abandoned_capture_writes_no_record_and_the_next_window_starts_with_an_empty_ring():
    """every plant armed at step 2 (due at 5); behind step 3 one lane of each wave is restored: no record for them, and their clock,
    back at 0, passes the limit again at step 6 with two samples in the ring.  The columns in an order of the caller's"""
    from nuclear_sim_amd import eventwin
    pre, post, steps = 4, 3, 12
    env = _make(autoreset=True, max_episode_steps=100)
    columns = ["reward", ("pump.oil_level", 0), ("obs", 5), ("sg.tube_wall_temp", 1), ("info", "electrical_power")]
    env.enable_event_windows(columns, [("prim.sim_time", ">", 12.5)], pre, post)
    mask = np.zeros(N, dtype=np.uint8); mask[[5, 69]] = 1

    def before(t):
        if t == 4:
            env.restore(torch.as_tensor(mask))
    values, clock, index = _run(env, steps, extra=lambda obs, rew, done, info: [info["episode_index"]], before=before)
    values = values[:, [4, 0, 3, 1, 2]]
    assert np.array_equal(index[:, 0], np.outer(np.arange(steps) >= 4, mask))      # the restore began the masked plants' next episode
    want = eventwin.record(values, clock, clock.reshape(steps, 1, N), [(">", 12.5)], pre, post, episode_index=index[:, 0])
    kept = want["plant"][want["step"] == 2]
    assert kept.tolist() == [p for p in range(N) if not mask[p]]
    again = _select(want, want["step"] == 6)
    assert again["plant"].tolist() == [5, 69] and again["n_pre"].tolist() == [2, 2] and again["episode"].tolist() == [1, 1] and len(want["plant"]) == N
    got = env.event_windows()
    eventwin.same(got, want)
    env.close()


def test_clear_does_by_hand_what_the_episode_index_does():
    """no autoreset, so no episode index: clear_event_windows(mask) forgets the masked plants' history and drops their armed captures"""
    from nuclear_sim_amd import eventwin
    pre, post = 4, 3
    env = _make()
    env.enable_event_windows(COLUMNS, [("prim.sim_time", ">", 12.5), ("prim.sim_time", ">", 32.5)], pre, post)
    mask = np.zeros(N, dtype=np.uint8); mask[[0, 63, 64]] = 1
    values, clock, _ = _run(env, 10, before=lambda t: env.clear_event_windows(torch.as_tensor(mask)) if t == 4 else None)
    index = np.outer(np.arange(10) >= 4, mask)               # in numpy the clear is a restart of the masked plants before sample 4
    want = eventwin.record(values, clock, np.stack([clock, clock], axis=1), [(">", 12.5), (">", 32.5)], pre, post, episode_index=index)
    want["episode"][:] = 0                                    # the handle carries no index
    assert np.sum(want["step"] == 2) == N - 3 and np.sum(want["step"] == 6) == N and set(want["step"].tolist()) == {2, 6}
    assert np.all(want["n_pre"][(want["step"] == 6) & (mask[want["plant"]] == 1)] == 2) and np.all(want["trigger"][want["step"] == 6] == 1)
    eventwin.same(env.event_windows(), want)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_off_means_off():
    """the same 30-step run with the windows on, never on, and switched off again: state, outputs and episode records by bits; the ring's
    memory goes back to the device when the windows are switched off"""
    L, steps = 12, 30
    outs = {}
    for which in ("never", "on", "off_again"):
        env = _make(autoreset=True, max_episode_steps=L)
        env.enable_episode_records()
        if which != "never":
            env.enable_event_windows(COLUMNS, [("trip", ALL_BITS), ("done",), ("prim.sim_time", ">", 27.5)], 4, 3)
        if which == "off_again":
            env.enable_event_windows(None)
            assert env._ewin is None
        per_step = []
        for t in range(steps):
            if t == 7:
                _poke(env, [3, 66])
            obs, rew, done, info = env.step(power_setpoint=_setpoint(t, N))
            per_step.append(torch.cat([obs.flatten(), rew, done.to(torch.float64), info["trip_flags"].to(torch.float64), info["electrical_power"],
                                       info["episode_length"].to(torch.float64)]).clone())
        f64, i32 = env.state_arrays()
        rec = env.episode_records()
        outs[which] = (_np(torch.stack(per_step)), _np(f64), _np(i32), rec)
        if which == "on":
            assert len(env.event_windows()["plant"]) > N
        env.close()
    for which in ("on", "off_again"):
        a, b = outs[which], outs["never"]
        assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64)), which
        assert np.array_equal(a[2], b[2]) and sorted(a[3]) == sorted(b[3]), which
        for k in b[3]:
            x, y = a[3][k], b[3][k]
            assert np.array_equal(x.view(np.int64), y.view(np.int64)) if x.dtype == np.float64 else np.array_equal(x, y), (which, k)
    # a ring of 1024 rows of 16 + 1 columns: 9.7 MB of the handle's own, given back by enable_event_windows(None)
    env = _make()
    cols = [("pump.oil_level", k) for k in range(3)] + [("obs", k) for k in range(12)] + ["reward"]
    env.enable_event_windows(cols, [("done",)], 600, 423, capacity=2)
    size = env._ewin["bytes"]
    assert size >= 1024 * 17 * N * 8 and size == int(env.L.npb_event_windows_bytes(ctypes.byref(env._ewin["desc"]), N))
    env.step(power_setpoint=_setpoint(0, N))
    torch.cuda.synchronize(env.device)
    held = torch.cuda.mem_get_info(env.device)[0]
    env.enable_event_windows(None)
    freed = torch.cuda.mem_get_info(env.device)[0] - held
    assert freed >= size // 2, (freed, size)
    env.step(power_setpoint=_setpoint(1, N))
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_a_second_set_replaces_the_first_and_clear_without_windows_is_refused(tmp_path):
    from nuclear_sim_amd import _lib, eventwin
    env = _make()
    assert env.L.npb_event_windows_clear(env._h, None, None) == -1        # NPB_EINVAL
    assert b"no event windows set" in env.L.npb_last_error(env._h)
    with pytest.raises(_lib.NpbError, match="enable_event_windows"):
        env.clear_event_windows()
    with pytest.raises(_lib.NpbError, match="enable_event_windows"):
        env.event_windows()
    with pytest.raises(ValueError, match="enable_maintenance_summary"):
        env.enable_event_windows(COLUMNS, [("work_order", 0)], 2, 2)
    env.enable_event_windows(COLUMNS, [("prim.sim_time", ">", 12.5)], 4, 3)
    old = env._ewin                                                          # kept alive: the first set's record columns
    va, ca, _ = _run(env, 3)                                                 # armed at step 2, due at 5
    # another shape, other columns, another trigger: the sample count starts at 0 again and the armed captures of the first set are gone
    columns = ["reward", ("pump.oil_level", 1)]
    env.enable_event_windows(columns, [("prim.sim_time", ">", 32.5)], 1, 2, capacity=N + 1)
    vb, cb, _ = _run(env, 7, members=[("pump.oil_level", 1)], first=3)
    want = eventwin.record(vb[:, [3, 0]], cb, cb.reshape(7, 1, N), [(">", 32.5)], 1, 2)
    assert want["step"].tolist() == [3] * N and want["n_pre"].tolist() == [1] * N          # steps 3 .. 9 are the second set's samples 0 .. 6
    # the table: one column per (row offset, recorded column), the offsets -pre .. post as m<k> / p<k>
    import pyarrow.parquet as pq
    env.write_event_windows(str(tmp_path / "w.parquet"), clear=False)
    t = pq.read_table(str(tmp_path / "w.parquet")).to_pydict()
    assert t["plant"] == list(range(N)) and t["early"] == [False] * N and "values" not in t and "times" not in t
    assert [k for k in t if k.startswith(("time_", "c0_", "c1_"))] == ["time_m1", "c0_m1", "c1_m1", "time_p0", "c0_p0", "c1_p0", "time_p1", "c0_p1", "c1_p1",
                                                                        "time_p2", "c0_p2", "c1_p2"]
    assert t["time_p0"] == want["time"].tolist() and t["c1_m1"] == want["values"][:, 0, 1].tolist() and t["c0_p2"] == want["values"][:, 3, 0].tolist()
    eventwin.same(env.event_windows(), want)
    assert int(_np(old["cursor"])[0]) == 0 and not _np(old["dev"]["values"]).any()          # the first set's columns were never written
    # a descriptor the library refuses leaves the windows as they are
    bad = _lib.NpbEventWindowsDesc.from_buffer_copy(env._ewin["desc"])
    bad.capacity = 0
    assert env.L.npb_set_event_windows(env._h, ctypes.byref(bad)) == -1 and b"capacity" in env.L.npb_last_error(env._h)
    vc, cc, _ = _run(env, 1, members=[("pump.oil_level", 1)], first=10)
    assert len(env.event_windows()["plant"]) == 0
    env.enable_event_windows(None)
    assert env.L.npb_event_windows_clear(env._h, None, None) == -1
    env.close()
