"""GPU: caller-defined policy inputs kept on the device (npb_set_features, BatchedPlantEnv.set_features).

The reference is nuclear_sim_amd.features, the numpy statement, over the rows the features read, read back through the EXISTING field and
buffer paths (env.features_samples: npb_get_field and the step's own output tensors).  Differences, products, comparisons, a narrowing and
copies: the stacks match by bits (view(int32) / view(int64)), with no tolerance anywhere.

The run is the task suite's: BatchedPlantEnv.action_test("oil_top_off", seeds=range(n), dt=5.0), every plant with a setpoint of its own,
at most 24 steps, and its pokes before a step: a fuel temperature of 1500 (the plant scrams on that step), a pump oil level of 4 (the pump
trips) and an infinite ``mpump.last_violation_time`` stamp, here read with itself as the second column, so the sample is inf - inf.

Where episodes restart on the device the terminal samples are gone by the time the step returns.  The reference then comes from a TWIN
without autoreset that is stepped and poked alike and restored by hand (restore(mask) / restore_from_bank(mask)) for the plants whose
episodes ended: its rows before the restore are the terminal samples, its rows behind it the fresh ones.  Every step first asserts that the
twin's observation is the env's, bit for bit, so a twin that strayed is reported as that.

Clip limits are medians over the plants of a dry twin run at a middle step (computed once and shared), so some plants clip and some do
not.  Every test asserts that what it claims to cover happened on some plant and not on another."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, N3, DT, STEPS, MID = 70, 130, 5.0, 12, 6
KERNEL_OF_VARIANT = {1: "npb_step_maint_kernel", 2: "npb_step2_wide_maint_kernel", 5: "npb_step4_maint_kernel"}
PUMP_TRIPS = 0xF00                                  # NPB_TRIP_FW_PUMP0 .. 3
STAMP = ("mpump.last_violation_time", 3, 15)
# before step t: {what: plants}; plants past the batch are left out
POKES = {2: {"stamp": [0, 11, 69, 128]}, 3: {"fuel": [5, 100]}, 4: {"oil": [0, 9, 64, 129]}, 9: {"fuel": [66]}}


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(a):
    """the bit patterns of a float tensor or array, as numpy integers"""
    a = np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _tbits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(got, want, where):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (where, g.shape, w.shape)
    assert np.array_equal(g, w), (where, np.argwhere(g != w)[:4].tolist())


def _make(n=N, **kw):
    from nuclear_sim_amd.env import BatchedPlantEnv
    return BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, **kw)


def _setpoint(t, n):
    return 90.0 + 8.0 * np.sin(2.0 * np.pi * t / (20.0 + np.arange(n) % 7))


def _set(env, name, plants, value, instance=0, k=0):
    plants = [p for p in plants if p < env.n]
    if plants:
        v = _np(env.get_field(name, instance, k))
        v[plants] = value
        env.set_field(name, v, instance, k)


def _poke(env, t, pokes=POKES):
    for what, plants in pokes.get(t, {}).items():
        if what == "fuel":
            _set(env, "prim.fuel_temperature", plants, 1500.0)
        elif what == "oil":
            _set(env, "pump.oil_level", plants, 4.0, 0)
        else:
            _set(env, STAMP[0], plants, np.inf, STAMP[1], STAMP[2])


@functools.lru_cache(maxsize=None)
def _dry():
    """the twin WITHOUT features, stepped and poked as the tests step and poke: per step obs, reward, done and the whole state (on the
    device), and the limits -- medians over the plants at step MID.  Computed once, never written"""
    env = _make()
    out = {"reward": [], "done": [], "obs": [], "f64": [], "i32": []}
    for t in range(STEPS):
        _poke(env, t)
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, N))
        f, i = env.state_arrays()
        for name, x in (("reward", rew), ("done", done), ("obs", obs), ("f64", f), ("i32", i)):
            out[name].append(x.clone())
        if t == MID:
            out["limits"] = {c: float(np.median(_np(env.get_field(*c)))) for c in (("pump.oil_level", 0), ("pump.oil_level", 1), ("sg.tube_wall_temp", 1))}
            out["power"] = float(np.median(_np(info["electrical_power"])))
    env.close()
    return out


def _columns(C):
    """C columns: first the ones with something to prove -- members carried and output, info, obs, reward, integer columns with BITS, second
    columns, NaNs replaced and kept, clips on either side, a value in float32's subnormal range -- then plain ones up to 64"""
    from nuclear_sim_amd.env import INFO_COLUMNS
    from nuclear_sim_amd.schema import SCHEMA
    lim, power = _dry()["limits"], _dry()["power"]
    cols = [(("pump.oil_level", 0), {"ref": lim[("pump.oil_level", 0)], "scale": 0.5, "clip": (None, 0.0)}),       # 0 carried member, clipped above
            ("flags", {"bits": PUMP_TRIPS, "fresh": 0x100}),                                                          # 1 BITS on an integer side
            (("obs", 5), {"ref": ("obs", 6), "scale": 3.0}),                                                          # 2 a second column, both live
            (STAMP, {"ref": STAMP, "nan_to": -1.0}),                                                                  # 3 inf - inf, replaced
            (("info", "electrical_power"), {"ref": power, "scale": 0.001, "clip": (-0.02, 0.02), "fresh": power}),   # 4 info, clipped on both sides
            (STAMP, {"ref": STAMP, "clip": (-1.0, 1.0)}),                                                             # 5 inf - inf, kept: it passes the clip
            (("sg.tube_wall_temp", 1), {"clip": (lim[("sg.tube_wall_temp", 1)], None)}),                              # 6 output member, clipped below
            ("reward", {"scale": 2.0, "fresh": 3.0}),                                                                 # 7 the step's reward
            (("pump.oil_level", 1), {"scale": 2.0 ** -140}),                                                          # 8 float32 subnormals
            ("maintenance", {"scale": 0.25}),                                                                         # 9 an int32 member
            ("done", {"bits": 0xFF}),                                                                                 # 10 BITS on a uint8 side
            ("reward", {"ref": ("pump.oil_level", 1), "ref_fresh": 1.0}),                                             # 11 a side against a member
            (("pump.status", 0), {"bits": 1}),                                                                        # 12 BITS on an int32 member
            ("pump.vibration_level", {"ref": ("info", "steam_flow"), "ref_fresh": 2.0, "scale": 1e300})]              # 13 overflows float32
    pad = [("info", name) for name in INFO_COLUMNS] + [("obs", i) for i in range(22)]
    pad += [name for name in SCHEMA.by_name if name.startswith(("prim.", "sec.", "sg.")) and SCHEMA.slot(name)[0] == "f64"]
    for j, word in enumerate(pad):
        cols.append((word, {"scale": 0.5, "ref": 1.0}) if j % 3 == 0 else word)
    return cols[:C]


class _Coverage:
    """what happened on some plant and not on another, over the newest frames of a run ([n, C] float64 views of the reference)"""
    CHECKS = {0: ("clipped above", lambda y: y == 0.0), 1: ("a pump tripped", lambda y: y == 1.0), 3: ("a NaN replaced", lambda y: y == -1.0),
              4: ("clipped on either side", lambda y: (np.abs(y) == 0.02) | (np.abs(y) == np.float32(0.02))), 5: ("a NaN kept", np.isnan),
              8: ("a float32 subnormal", lambda y: (y != 0.0) & (np.abs(y) < 2.0 ** -126)), 10: ("a scram", lambda y: y == 1.0)}

    def __init__(self, C, dtype):
        self.hit, self.miss = {}, {}
        self.checks = {c: v for c, v in self.CHECKS.items() if c < C and not (c == 8 and dtype == torch.float64)}

    def add(self, frames):
        for c, (_what, test) in self.checks.items():
            m = test(frames[:, c].astype(np.float64))
            self.hit[c] = self.hit.get(c, False) or bool(m.any())
            self.miss[c] = self.miss.get(c, False) or bool((~m).any())

    def check(self, n):
        for c, (what, _test) in self.checks.items():
            assert self.hit[c], "column %d: never %s" % (c, what)
            assert self.miss[c] or n == 1 or c == 8, "column %d: %s everywhere" % (c, what)      # (column 8 is subnormal on every plant, by its scale)


def _reference(env, final=False, final_fill=0):
    from nuclear_sim_amd import features
    return features.Stack(env.features_spec()["spec"], env.n, final=final, final_fill=final_fill)


# ---------------------------------------------------------------------------------------------------------------- 1
CASES = [(1, "f64", N, 5, 4, torch.float32, False), (2, "f64", N3, 64, 4, torch.float32, True), (5, "f64", N, 32, 8, torch.float64, False),
         (2, "f32", N3, 5, 4, torch.float64, True), (5, "f64", 1, 1, 1, torch.float32, True), (1, "f64", 1, 64, 4, torch.float64, False),
         (5, "f32", N, 64, 4, torch.float32, False), (2, "f64", N, 1, 1, torch.float64, False), (1, "f32", N3, 32, 8, torch.float32, True),
         (5, "f64", N3, 14, 3, torch.float64, True)]


@pytest.mark.parametrize("variant, storage, n, C, K, dtype, prime", CASES)
def test_bit_for_bit_with_the_numpy_statement(variant, storage, n, C, K, dtype, prime):
    """Per step the rows the features read are read back and fed to features.Stack; the device's stack is its bits.  ``prime``: the stack
    is first asked for before any step (the fresh frame), else the first step fills it.  Fails without the feature: set_features does not
    exist"""
    env = _make(n, storage=storage)
    env.set_step_kernel(variant)
    env.set_features(_columns(C), stack=K, dtype=dtype)
    ref, cover = _reference(env), _Coverage(C, dtype)
    assert env.features_spec()["spec"]["stack"] == K and len(env.features_spec()["spec"]["columns"]) == C
    if prime:
        got = env.features()
        assert got.shape == (n, K, C) and got.dtype == dtype and got.is_contiguous()
        assert ref.prime(_np(env.features_samples())).all()
        _same(got, ref.out, "primed")
    for t in range(STEPS):
        _poke(env, t)
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, n))
        fill = ref.step(_np(env.features_samples()))
        assert bool(fill.all()) == (t == 0 and not prime) and bool(fill.any()) == (t == 0 and not prime), t
        assert info["features"].data_ptr() == env.features().data_ptr() and "final_features" not in info
        _same(info["features"], ref.out, t)
        cover.add(ref.out[:, -1])
    if n > 1:
        assert env.last_step_kernel() == KERNEL_OF_VARIANT[variant], env.last_step_kernel()
    if n >= N and C >= 14:
        cover.check(n)
        assert np.isinf(ref.out[:, -1, 13]).any() == (dtype == torch.float32)          # 1e300 x: beyond float32, within float64
    elif n >= N and C >= 5:
        cover.check(n)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2, 3
def _run_with_restarts(env, twin, L, steps, pokes, restore):
    """env restarts its episodes on the device, the twin is restored by hand; the reference stack follows the twin.  Returns per step the
    plants that restarted"""
    n, K = env.n, env.features_spec()["spec"]["stack"]
    sentinel = -(1000.0 + np.arange(n * K * len(env.features_spec()["spec"]["columns"]))).reshape(env.final_features().shape)
    env.final_features().copy_(torch.as_tensor(sentinel).to(env.final_features()))
    ref = _reference(twin, final=True)
    ref.final[:] = sentinel
    index, length, restarts = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64), []
    for t in range(steps):
        _poke(env, t, pokes); _poke(twin, t, pokes)
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, n))
        t_obs, t_rew, t_done, t_info = twin.step(power_setpoint=_setpoint(t, n))
        t_obs_step = t_obs.clone()
        assert torch.equal(_tbits(rew), _tbits(t_rew)) and torch.equal(done, t_done), ("the twin strayed", t)
        ref.step(_np(twin.features_samples()), index)
        _same(t_info["features"], ref.out, ("the twin, without autoreset", t))
        length += 1
        ended = (_np(t_done) != 0) | (length >= L)
        assert np.array_equal(ended, (_np(done) != 0) | (_np(info["truncated"]) != 0)), t
        if ended.any():
            restore(twin, torch.as_tensor(ended))
        during = index.copy()
        index[ended] += 1; length[ended] = 0
        now = torch.as_tensor(ended, device=obs.device)      # the rows the episode kernel rewrote against the restored twin's; the others against its step
        assert torch.equal(_tbits(obs[now]), _tbits(twin.get_observation()[now])) and torch.equal(_tbits(obs[~now]), _tbits(t_obs_step[~now])), ("the twin strayed", t)
        assert np.array_equal(_np(info["episode_index"]), during), t      # (the index of the episode the transition belonged to)
        got = ref.restart(_np(twin.features_samples()), index)
        assert np.array_equal(got, ended), t
        _same(info["features"], ref.out, t)
        _same(info["final_features"], ref.final, ("final", t))
        assert info["final_features"].data_ptr() == env.final_features().data_ptr()
        st = env.features_state()
        assert np.array_equal(st["seen"], index) and st["primed"].all(), t
        restarts.append(np.flatnonzero(ended))
    return ref, restarts, sentinel


def test_autoreset_from_the_snapshot_restarts_the_stacks():
    """max_episode_steps 3 and scram pokes: plants restart on most steps, different ones.  Their stacks are K copies of the fresh frame,
    side columns at their fresh values; final_features holds the stacks that ended, terminal frame included, and the sentinel elsewhere"""
    from nuclear_sim_amd import features
    L, steps, K = 3, 10, 4
    pokes = {1: {"fuel": [5, 66]}, 3: {"fuel": [9], "stamp": [11, 69]}, 4: {"oil": [0, 64]}}
    cols = _columns(14)
    env, twin = _make(autoreset=True, max_episode_steps=L), _make()
    twin.snapshot()
    for e in (env, twin):
        e.set_features(cols, stack=K, final=True)
    ref, restarts, sentinel = _run_with_restarts(env, twin, L, steps, pokes, lambda e, m: e.restore(m))
    assert [r.tolist() for r in restarts[:3]] == [[], [5, 66], [p for p in range(N) if p not in (5, 66)]]
    assert sum(len(r) > 0 for r in restarts) >= 6 and all(len(r) < N for r in restarts)
    # the last restart: K copies of one frame, side columns at their fresh values through the transform, members live
    out, last = _np(env.features()), restarts[-1]
    assert len(last) and len(last) < N
    spec = env.features_spec()["spec"]
    fresh = features.frame(np.zeros((len(env.features_spec()["columns"]), 1)), spec, fresh=True)[0]
    for p in last:
        assert all(np.array_equal(_bits(out[p, k]), _bits(out[p, 0])) for k in range(K)), p
        assert out[p, 0, 1] == 1.0 and out[p, 0, 7] == 6.0 and out[p, 0, 4] == 0.0 and out[p, 0, 10] == 0.0, p      # flags 0x100 & 0xF00; 3.0 * 2; power - power; done 0
        assert np.array_equal(_bits(out[p, 0, [1, 4, 7, 10]]), _bits(fresh[[1, 4, 7, 10]])), p
        assert out[p, 0, 0] != fresh[0] and out[p, 0, 8] != 0.0, p                                                    # live members
    others = [p for p in range(N) if p not in last]
    assert any(not np.array_equal(out[p, 0], out[p, K - 1]) for p in others)
    # final: a plant that restarted holds a terminal stack (no sentinel left), one that never did holds the sentinel -- none here: every
    # plant was truncated; the ones whose last restart is long ago keep that terminal stack though others restarted since
    fin = _np(env.final_features())
    assert not np.any(fin == sentinel.astype(np.float32))
    env.close(); twin.close()


def test_autoreset_from_a_start_bank_with_a_task_ending_the_episodes():
    """the episodes end by the task's rules (an oil-level limit, the scram pulse) or by max_episode_steps, and restart from bank entries;
    the features read the task's reward too.  Some plants never restart within the run: their final rows keep the sentinel"""
    L, steps, K = 6, 8, 3
    pokes = {2: {"fuel": [5]}, 3: {"oil": [9, 64]}}
    lim = _dry()["limits"][("pump.oil_level", 1)]
    task = dict(reward=[("reward", 1.0), (("pump.oil_level", 0), -0.25, "beyond", "<", 10.0)], terminate=[("done", -100.0), (("pump.oil_level", 0), "<", 10.0, -7.0)])
    cols = _columns(5) + [("task_reward", {"scale": 0.5, "fresh": -1.0}), ("obs", 3)]
    env, twin = _make(autoreset=True, max_episode_steps=L, bank_seeds=range(100, 110)), _make(bank_seeds=range(100, 110))
    for e in (env, twin):
        e.set_task(**task)
        e.set_features(cols, stack=K, dtype=torch.float64, final=True)
    ref, restarts, sentinel = _run_with_restarts(env, twin, L, steps, pokes, lambda e, m: e.restore_from_bank(m))
    assert restarts[2].tolist() == [5] and restarts[3].tolist() == [9, 64] and len(restarts[5]) == N - 3
    fin, out = _np(env.final_features()), _np(env.features())
    assert np.all(fin[5] != sentinel[5]) and np.all(fin[9] != sentinel[9])
    assert out[5, -1, 5] != -0.5 and out[restarts[5][0], 0, 5] == -0.5                 # task_reward: live since, fresh in the restart frame still in the stack
    with pytest.raises(Exception, match="features"):
        env.set_task(None)                                                              # the features hold the task's reward column
    env.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_without_autoreset_resets_restores_and_clears_refill_only_the_masked_plants():
    cols, K = _columns(14), 4
    env = _make()
    env.snapshot()
    env.set_features(cols, stack=K)
    ref = _reference(env)
    got = env.features()                                   # before the first step: the fresh frame
    assert ref.prime(_np(env.features_samples())).all()
    _same(got, ref.out, "before the first step")
    assert np.all(_np(got)[:, :, 7] == 6.0) and np.array_equal(_np(got)[:, 0], _np(got)[:, K - 1])

    def step(t):
        _poke(env, t)
        env.step(power_setpoint=_setpoint(t, N))
        fill = ref.step(_np(env.features_samples()))
        _same(env.features(), ref.out, t)
        return fill
    for t in range(3):
        assert not step(t).any()
    before = _np(env.features())
    for k, (what, mask) in enumerate((("reset", np.arange(N) % 3 == 0), ("restore", np.arange(N) % 5 == 1))):
        getattr(env, what)(torch.as_tensor(mask))
        ref.clear(mask)
        assert np.array_equal(ref.prime(_np(env.features_samples())), mask)
        got = _np(env.features())
        _same(got, ref.out, what)
        assert np.array_equal(_bits(got[~mask]), _bits(before[~mask])), what                  # only the masked plants
        assert all(np.array_equal(_bits(got[p, 0]), _bits(got[p, K - 1])) for p in np.flatnonzero(mask)) and np.all(got[mask][:, :, 7] == 6.0)
        assert not np.array_equal(_bits(got[mask]), _bits(before[mask]))
        assert not step(3 + k).any()                                                           # primed again: they shift
        before = _np(env.features())
    mask = np.arange(N) % 7 == 2
    env.clear_features(torch.as_tensor(mask))
    ref.clear(mask)
    _poke(env, 5)
    env.step(power_setpoint=_setpoint(5, N))                                                   # cleared, then a step: fills, does not shift
    assert np.array_equal(ref.step(_np(env.features_samples())), mask)
    got = _np(env.features())
    _same(got, ref.out, "cleared")
    assert all(np.array_equal(_bits(got[p, 0]), _bits(got[p, K - 1])) for p in np.flatnonzero(mask))
    assert np.array_equal(_bits(got[~mask][:, :-1]), _bits(before[~mask][:, 1:]))              # the others shifted
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_a_callers_restore_between_two_steps_with_autoreset_on_fills():
    """npb_restore bumps the carried episode index: pass A sees it differ from the one seen and fills; nothing ended, so pass B is idle
    and the final rows keep their sentinel"""
    cols, K = _columns(14), 4
    env = _make(autoreset=True)
    env.set_features(cols, stack=K)
    env.final_features().fill_(-5.0)
    ref = _reference(env)
    index = np.zeros(N, dtype=np.int32)
    for t in range(3):
        env.step(power_setpoint=_setpoint(t, N))
        ref.step(_np(env.features_samples()), index)
    mask = np.arange(N) % 4 == 1
    m = torch.as_tensor(mask).to(device=env.device, dtype=torch.uint8)
    assert env.L.npb_restore(env._h, ctypes.c_void_p(m.data_ptr()), env._stream()) == 0       # the C entry point: the env's own restore would refill
    index[mask] += 1
    for t in range(3, 5):
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, N))
        assert not bool(done.any()) and not bool(info["truncated"].any()) and np.array_equal(_np(info["episode_index"]), index)
        fill = ref.step(_np(env.features_samples()), index)
        assert np.array_equal(fill, mask if t == 3 else np.zeros(N, dtype=bool)), t
        _same(info["features"], ref.out, t)
    assert bool((env.final_features() == -5.0).all())
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_segmented_arena():
    """45 120 plants, the smallest segmented handle: every plant with an oil level and a setpoint of its own, against the statement on all"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 45120
    env = BatchedPlantEnv(n, dt=DT)
    assert env.L.npb_state_arena_segment(env._h) > 0
    env.set_field("pump.oil_level", 60.0 + 30.0 * (np.arange(n) % 997) / 997.0, 1)
    env.set_features([(("pump.oil_level", 1), {"ref": 75.0, "scale": 0.1, "clip": (-1.0, 1.0)}), ("info", "thermal_power"),
                      (("obs", 5), {"ref": ("obs", 6)}), ("flags", {"bits": 0xFFFF})], stack=2)
    ref = _reference(env)
    got = env.features()
    ref.prime(_np(env.features_samples()))
    _same(got, ref.out, "primed")
    for t in range(3):
        env.step(power_setpoint=90.0 + 8.0 * np.sin(np.arange(n) * 0.001 + t))
        ref.step(_np(env.features_samples()))
        _same(env.features(), ref.out, t)
    y = ref.out[:, -1, 0]
    assert (y == 1.0).any() and (y == -1.0).any() and ((y > -1.0) & (y < 1.0)).any()
    assert len(np.unique(y)) > 100                                          # a value of its own per plant, up to the clip
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_checkpoint():
    """stop after 5 steps, save state_arrays, features_state and the stack, load them into a NEW env: the remaining steps' features are
    the uninterrupted run's"""
    steps, at, cols, K = 10, 5, _columns(14), 4
    z = np.random.default_rng(7).standard_normal((steps, N))

    def run(env, first, last):
        out = []
        for t in range(first, last):
            _poke(env, t)
            env.step(power_setpoint=_setpoint(t, N), noise_z=z[t])
            out.append(env.features().clone())
        return torch.stack(out)
    a = _make()
    a.set_features(cols, stack=K)
    run(a, 0, at)
    f, i = a.state_arrays()
    state, stack = a.features_state(), _np(a.features())
    assert state["primed"].all() and not state["seen"].any()
    rest = run(a, at, steps)
    b = _make()
    b.set_features(cols, stack=K)
    b.load_state_arrays(f, i)
    b.load_features_state(state, stack)
    assert torch.equal(_tbits(run(b, at, steps)), _tbits(rest))
    c = _make()                                        # ... and without the features' own state the first frame fills
    c.set_features(cols, stack=K)
    c.load_state_arrays(f, i)
    first = run(c, at, at + 1)[0]
    assert torch.equal(_tbits(first[:, -1]), _tbits(rest[0][:, -1])) and not torch.equal(_tbits(first[:, 0]), _tbits(rest[0][:, 0]))
    for e in (a, b, c):
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_lifecycle_of_the_features():
    from nuclear_sim_amd import _lib
    dry = _dry()
    env = _make()
    _poke(env, 0)
    obs, rew, done, info = env.step(power_setpoint=_setpoint(0, N))
    assert "features" not in info and obs.shape == (N, 22)
    with pytest.raises(_lib.NpbError, match="no features"):
        env.features()
    env.set_features(_columns(5), stack=4)
    _poke(env, 1)
    obs, rew, done, info = env.step(power_setpoint=_setpoint(1, N))
    assert info["features"].shape == (N, 4, 5) and obs.shape == (N, 22) and "observation" not in info
    env.set_features(_columns(32), stack=8, dtype=torch.float64, as_observation=True)          # again, another shape
    ref = _reference(env)
    _poke(env, 2)
    obs, rew, done, info = env.step(power_setpoint=_setpoint(2, N))
    assert ref.step(_np(env.features_samples())).all()                                          # every plant unprimed by the new set
    assert obs.shape == (N, 8, 32) and obs.dtype == torch.float64 and obs.data_ptr() == info["features"].data_ptr()
    _same(obs, ref.out, "as_observation")
    assert torch.equal(_tbits(info["observation"]), _tbits(dry["obs"][2]))
    # refusals of the library surface as NpbError with the reason, and leave what was set
    d = _lib.NpbFeaturesDesc()
    col = (_lib.NpbFeatureColumn * 1)()
    col[0].column.kind, col[0].column.slot, col[0].scale, col[0].lo, col[0].hi = 0, 0, 1.0, -np.inf, np.inf
    d.n_columns, d.columns, d.stack, d.out_type, d.out = 1, col, 1, 0, None
    with pytest.raises(_lib.NpbError, match="a NULL out tensor"):
        _lib.check(env.L.npb_set_features(env._h, ctypes.byref(d)), env._h)
    d.out, d.stack = env.features().data_ptr(), 17
    with pytest.raises(_lib.NpbError, match="stack depth must be 1 .. NPB_FEATURES_STACK_MAX"):
        _lib.check(env.L.npb_set_features(env._h, ctypes.byref(d)), env._h)
    with pytest.raises(ValueError, match="unknown column"):
        env.set_features(["no.such_member"])
    _poke(env, 3)
    obs, rew, done, info = env.step(power_setpoint=_setpoint(3, N))
    assert not ref.step(_np(env.features_samples())).any()
    _same(obs, ref.out, "after the refusals")
    env.set_features(None)                                                                      # off: step()'s return and info keys are back
    for t in range(4, 6):
        _poke(env, t)
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, N))
        assert "features" not in info and "observation" not in info and "final_features" not in info and obs.shape == (N, 22)
        assert torch.equal(_tbits(obs), _tbits(dry["obs"][t])) and torch.equal(_tbits(rew), _tbits(dry["reward"][t]))
    for name, args in (("npb_features_prime", (None,)), ("npb_features_clear", (None, None)), ("npb_features_get_state", (None, None, None)),
                       ("npb_features_set_state", (None, None, None))):
        assert getattr(env.L, name)(env._h, *args) == -1 and b"no features set" in env.L.npb_last_error(env._h), name
    with pytest.raises(_lib.NpbError, match="no features"):
        env.features_state()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 9
def test_off_is_off():
    """a run with features never set (the dry twin) and one where they were set and then dropped: obs, reward, done and the whole state
    are identical at every step, also while they were on"""
    dry = _dry()
    env = _make(autoreset=False)
    for t in range(STEPS):
        if t == 2:
            env.set_features(_columns(64), stack=4)
        if t == 7:
            env.set_features(None)
        _poke(env, t)
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, N))
        assert ("features" in info) == (2 <= t < 7), t
        assert torch.equal(_tbits(obs), _tbits(dry["obs"][t])) and torch.equal(_tbits(rew), _tbits(dry["reward"][t])) and torch.equal(done, dry["done"][t]), t
        f, i = env.state_arrays()
        assert torch.equal(_tbits(f), _tbits(dry["f64"][t])) and torch.equal(i, dry["i32"][t]), t
    env.close()
