"""GPU: caller-defined policy outputs decoded on the device in front of the step (npb_set_controls, BatchedPlantEnv.set_controls).

The reference is nuclear_sim_amd.controls.Decoder, the numpy statement, and a TWIN: an env without controls in the same state that
receives the Decoder's new members through set_field and the Decoder's columns through step(power_setpoint=..., cooling_water_temp=...).
After every step the observation, the reward, done, the info columns, the trip flags and the whole state of the two are compared by bits,
and the device's held / prev with the Decoder's, with no tolerance anywhere.

The inputs are drawn per plant and step, so the plants diverge, with the special values a branch needs placed on fixed plants: a NaN, a
value inside the deadband, an exact zero, at step 0 the position itself (TARGET equal; the start positions are float32 values so that a
float32 input can name them).  A quarter of the plants start just below each actuator's upper limit and a quarter just above the lower
one, so that rates run into both clamps and targets outside the range land on the limit.

Coverage is a condition: from the Decoder's branch report every case with n >= 130 asserts that every branch of every axis it has was
entered on some plant -- per RATE axis up, down, zero, the deadband, both range clamps; per TARGET axis reached, not reached, equal, out
of range; on every axis a NaN input, both clip ends, a latching step and, with an interval above 1, a held one.  (A single plant cannot
enter them all in 12 steps: the cases with n = 1 compare bits only.)  Four actuators and two inputs, each named at most once, make six
axes; the cases with eight add two VALUE axes.  Over the two layouts every actuator is moved as a RATE and as a TARGET."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N3, NSEG, DT, STEPS = 130, 45120, 5.0, 12
KERNEL_OF_VARIANT = {1: "npb_step_maint_kernel", 2: "npb_step2_wide_maint_kernel", 5: "npb_step4_maint_kernel"}


def _np(t):
    return t.detach().cpu().numpy().copy()


def _tbits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64) if t.is_floating_point() else t


def _same_np(got, want, where):
    g = np.ascontiguousarray(_np(got) if isinstance(got, torch.Tensor) else got, dtype=np.float64).view(np.int64)
    w = np.ascontiguousarray(want, dtype=np.float64).view(np.int64)
    assert g.shape == w.shape, (where, g.shape, w.shape)
    assert np.array_equal(g, w), (where, np.argwhere(g != w)[:4].tolist())


def _make(n, **kw):
    from nuclear_sim_amd.env import BatchedPlantEnv
    if n >= NSEG:      # a segmented arena: the plain env (a scenario per plant is host work)
        env = BatchedPlantEnv(n, dt=DT, storage=kw.pop("storage", "f64"), **kw)
        assert env.L.npb_state_arena_segment(env._h) > 0
        return env
    return BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, **kw)


def _setpoint(t, n):
    return 90.0 + 8.0 * np.sin(2.0 * np.pi * t / (20.0 + np.arange(n) % 7))


def _axes(A, layout=0):
    """the axes of a case: A = 1 one rod RATE; A = 3 a TARGET, a RATE and a COLUMN; A = 8 all four actuators (layout 0: rod and flow RATE,
    valve and boron TARGET; layout 1 the other way round), both columns and two VALUE axes"""
    from nuclear_sim_amd import controls
    span = {a: controls.RANGES[a][1] - controls.RANGES[a][0] for a in controls.ACTUATORS}

    def rate(a):
        return (a, "rate", {"scale": 1.25, "offset": 0.0625, "deadband": 0.05, "nan_to": -0.5})

    def target(a):
        lo, hi = controls.RANGES[a]
        return (a, "target", {"clip": (lo - 0.1 * span[a], hi + 0.1 * span[a]), "max_magnitude": 0.25, "nan_to": 0.5 * (lo + hi)})
    setpoint = ("power_setpoint", "column", {"scale": 10.0, "offset": 90.0, "clip": (82.0, 99.0), "nan_to": 0.25})
    cooling = ("cooling_water_temp", "column", {"scale": 4.0, "offset": 25.0, "clip": (20.0, 30.0)})
    if A == 1:
        return [rate("rod")]
    if A == 3:
        return [target("valve"), rate("flow"), setpoint]
    kinds = (rate, rate, target, target) if layout == 0 else (target, target, rate, rate)
    return [kinds[0]("rod"), kinds[1]("flow"), kinds[2]("valve"), kinds[3]("boron"), setpoint, cooling,
            (None, "value", {"scale": 2.0, "clip": (-1.0, 1.0)}), (None, "value")]


def _start(n):
    """the actuators' start positions, float32 values: a quarter of the plants just below the upper limit, a quarter just above the lower"""
    from nuclear_sim_amd import controls
    out, p = {}, np.arange(n)
    for a in controls.ACTUATORS:
        lo, hi = controls.RANGES[a]
        span = hi - lo
        pos = lo + span * (0.3 + 0.4 * ((p * 7) % 11) / 11.0)
        pos = np.where(p % 4 == 0, hi - span / 256.0, np.where(p % 4 == 1, lo + span / 256.0, pos))
        out[a] = pos.astype(np.float32).astype(np.float64)
    return out


def _put_start(env, start):
    from nuclear_sim_amd import controls
    for a, pos in start.items():
        env.set_field(controls.MEMBERS[a], pos)


def _inputs(spec, t, n, start, rng):
    """the policy's output of step t, [n, A] in the spec's dtype"""
    from nuclear_sim_amd import controls
    A, p = len(spec["axes"]), np.arange(n)
    x = np.empty((n, A))
    for a, D in enumerate(spec["axes"]):
        if D["kind"] == "target":
            lo, hi = controls.RANGES[D["target"]]
            x[:, a] = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), n)
            near = (p + t + a) % 5 == 0      # within one move of where the actuator is likely to be: around its start
            x[near, a] = start[D["target"]][near] + rng.uniform(-1.0, 1.0, near.sum()) * (hi - lo) / 512.0
            if t == 0:
                x[(p + a) % 16 == 6, a] = start[D["target"]][(p + a) % 16 == 6]      # the position itself
        else:
            x[:, a] = rng.uniform(-1.5, 1.5, n)
            x[(p + t + a) % 16 == 4, a] = -0.03      # (* 1.25 + 0.0625 = 0.025: inside a rate's deadband)
            x[(p + t + a) % 16 == 5, a] = -0.05      # (* 1.25 + 0.0625 = 0.0 exactly)
        x[(p + t + a) % 16 == 3, a] = np.nan
    return x.astype(np.dtype(spec["dtype"]))


def _wanted(spec):
    """per axis the branches its kind has: the coverage condition"""
    from nuclear_sim_amd import controls as c
    out = []
    for D in spec["axes"]:
        need = [c.LATCHED, c.UNPRIMED, c.NAN_IN, c.CLIP_LO, c.CLIP_HI] + ([c.HELD] if spec["interval"] > 1 else [])
        if D["kind"] == "rate":
            need += [c.RATE_UP, c.RATE_DOWN, c.RATE_ZERO, c.DEADBAND, c.LIMIT_HI, c.LIMIT_LO]
        elif D["kind"] == "target":
            need += [c.TARGET_REACHED, c.TARGET_NOT_REACHED, c.TARGET_EQUAL, c.TARGET_OUT_OF_RANGE]
        elif D["kind"] == "column":
            need += [c.COLUMN]
        else:
            need += [c.VALUE]
        if D["kind"] == "value" and D["lo"] == -np.inf:
            need = [b for b in need if b not in (c.CLIP_LO, c.CLIP_HI)]      # (the unclipped VALUE axis)
        out.append(need)
    return out


def _decoder(env, storage="f64"):
    from nuclear_sim_amd import controls
    P = env.params
    return controls.Decoder(env.controls_spec(), env.n, dt=float(P.dt), storage={"f64": "float64", "f32": "float32"}[storage],
                            speeds={"rod": P.max_control_rod_speed, "flow": P.max_flow_change_rate, "valve": P.max_valve_speed})


def _sp(spec, t, n):
    """the caller's setpoint column of step t, unless an axis fills that input"""
    return None if any(D["target"] == "power_setpoint" for D in spec["axes"]) else _setpoint(t, n)


def _positions(env, spec):
    from nuclear_sim_amd import controls
    return {D["target"]: _np(env.get_field(controls.MEMBERS[D["target"]])) for D in spec["axes"] if D["kind"] in ("rate", "target")}


def _compare_envs(a, ra, b, rb, where):
    """obs, reward, done, info and the whole state of two envs behind a step, by bits"""
    from nuclear_sim_amd.env import INFO_COLUMNS
    for k, (x, y) in enumerate(zip(ra[:3], rb[:3])):
        assert torch.equal(_tbits(x), _tbits(y)), (where, ("obs", "reward", "done")[k])
    for name in tuple(INFO_COLUMNS) + ("trip_flags",):
        assert torch.equal(_tbits(ra[3][name]), _tbits(rb[3][name])), (where, name)
    (fa, ia), (fb, ib) = a.state_arrays(), b.state_arrays()
    assert torch.equal(_tbits(fa), _tbits(fb)) and torch.equal(ia, ib), (where, "state")


# ---------------------------------------------------------------------------------------------------------------- 1, 3
CASES = [(1, "f64", N3, 8, 0, torch.float32, 1), (2, "f64", N3, 8, 1, torch.float64, 3), (5, "f32", N3, 8, 0, torch.float64, 3),
         (5, "f64", N3, 3, 0, torch.float32, 3), (2, "f32", N3, 1, 0, torch.float32, 1), (1, "f32", N3, 8, 1, torch.float32, 3),
         (5, "f64", 1, 8, 0, torch.float32, 1), (1, "f64", 1, 1, 0, torch.float64, 3), (2, "f32", 1, 3, 1, torch.float64, 1),
         (0, "f64", NSEG, 8, 1, torch.float32, 3), (0, "f32", NSEG, 3, 0, torch.float64, 1)]


@pytest.mark.parametrize("variant, storage, n, A, layout, dtype, K", CASES)
def test_bit_for_bit_with_the_numpy_statement_and_the_twin(variant, storage, n, A, layout, dtype, K):
    """Fails without the feature: set_controls does not exist.  A wrong kernel cannot pass: every member it moves, every column it fills and
    every value it holds is compared by bits at every step"""
    from nuclear_sim_amd import controls
    env, twin = _make(n, storage=storage), _make(n, storage=storage)
    start = _start(n)
    for e in (env, twin):
        if variant:
            e.set_step_kernel(variant)
        _put_start(e, start)
    env.set_controls(_axes(A, layout), interval=K, dtype=dtype)
    spec = env.controls_spec()
    assert len(spec["axes"]) == A and spec["interval"] == K
    tin = env.controls_input()
    assert tin.shape == (n, A) and tin.dtype == dtype and tin.is_contiguous() and env.controls_input().data_ptr() == tin.data_ptr()
    dec, rng = _decoder(env, storage), np.random.default_rng(1000 * A + K)
    seen = np.zeros(A, dtype=np.uint32)
    for t in range(STEPS):
        x = _inputs(spec, t, n, start, rng)
        out = dec.step(x, _positions(twin, spec))
        sp = _sp(spec, t, n)
        if t % 2:      # the policy writes into the bound tensor ... or hands its own
            tin.copy_(torch.as_tensor(x).to(tin))
            ra = env.step(power_setpoint=sp, controls=tin)
        else:
            ra = env.step(power_setpoint=sp, controls=torch.as_tensor(x))
        for a, pos in out["members"].items():
            twin.set_field(controls.MEMBERS[a], pos)
        rb = twin.step(power_setpoint=out["columns"].get("power_setpoint", sp), cooling_water_temp=out["columns"].get("cooling_water_temp"))
        _compare_envs(env, ra, twin, rb, t)
        assert ra[3]["controls"].shape == (A, n)
        _same_np(ra[3]["controls"], out["held"], ("held", t))
        st = env.controls_state()
        _same_np(st["held"], out["held"], ("held state", t))
        _same_np(st["prev"], out["prev"], ("prev", t))
        assert np.array_equal(st["age"], dec.age) and st["primed"].all() and not st["seen"].any(), t
        seen |= np.bitwise_or.reduce(out["report"], axis=1)
    if variant:
        assert env.last_step_kernel() == KERNEL_OF_VARIANT[variant] == twin.last_step_kernel(), env.last_step_kernel()
    else:
        assert env.last_step_kernel() == twin.last_step_kernel()
    if n >= N3:
        names = {v: k for k, v in controls.BRANCHES.items()}
        missing = [(a, names[b]) for a, need in enumerate(_wanted(spec)) for b in need if not seen[a] & b]
        assert not missing, missing
    env.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("code", [0, 1, 2, 3, 4, 5, 9, 10])
def test_one_rate_axis_is_step_with_that_action(code):
    """float64 storage: the controls env and a plain env stepping with (code, |y|) agree on everything, bit for bit -- the new path tied to
    the one the golden fixtures pin"""
    from nuclear_sim_amd import controls
    actuator = [a for a in controls.ACTUATORS if code in (controls.UP_CODES[a], controls.DOWN_CODES[a])][0]
    up = code == controls.UP_CODES[actuator]
    n = N3
    env, plain = _make(n), _make(n)
    start = _start(n)
    for e in (env, plain):
        _put_start(e, start)
    env.set_controls([(actuator, "rate")], dtype=torch.float64)
    rng = np.random.default_rng(code)
    moved = False
    for t in range(8):
        mag = rng.uniform(0.0, 1.0, n)
        mag[(np.arange(n) + t) % 9 == 0] = 0.0
        before = _np(env.get_field(controls.MEMBERS[actuator]))
        ra = env.step(power_setpoint=_setpoint(t, n), controls=torch.as_tensor((mag if up else -mag).reshape(n, 1)))
        rb = plain.step(action=np.full(n, code, dtype=np.int32), magnitude=mag, power_setpoint=_setpoint(t, n))
        _compare_envs(env, ra, plain, rb, (code, t))
        moved = moved or not np.array_equal(before, _np(env.get_field(controls.MEMBERS[actuator])))
    assert moved
    env.close(); plain.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def _hold_run(env, dec, steps, rng, start, between=None, autoreset_L=None):
    """steps of env against the Decoder's hold; the episode indices are counted from done / truncated as the episode kernel counts them"""
    n, spec = env.n, env.controls_spec()
    index = np.zeros(n, dtype=np.int32)
    restarted_latches = 0
    for t in range(steps):
        if between is not None:
            between(t)
        x = _inputs(spec, t, n, start, rng)
        age_before = dec.age.copy()
        fresh = (dec.primed == 0) | (dec.seen != index)
        out = dec.step(x, _positions(env, spec), index if autoreset_L is not None else None)
        obs, rew, done, info = env.step(power_setpoint=_sp(spec, t, n), controls=torch.as_tensor(x))
        st = env.controls_state()
        _same_np(st["held"], out["held"], ("held", t))
        _same_np(st["prev"], out["prev"], ("prev", t))
        assert np.array_equal(st["age"], dec.age) and st["primed"].all(), t
        if autoreset_L is not None:
            assert np.array_equal(st["seen"], dec.seen), t
        # a plant on the first step of a new hold latched whatever its age was, and prev == held
        if fresh.any():
            assert np.array_equal(out["held"][:, fresh].view(np.int64), out["prev"][:, fresh].view(np.int64)), t
            assert (dec.age[fresh] == 1).all(), t
            restarted_latches += int((age_before[fresh] % spec["interval"] != 0).sum())
        if autoreset_L is not None:
            ended = (_np(done) != 0) | (_np(info["truncated"]) != 0)
            assert np.array_equal(_np(info["episode_index"]), index), t
            index[ended] += 1
    return restarted_latches


@pytest.mark.parametrize("source", ["snapshot", "bank"])
def test_autoreset_restarts_the_hold(source):
    """a task ends the episodes at different steps per plant (a limit on the valve the controls move), max_episode_steps the rest: on the
    first step of a new episode a plant latches although its age was not due"""
    n, L, K = N3, 5, 3
    kw = dict(bank_seeds=range(100, 110)) if source == "bank" else {}
    env = _make(n, autoreset=True, max_episode_steps=L, **kw)
    start = _start(n)
    _put_start(env, start)
    env.snapshot()
    env.set_task(reward=[("reward", 1.0)], terminate=[("prim.steam_valve_position", ">", 70.0, -1.0)])
    env.set_controls(_axes(3), interval=K)
    dec, rng = _decoder(env), np.random.default_rng(5)
    off_phase = _hold_run(env, dec, 14, rng, start, autoreset_L=L)
    assert off_phase > 0                                   # restarts that an age counter alone would have held through
    assert len(np.unique(dec.seen)) > 1                    # the plants ended different numbers of episodes
    env.close()


def test_a_callers_restore_and_reset_restart_exactly_the_masked_plants():
    n, K = N3, 3
    env = _make(n)
    start = _start(n)
    _put_start(env, start)
    env.snapshot()
    env.set_controls(_axes(3), interval=K)
    dec, rng = _decoder(env), np.random.default_rng(6)
    masks = {4: np.arange(n) % 3 == 0, 8: np.arange(n) % 5 == 1}

    def between(t):
        if t in masks:
            m = torch.as_tensor(masks[t].astype(np.uint8))
            env.restore(m) if t == 4 else env.reset(m)
            dec.clear(masks[t])
    off_phase = _hold_run(env, dec, 11, rng, start, between=between)
    assert off_phase > 0
    assert len(np.unique(dec.age)) == 3                    # the two masked groups and the rest run on phases of their own
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_the_action_as_a_column_of_the_task_and_the_features():
    """an effort term and a jerk term over ("control", a) / ("control_prev", a), and ("control", a) stacked as a feature: the task's reward
    and terms and the stack are task.evaluate and features.Stack over the Decoder's held and prev"""
    from nuclear_sim_amd import features, task
    n, K = N3, 2
    env = _make(n)
    start = _start(n)
    _put_start(env, start)
    env.set_controls(_axes(3), interval=K, dtype=torch.float64)
    with pytest.raises(ValueError, match="the controls' axes are 0 .. 2, not 3"):
        env.set_task(reward=[(("control", 3), 1.0)])
    env.set_task(keep_terms=True, reward=[("reward", 1.0), (("control", 1), -0.1, "abs_err", 0.0), (("control", 1), -2.0, "sq_err", ("control_prev", 1)),
                                          (("control", 0), -0.001, "sq_err", "prim.steam_valve_position")])
    env.set_features([("control", 1), (("control", 0), {"ref": ("control_prev", 0), "scale": 0.01}), ("obs", 3), "task_reward"], stack=3, dtype=torch.float64)
    tspec, fspec = env.task_spec(), env.features_spec()
    stack = features.Stack(fspec["spec"], n)
    dec, rng = _decoder(env), np.random.default_rng(7)

    def with_decoder(samples, rows, out):
        samples = samples.copy()
        for r, R in enumerate(rows):
            if R["side"] and R["side"][0] in ("control", "control_prev"):
                samples[r] = out["held" if R["side"][0] == "control" else "prev"][R["side"][1]]
        return samples
    prev, primed, n_control_rows = None, np.zeros(n, dtype=bool), 0
    for t in range(8):
        x = _inputs(env.controls_spec(), t, n, start, rng)
        out = dec.step(x, _positions(env, env.controls_spec()))
        obs, rew, done, info = env.step(controls=torch.as_tensor(x))
        trows, frows = env._task["request"]["columns"], fspec["columns"]
        n_control_rows = sum(bool(R["side"]) and R["side"][0].startswith("control") for R in list(trows) + list(frows))
        w_rew, w_done, w_cause, w_terms, prev = task.evaluate(with_decoder(_np(env.task_samples()), trows, out), prev, primed, tspec)
        primed[:] = True
        _same_np(rew, w_rew, ("task reward", t))
        _same_np(info["task_terms"], w_terms, ("task terms", t))
        stack.step(with_decoder(_np(env.features_samples()), frows, out))
        _same_np(info["features"], stack.out, ("features", t))
        if t >= 2:
            assert (w_terms[1] < 0).any() and (w_terms[2] < 0).any() and (w_terms[3] < 0).any(), t      # effort; jerk; the valve's distance to its target
    assert n_control_rows >= 5
    with pytest.raises(Exception, match="the task and the features"):
        env.set_controls(None)                             # both read the controls' columns
    env.set_features(None); env.set_task(None)
    env.set_controls(None)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_checkpoint():
    """stop after 5 steps, save controls_state() beside state_arrays(), load both into a NEW env: the remaining steps are the
    uninterrupted run's; without the controls' state the hold starts anew and the run differs"""
    n, K, steps, at = N3, 3, 11, 5
    start = _start(n)
    z = np.random.default_rng(8).standard_normal((steps, n))

    def make():
        e = _make(n)
        _put_start(e, start)
        e.set_controls(_axes(8, 1), interval=K)
        return e

    def run(env, first, last):
        out = []
        for t in range(first, last):
            x = _inputs(env.controls_spec(), t, n, start, np.random.default_rng(100 + t))
            obs, rew, done, info = env.step(noise_z=z[t], controls=torch.as_tensor(x))
            f, i = env.state_arrays()
            out.append((obs.clone(), rew.clone(), f.clone(), i.clone(), info["controls"].clone()))
        return out
    a = make()
    run(a, 0, at)
    f, i = a.state_arrays()
    state = a.controls_state()
    assert sorted(state) == ["age", "held", "prev", "primed", "seen"] and (state["age"] == at).all()
    rest = run(a, at, steps)
    b = make()
    b.load_state_arrays(f, i)
    b.load_controls_state(state)
    for t, (x, y) in enumerate(zip(run(b, at, steps), rest)):
        assert all(torch.equal(_tbits(u), _tbits(v)) for u, v in zip(x, y)), t
    c = make()                                             # ... and without it every plant latches at once, out of phase
    c.load_state_arrays(f, i)
    first = run(c, at, at + 1)[0]
    assert not torch.equal(_tbits(first[4]), _tbits(rest[0][4]))
    for e in (a, b, c):
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def _raw_desc(env, axes, interval=1):
    """an npb_controls_desc_t over tensors of the test's own, past the Python refusals; returns (desc, keep)"""
    from nuclear_sim_amd import _lib
    spec = _lib.controls_request(axes, interval)
    cax = (_lib.NpbControlAxis * len(spec["axes"]))()
    for X, D in zip(cax, spec["axes"]):
        X.kind = _lib.CONTROL_KINDS[D["kind"]]
        X.target = 0 if D["target"] is None else (_lib.CONTROL_INPUTS if D["kind"] == "column" else _lib.CONTROL_ACTUATORS)[D["target"]]
        X.scale, X.offset, X.lo, X.hi, X.nan_to, X.deadband, X.max_magnitude = (D[k] for k in ("scale", "offset", "lo", "hi", "nan_to", "deadband", "max_magnitude"))
    A = len(spec["axes"])
    keep = [torch.zeros((env.n, A), dtype=torch.float32, device=env.device), torch.zeros((A, env.n), dtype=torch.float64, device=env.device),
            torch.zeros((A, env.n), dtype=torch.float64, device=env.device), cax]
    d = _lib.NpbControlsDesc()
    d.n_axes, d.axes, d.interval, d.in_type = A, cax, interval, 0
    d.input, d.held, d.prev = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()
    return d, keep


def test_lifecycle_and_refusals_on_a_live_handle():
    from nuclear_sim_amd import _lib
    n = 70
    env = _make(n)
    obs, rew, done, info = env.step(power_setpoint=_setpoint(0, n))
    assert "controls" not in info
    with pytest.raises(_lib.NpbError, match="no controls"):
        env.controls_input()
    with pytest.raises(_lib.NpbError, match="without controls"):
        env.step(controls=torch.zeros((n, 1)))
    env.set_controls([("rod", "rate")])
    env.step(power_setpoint=_setpoint(1, n), controls=torch.full((n, 1), 0.5))
    env.set_controls(_axes(3), interval=2)                                                       # again, another shape: every plant unprimed
    st = env.controls_state()
    assert st["held"].shape == (3, n) and not st["primed"].any()
    # a caller column for an input an axis fills is refused at step, naming the axis; what was set stays
    with pytest.raises(_lib.NpbError, match="the power_setpoint column must be NULL: axis 2 of the controls fills it"):
        env.step(power_setpoint=_setpoint(2, n))
    obs, rew, done, info = env.step(cooling_water_temp=np.full(n, 24.0))                         # the other input is the caller's still
    assert info["controls"].shape == (3, n) and env.controls_state()["primed"].all()
    # refusals of the library surface as NpbError with the reason, and leave what was set
    d, keep = _raw_desc(env, [("rod", "rate")])
    d.interval = 65
    with pytest.raises(_lib.NpbError, match="interval must be 1 .. NPB_CONTROLS_INTERVAL_MAX"):
        _lib.check(env.L.npb_set_controls(env._h, ctypes.byref(d)), env._h)
    with pytest.raises(ValueError, match="unknown actuator"):
        env.set_controls([("pump", "rate")])
    assert env.controls_input().shape == (n, 3)
    env.set_controls(None)
    obs, rew, done, info = env.step(power_setpoint=_setpoint(3, n))
    assert "controls" not in info
    for name, args in (("npb_controls_clear", (None, None)), ("npb_controls_get_state", (None,) * 6), ("npb_controls_set_state", (None,) * 6)):
        assert getattr(env.L, name)(env._h, *args) == -1 and b"no controls set" in env.L.npb_last_error(env._h), name
    with pytest.raises(_lib.NpbError, match="no controls"):
        env.controls_state()
    env.set_controls(None)                                                                       # off twice is fine
    env.close()
    ext = _make_external(n)
    with pytest.raises(ValueError, match="the plugin's power"):
        ext.set_controls([("power_setpoint", "column")])
    d, keep = _raw_desc(ext, [("power_setpoint", "column")])
    with pytest.raises(_lib.NpbError, match="a POWER_SETPOINT axis under NPB_HEAT_EXTERNAL"):
        _lib.check(ext.L.npb_set_controls(ext._h, ctypes.byref(d)), ext._h)
    ext.close()


def _make_external(n):
    from nuclear_sim_amd.env import BatchedPlantEnv
    return BatchedPlantEnv(n, dt=DT, heat_source="external")


def test_the_episode_streams_conflict_is_refused_both_ways():
    from nuclear_sim_amd import _lib
    n = 70
    # streams that drive the profile first: a POWER_SETPOINT axis is refused, by the env and by the library
    env = _make(n, autoreset=True, max_episode_steps=6, noise_generator="device", power_profile_steps=8, episode_streams=True)
    with pytest.raises(ValueError, match="the power profile drives"):
        env.set_controls([("power_setpoint", "column")])
    d, keep = _raw_desc(env, [("power_setpoint", "column")])
    with pytest.raises(_lib.NpbError, match="a POWER_SETPOINT axis while episode streams drive the profile"):
        _lib.check(env.L.npb_set_controls(env._h, ctypes.byref(d)), env._h)
    env.set_controls([("rod", "rate"), ("cooling_water_temp", "column")])                        # no setpoint axis: fine beside the streams
    env.step(controls=torch.zeros((n, 2)))
    env.close()
    # the axis first: streams with a profile are refused
    env = _make(n, autoreset=True, max_episode_steps=6, noise_generator="device", power_profile_steps=8)
    d, keep = _raw_desc(env, [("power_setpoint", "column")])
    _lib.check(env.L.npb_set_controls(env._h, ctypes.byref(d)), env._h)
    with pytest.raises(_lib.NpbError, match="a POWER_SETPOINT axis of the controls fills the setpoint column the profile would drive"):
        env.enable_episode_streams()
    _lib.check(env.L.npb_set_controls(env._h, None), env._h)
    env.enable_episode_streams()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_off_is_off():
    """an env that set and then dropped the controls steps bit for bit with one that never set them"""
    n = N3
    env, plain = _make(n), _make(n)
    env.set_controls(_axes(8), interval=2)
    env.set_controls(None)
    for t in range(6):
        ra, rb = env.step(power_setpoint=_setpoint(t, n)), plain.step(power_setpoint=_setpoint(t, n))
        assert "controls" not in ra[3]
        _compare_envs(env, ra, plain, rb, t)
    env.close(); plain.close()


# ---------------------------------------------------------------------------------------------------------------- 9
def test_the_shared_unprime_and_state_copy_of_task_features_and_controls():
    """The task, the features and the controls share one unprime kernel (blocks of 256) and one state copy over a parts list each.  On one
    env of 300 plants -- a full clear block and a partial one, four full waves and 44 lanes -- with all three set, ``clear_*`` under the mask
    ``plant % 3 == 0`` zeroes ``primed`` of exactly the masked plants in exactly that attachment and touches nothing else of its state, and
    a saved state put back over a later one reads back bit for bit; the same for a task without ``"delta"`` terms, whose ``prev`` is
    [0, n].  Integers and bits only: no tolerance."""
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 300
    mask = np.arange(n) % 3 == 0
    env = BatchedPlantEnv(n, dt=DT)
    env.set_controls([(None, "value")])
    env.set_features(["prim.fuel_temperature"], stack=2)
    parts = {"task": ("prev", "primed", "seen"), "features": ("primed", "seen"), "controls": ("held", "prev", "age", "primed", "seen")}
    states = {"task": env.task_state, "features": env.features_state, "controls": env.controls_state}
    loads = {"task": env.load_task_state, "features": env.load_features_state, "controls": env.load_controls_state}
    clears = {"task": env.clear_task, "features": env.clear_features, "controls": env.clear_controls}

    def step(t):
        env.step(power_setpoint=_setpoint(t, n), controls=torch.as_tensor(0.25 * t + 0.01 * np.arange(n)[:, None]))

    def same(got, want, where):
        assert sorted(got) == sorted(want), where
        for name in want:
            assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (where, name, got[name].dtype, got[name].shape)
            assert got[name].tobytes() == want[name].tobytes(), (where, name)

    t = 0
    for reward, n_delta in (([("prim.fuel_temperature", 1.0, "delta")], 1), ([("prim.fuel_temperature", 1.0)], 0)):
        env.set_task(reward=reward)
        step(t); step(t + 1)
        t += 2
        whose = ("task", "features", "controls") if n_delta else ("task",)
        last = {name: states[name]() for name in states}
        assert last["task"]["prev"].shape == (n_delta, n) and last["controls"]["held"].shape == (1, n)
        for who in whose:
            assert sorted(last[who]) == sorted(parts[who]) and (last[who]["primed"] == 1).all(), who
            clears[who](mask)
            now = {name: states[name]() for name in states}
            assert np.array_equal(now[who]["primed"], np.where(mask, 0, 1).astype(np.int32)), (who, n_delta)
            for other in states:      # nothing else of its own state has moved, and nothing at all of the other two's
                same({k: v for k, v in now[other].items() if (other, k) != (who, "primed")},
                     {k: v for k, v in last[other].items() if (other, k) != (who, "primed")}, (who, "clear", other))
            last = now
        step(t)      # the state moves on: every plant primed again, the controls' held, prev and age other values
        t += 1
        for who in whose:
            moved = states[who]()
            assert (moved["primed"] == 1).all() and (who != "controls" or moved["held"].tobytes() != last[who]["held"].tobytes()), who
            loads[who](last[who])
            same(states[who](), last[who], (who, "round trip"))
    env.close()
