"""GPU: order rules on the controls' axes (npb_set_control_orders, BatchedPlantEnv.set_control_orders): a policy output on a "value" axis
orders maintenance on the device, behind the decode and in front of the step.

The reference is a TWIN and the numpy statement.  Env A has the rules.  Env B has the same controls and no rules: which plants fire is
formed by nuclear_sim_amd.controls.Orders from controls.Decoder's held / latch / restart (B's own held is held against the Decoder's),
and B gets the perform_* calls of Orders.calls before each step.  Behind every step the observation, the reward, done, the info columns,
the trip flags and the whole state of A and B are compared by bits, A's fired and since with the statement's, and at the end the drained
maintenance logs record by record (sorted: across waves the log's order is the atomics').  Env C has the controls only: a plant on which
no rule has fired yet is, by bits, C's plant -- nothing was stored to it.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

from control_orders_support import (AXES, DT, NEVER, QUIET, RULES, STEPS, _compare_envs, _decoder, _follow, _inputs, _make, _np, _poke,  # noqa: F401
                                    _loop_env, _positions, _quiet, _records, _same_np, _tbits)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- the twin, by bits
CASES = [(70, 1, 1, np.float32, "f64"), (130, 3, 8, np.float64, "f64"), (130, 1, 8, np.float32, "f32"), (70, 3, 8, np.float64, "f32"),
         (130, 3, 1, np.float32, "f32")]


@pytest.mark.parametrize("n, K, R, dtype, storage", CASES)
def test_bit_for_bit_with_the_perform_calls_of_the_numpy_statement(n, K, R, dtype, storage):
    tdtype = torch.float64 if dtype is np.float64 else torch.float32
    A, B, C = (_make(n, storage=storage, maintenance_log=8192) for _ in range(3))
    for e in (A, B, C):
        _poke(e)
        e.set_controls(AXES, interval=K, dtype=tdtype)
    A.set_control_orders(RULES[:R])
    orders, dec, rng = A.control_orders_spec(), _decoder(B, storage), np.random.default_rng(11 + n + R)
    assert (A.control_orders_state()["since"] == NEVER).all()
    fired_ever, counts, at_threshold = np.zeros(n, dtype=bool), np.zeros(R, dtype=int), 0
    for t in range(STEPS):
        x = _inputs(t, n, rng, dtype)
        out = dec.step(x, _positions(B))
        fire = orders.step(out["held"], out["latch"], out["restart"])
        at_threshold += sum(int((out["latch"] & (out["held"][D["axis"]] == D["threshold"])).sum()) for D in orders.rules)
        for name, kw in orders.calls(fire):
            ok = getattr(B, name)(**kw)
            assert np.array_equal(_np(ok) != 0, kw["mask"] != 0), (t, name)      # at run time fire means success
        rb = B.step(controls=torch.as_tensor(x))
        _same_np(B.controls_state()["held"], out["held"], ("the twin's held", t))
        ra = A.step(controls=torch.as_tensor(x))
        rc = C.step(controls=torch.as_tensor(x))
        fa, ia = _compare_envs(A, ra, B, rb, t)
        got = A.control_orders()
        _same_np(got["fired"], fire.astype(np.float64), ("fired", t))
        assert torch.equal(ra[3]["orders"], got["fired"]) and "orders" not in rb[3]
        assert np.array_equal(got["since"], orders.since), ("since", t, np.argwhere(got["since"] != orders.since)[:4].tolist())
        # a plant on which nothing has fired is the plant of an env without rules: nothing was stored to it
        fired_ever |= fire.any(axis=0)
        fc, ic = C.state_arrays()
        still = torch.as_tensor(~fired_ever, device=fa.device)
        assert torch.equal(_tbits(fa[:, still]), _tbits(fc[:, still])) and torch.equal(ia[:, still], ic[:, still]), t
        for k, (u, v) in enumerate(zip(ra[:3], rc[:3])):
            assert torch.equal(_tbits(u[still]), _tbits(v[still])), (t, k)
        counts += fire.sum(axis=1)
    assert (counts > 0).all(), counts                      # every rule fired somewhere,
    assert not fired_ever[_quiet(n)].any() and fired_ever[~_quiet(n)].any() and at_threshold > 0      # the quiet never, and y == threshold was met
    fa, _ia = A.state_arrays()
    fc, _ic = C.state_arrays()
    moved = torch.as_tensor(fired_ever, device=fa.device)
    assert not torch.equal(_tbits(fa[:, moved]), _tbits(fc[:, moved]))      # and the service moved something
    (got, kinds), (want, _k), (plain, plain_kinds) = _records(A), _records(B), _records(C)
    assert got == want and got != plain
    families = {2} if R == 1 else {2, 3, 4}                # NPB_MAINT_EVENT_OPERATOR, _OPERATOR_COMPONENT, _OPERATOR_TURBINE
    assert sum(kinds.get(k, 0) for k in (2, 3, 4)) == counts.sum()      # one operator record per firing, beside the automatic maintenance's own
    assert families <= set(kinds) and not {2, 3, 4} & set(plain_kinds), (kinds, plain_kinds)
    for e in (A, B, C):
        e.close()


# ---------------------------------------------------------------------------------------------------------------- lifecycle
LIFE_RULES = [RULES[0], RULES[6], (3, "lubrication", "turbine_oil_change", {"min_interval": 4})]      # min_interval 1, 5 and 4


@pytest.mark.parametrize("source", ["snapshot", "bank"])
def test_autoreset_restarts_since_for_exactly_the_restarted_plants(source):
    """a task ends the episodes at different steps per plant (a limit on the valve the controls move), max_episode_steps the rest: on the
    first step of a new episode every rule of the plant may fire again, whatever its count was"""
    n, L, K = 130, 5, 2
    kw = dict(bank_seeds=range(100, 110)) if source == "bank" else {}
    env = _make(n, autoreset=True, max_episode_steps=L, **kw)
    env.set_field("prim.steam_valve_position", 40.0 + 0.25 * (np.arange(n) % 64))
    env.snapshot()
    env.set_task(reward=[("reward", 1.0)], terminate=[("prim.steam_valve_position", ">", 55.0, -1.0)])
    env.set_controls(AXES, interval=K)
    env.set_control_orders(LIFE_RULES)
    dec, orders = _decoder(env, "f64"), env.control_orders_spec()
    restarts = _follow(env, dec, orders, 14, np.random.default_rng(5), autoreset=True)
    assert restarts > 0 and len(np.unique(dec.seen)) > 1      # the plants ended different numbers of episodes
    env.close()


def test_reset_restore_and_clear_controls_restart_exactly_the_masked_plants():
    n, K = 130, 1
    env = _make(n)
    env.snapshot()
    env.set_controls(AXES, interval=K)
    env.set_control_orders(LIFE_RULES)
    dec, orders = _decoder(env, "f64"), env.control_orders_spec()
    masks = {3: np.arange(n) % 3 == 0, 6: np.arange(n) % 5 == 1, 8: np.arange(n) % 7 == 2}

    def between(t):
        if t in masks:
            m = torch.as_tensor(masks[t].astype(np.uint8))
            {3: env.restore, 6: env.reset, 8: env.clear_controls}[t](m)
            dec.clear(masks[t])
    restarts = _follow(env, dec, orders, 11, np.random.default_rng(6), between=between)
    assert restarts == sum(int(m.sum()) for m in masks.values())
    env.close()


def test_a_checkpoint_mid_interval_resumes_by_bits():
    n, K, steps, at = 70, 2, 11, 4
    z = np.random.default_rng(8).standard_normal((steps, n))      # the noise as a column: a new env's own stream would start over

    def make():
        e = _make(n)
        _poke(e)
        e.set_controls(AXES, interval=K)
        e.set_control_orders(LIFE_RULES)
        return e

    def run(env, first, last):
        out = []
        for t in range(first, last):
            x = _inputs(t, n, np.random.default_rng(100 + t), np.float32)
            x[~_quiet(n), 2:] = np.abs(x[~_quiet(n), 2:]) + 0.8
            obs, rew, done, info = env.step(noise_z=z[t], controls=torch.as_tensor(x))
            f, i = env.state_arrays()
            out.append((obs.clone(), rew.clone(), f.clone(), i.clone(), info["orders"].clone(), torch.as_tensor(env.control_orders()["since"])))
        return out
    a = make()
    run(a, 0, at)
    f, i = a.state_arrays()
    cstate, ostate = a.controls_state(), a.control_orders_state()
    assert sorted(ostate) == ["since"] and ostate["since"].shape == (3, n) and ostate["since"].dtype == np.int32
    waiting = ~_quiet(n)
    waiting[7] = False                                     # (plant 7's NaN on axis 2 became nan_to = 0.0: it never fires)
    assert (ostate["since"][1][waiting] == 4).all() and (ostate["since"][1][~waiting] == NEVER).all()      # mid-interval: rule 1 waits for its 5 steps
    rest = run(a, at, steps)
    b = make()
    b.load_state_arrays(f, i)
    b.load_controls_state(cstate)
    b.load_control_orders_state(ostate)
    for t, (x, y) in enumerate(zip(run(b, at, steps), rest)):
        assert all(torch.equal(_tbits(u), _tbits(v)) for u, v in zip(x, y)), t
    c = make()                                             # ... and without the rules' state every rule fires at once
    c.load_state_arrays(f, i)
    c.load_controls_state(cstate)
    first = run(c, at, at + 1)[0]
    assert not torch.equal(first[4], rest[0][4])
    for e in (a, b, c):
        e.close()


# ---------------------------------------------------------------------------------------------------------------- readers
def test_a_task_prices_an_order_the_features_carry_it_and_a_window_is_triggered_by_it():
    from nuclear_sim_amd import eventwin
    n, steps, pre, post = 130, 10, 1, 2
    env = _make(n)
    env.set_controls(AXES)
    with pytest.raises(ValueError, match="unknown column"):
        env.set_task(reward=[(("order", 0), 1.0)])         # no word without rules
    env.set_control_orders([RULES[0], (3, "stage", "overhaul", {"unit": 7, "threshold": 0.75, "min_interval": 3})])
    with pytest.raises(ValueError, match="the order rules are 0 .. 1, not 2"):
        env.set_task(reward=[(("order", 2), 1.0)])
    env.set_task(reward=[(("order", 1), -2.0), (("order", 0), -0.25)], bias=0.5)
    env.set_features([("order", 0), ("order", 1)], stack=2, dtype=torch.float64)
    env.enable_event_windows([("order", 1), ("pump.oil_level", 1)], triggers=[(("order", 1), ">", 0.5)], pre=pre, post=post)
    dec, orders, rng = _decoder(env, "f64"), env.control_orders_spec(), np.random.default_rng(9)
    fires, clock, oil = [], [], []
    for t in range(steps):
        x = _inputs(t, n, rng, np.float32)
        out = dec.step(x, _positions(env))
        fire = orders.step(out["held"], out["latch"], out["restart"]).astype(np.float64)
        obs, rew, done, info = env.step(controls=torch.as_tensor(x))
        _same_np(rew, (0.5 + -2.0 * fire[1]) + -0.25 * fire[0], ("the price of an order", t))
        feat = _np(info["features"])
        _same_np(feat[:, -1, :], fire.T, ("the newest frame", t))
        if t > 0:
            _same_np(feat[:, 0, :], fires[-1].T, ("the frame before", t))
        fires.append(fire); clock.append(_np(env.get_field("prim.sim_time"))); oil.append(_np(env.get_field("pump.oil_level", 1)))
    fires = np.array(fires)
    assert fires[:, 0].any() and fires[:, 1].any()
    values = np.stack([fires[:, 1], np.array(oil)], axis=1)
    want = eventwin.record(values, np.array(clock), fires[:, 1][:, None, :], [(">", 0.5)], pre, post)
    got = env.event_windows()
    assert len(want["plant"]) > 0
    eventwin.same(got, want)
    from nuclear_sim_amd._lib import NpbError
    for what in (lambda: env.set_control_orders(None), lambda: env.set_control_orders(RULES[:1]), lambda: env.set_controls(None), lambda: env.set_controls(AXES)):
        with pytest.raises(NpbError, match="the task and the features and the event windows read\\(s\\) the order rules' columns"):
            what()
    env.enable_event_windows(None); env.set_features(None); env.set_task(None)
    env.set_control_orders(None)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- the loop
def test_collect_is_t_steps_and_the_firing_history_is_what_the_rollouts_own_actions_make():
    n, T = 70, 8
    env, twin = _loop_env(n, T), _loop_env(n, T)
    got = env.collect(T)
    for t in range(T):
        twin.step()
    want = twin.rollout()
    assert got["t"] == want["t"] == T
    for name in ("obs", "act", "reward", "ended", "episode", "final_row", "final_obs"):
        g, w = got[name], want[name]
        assert (g is None) == (w is None), name
        if g is not None:
            assert torch.equal(_tbits(g), _tbits(w)), name
    (fa, ia), (fb, ib) = env.state_arrays(), twin.state_arrays()
    assert torch.equal(_tbits(fa), _tbits(fb)) and torch.equal(ia, ib)
    assert np.array_equal(env.control_orders()["since"], twin.control_orders()["since"])
    assert torch.equal(env.control_orders()["fired"], twin.control_orders()["fired"])
    # obs[t] is the stack in FRONT of step t: its newest frame carries what fired on step t - 1; Decoder + Orders make it of act[t - 1]
    act, obs, episode = _np(got["act"]), _np(got["obs"]), _np(got["episode"])
    dec, orders = _decoder(env, "f64"), env.control_orders_spec()
    members = {"rod": np.full(n, 50.0), "valve": np.full(n, 50.0)}      # (the value axis does not depend on the positions)
    fired_any = np.zeros(2, dtype=int)
    for t in range(T - 1):
        out = dec.step(act[t], members, episode[t].astype(np.int32))
        fire = orders.step(out["held"], out["latch"], out["restart"])
        restarted = episode[t + 1] != episode[t]           # a restarted plant's stack is its fresh frame: the order columns of the new state's step
        frame = obs[t + 1][:, -1, 2:]
        assert np.array_equal(frame[~restarted], fire.T[~restarted].astype(np.float32)), t
        fired_any += fire.sum(axis=1)
    assert (fired_any > 0).all() and (_np(got["ended"]) != 0).any()
    with pytest.raises(Exception, match="policy"):
        env.set_control_orders(None)
    env.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- refusals; off is off
def test_refusals_on_a_live_handle_and_off_is_off():
    from nuclear_sim_amd._lib import NpbError
    n = 130
    env, plain = _make(n), _make(n)
    with pytest.raises(NpbError, match="no controls"):
        env.set_control_orders(RULES)
    with pytest.raises(NpbError, match="no order rules"):
        env.control_orders()
    env.set_controls(AXES, interval=2)
    for bad, why in (([(0, "pump", "oil_change")], "a rule reads a 'value' axis"), ([(4, "pump", "oil_change")], "the controls' axes are 0 .. 3"),
                     ([(2, "pump", "npsh_analysis")], "has no handler"), ([(2, "pump", "oil_change", {"unit": 4})], "does not exist"),
                     ([(2, "bearing", "thrust_bearing_adjustment", {"unit": 0})], "thrust adjustment"),
                     ([(2, "stage", "cleaning")], "is not offered on the device"), ([(2, "pump", "oil_change", {"min_interval": 0})], "min_interval"),
                     ([(2, "pump", "oil_change", {"threshold": float("nan")})], "finite"), ([(2, "pump", "oil_change")] * 9, "1 to 8")):
        with pytest.raises(ValueError, match=why):
            env.set_control_orders(bad)
    # the library's own refusal, past the Python layer: a raw descriptor on the live handle
    import ctypes
    from nuclear_sim_amd import _lib
    table = (_lib.NpbControlOrder * 1)()
    table[0].axis, table[0].family, table[0].action, table[0].min_interval, table[0].amount = 1, 0, 0, 1, 95.0
    fired = torch.zeros((1, n), dtype=torch.float64, device=env.device)
    d = _lib.NpbControlOrdersDesc()
    d.n_orders, d.orders, d.fired = 1, table, fired.data_ptr()
    assert env.L.npb_set_control_orders(env._h, ctypes.byref(d)) != 0
    assert "not NPB_CONTROL_VALUE" in env.L.npb_last_error(env._h).decode()
    since = np.zeros((1, n), dtype=np.int32)
    assert env.L.npb_control_orders_get_state(env._h, since.ctypes.data, None) != 0
    assert "no order rules set" in env.L.npb_last_error(env._h).decode()
    # set and dropped -- by None, and by a new set_controls -- steps as an env that never had rules
    env.set_control_orders(RULES)
    env.set_control_orders(None)
    env.set_control_orders(RULES[:2])
    env.set_controls(None)
    with pytest.raises(NpbError, match="no order rules"):
        env.control_orders_state()
    for t in range(4):
        sp = 90.0 + 5.0 * np.sin(0.3 * t + np.arange(n))
        ra, rb = env.step(power_setpoint=sp), plain.step(power_setpoint=sp)
        assert "orders" not in ra[3]
        _compare_envs(env, ra, plain, rb, t)
    env.close(); plain.close()
