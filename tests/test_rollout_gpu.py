"""GPU: trajectories recorded on the device and their GAE advantages (npb_set_rollout, BatchedPlantEnv.set_rollout).

The reference is nuclear_sim_amd.rollout, the numpy statement, fed per step with what the caller would have copied by hand: a clone of
env.features() taken in front of the step, the inputs it wrote, and what step() returned.  Copies, comparisons, products, sums and a
narrowing: every comparison is by bits (view(int32) / view(int64)), with no tolerance anywhere.

The run is the features suite's: BatchedPlantEnv.action_test("oil_top_off", seeds=range(n), dt=5.0, autoreset=True), every plant with a
setpoint of its own, at most 12 steps, and its poke before a step: a fuel temperature of 1500 (the plant scrams on that step).  The pokes
are placed so that, with max_episode_steps 2 and 3 alike, every outcome -- neither bit, terminated, truncated, terminated on the step on
which the truncation was due -- occurs on some plant and not on another, on at least two different slots; each test asserts it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DT, T = 5.0, 8
# before step t: the plants whose fuel temperature is set to 1500; plants past the batch are left out
POKES = {1: [5, 66, 100], 2: [9, 64, 129], 4: [11, 200], 5: [20, 69, 299]}
COLUMNS = [(("pump.oil_level", 0), {"ref": 50.0, "scale": 0.02}), ("reward", {"scale": 0.5, "fresh": 0.0}), ("obs", 3), ("prim.fuel_temperature", {"scale": 1e-3}),
           (("obs", 5), {"ref": ("obs", 6), "scale": 3.0})]
AXES = [("rod", "rate"), ("valve", "rate", {"scale": 0.5}), (None, "value")]
TASK = dict(reward=[("reward", 1.0), (("pump.oil_level", 0), -0.25, "beyond", "<", 10.0)], terminate=[("done", -100.0)])
BANK = range(100, 110)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(a):
    """the bit patterns of a float tensor or array, as numpy integers; other types as they are"""
    a = np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a)
    return a.view(np.int32) if a.dtype == np.float32 else a.view(np.int64) if a.dtype == np.float64 else a


def _same(got, want, where):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (where, g.shape, w.shape, g.dtype, w.dtype)
    assert np.array_equal(g, w), (where, np.argwhere(g != w)[:4].tolist())


def _make(n, **kw):
    from nuclear_sim_amd.env import BatchedPlantEnv
    return BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, **kw)


def _setpoint(t, n):
    return 90.0 + 8.0 * np.sin(2.0 * np.pi * t / (20.0 + np.arange(n) % 7))


def _poke(env, t):
    plants = [p for p in POKES.get(t, ()) if p < env.n]
    if plants:
        v = _np(env.get_field("prim.fuel_temperature"))
        v[plants] = 1500.0
        env.set_field("prim.fuel_temperature", v)


def _env(n, L, C=4, K=2, dtype=torch.float32, storage="f64", bank=False, task=False, controls=True, autoreset=True):
    kw = dict(autoreset=True, max_episode_steps=L) if autoreset else {}
    env = _make(n, storage=storage, bank_seeds=BANK if bank else None, **kw)
    if task:
        env.set_task(**TASK)
    env.set_features(COLUMNS[:C], stack=K, dtype=dtype, final=True if autoreset else None)
    if controls:
        env.set_controls(AXES)
    return env


def _inputs(env, t, extras):
    """what the policy writes in front of step t: its controls and its extras, random and reproducible"""
    g = torch.Generator().manual_seed(1000 + t)
    act = extra = None
    if env._ctl is not None:
        act = (2.0 * torch.rand(env.controls_input().shape, generator=g) - 1.0).to(env.controls_input().dtype)
        env.controls_input().copy_(act)
    if extras:
        extra = (0.25 * torch.rand((env.n, extras), generator=g)).to(torch.float32)
        env.rollout_extras_input().copy_(extra)
    return act, extra


def _recorder(env):
    from nuclear_sim_amd import rollout
    s = env.rollout_spec()
    return rollout.Recorder(s["horizon"], env.n, s["stack"], axes=s["axes"], extras=s["extras"], final_rows=s["final_rows"], autoreset=s["autoreset"],
                            max_episode_steps=s["max_episode_steps"], obs_dtype=getattr(np, s["obs_dtype"]),
                            act_dtype=getattr(np, s["act_dtype"] or "float32"))


def _record(env, rec, steps, extras, t0=0, by_hand=None):
    """``steps`` recorded steps: the env's, and what the caller would have copied by hand into ``rec`` (and into the lists of ``by_hand``)"""
    for t in range(t0, t0 + steps):
        _poke(env, t)
        before = _np(env.features())
        act, extra = _inputs(env, t, extras)
        due = rec.length + 1 >= rec.max_steps if rec.max_steps else np.zeros(env.n, dtype=bool)
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, env.n))
        if env._episode is not None:
            over = (_np(done) != 0) | (_np(info["truncated"]) != 0)
            stack = np.where(over[:, None, None], _np(info["final_features"]), _np(info["features"]))      # the terminal frame appended
            index = _np(info["episode_index"])
        else:
            stack, index = _np(info["features"]), None
        rec.pre(before, None if act is None else _np(act), None if extra is None else _np(extra))
        bits = rec.post(_np(rew), _np(done), stack, episode=index)
        if by_hand is not None:
            by_hand.append({"obs": before, "act": act, "extra": extra, "reward": _np(rew), "done": _np(done) != 0, "due": due,
                            "truncated": _np(info["truncated"]) != 0 if env._episode is not None else np.zeros(env.n, dtype=bool), "episode": index,
                            "final": _np(info["final_features"]) if env._episode is not None else None, "bits": bits.copy()})


def _assert_outcomes_covered(ended, due):
    """neither bit, terminated, truncated and terminated-where-the-truncation-was-due: each on some plant and not on another of its slot, on
    at least two different slots"""
    kinds = {"neither": ended == 0, "terminated": (ended == 1) & ~due, "truncated": ended == 2, "terminated where the truncation was due": (ended == 1) & due}
    for what, m in kinds.items():
        slots = [t for t in range(m.shape[0]) if m[t].any() and not m[t].all()]
        assert len(slots) >= 2, (what, slots)


# ---------------------------------------------------------------------------------------------------------------- 1
CASES = [("snapshot", 70, "f64", 4, 2, torch.float32, 3, False, True), ("bank", 130, "f64", 3, 3, torch.float32, 2, True, True),
         ("snapshot", 300, "f32", 5, 2, torch.float64, 3, False, False), ("bank", 70, "f64", 4, 2, torch.float32, 3, True, False)]


@pytest.mark.parametrize("source, n, storage, C, K, dtype, L, task, controls", CASES)
def test_the_record_bit_for_bit(source, n, storage, C, K, dtype, L, task, controls):
    """Every recorded tensor against what the caller would have copied by hand, and the whole against rollout.Recorder.  K * C = 9 is no
    multiple of 16 bytes (the one-element copies and the 4-byte tail), n * K * C of the other float cases puts slot 1 on 16, 8 or 4 bytes.
    Fails without the feature: set_rollout does not exist"""
    E = 2
    env = _env(n, L, C, K, dtype, storage, bank=source == "bank", task=task, controls=controls)
    env.set_rollout(T, extras=E)
    spec = env.rollout_spec()
    assert spec["final_rows"] == -(-T // L) and env.rollout()["t"] == 0
    rec, hand = _recorder(env), []
    _record(env, rec, T, E, by_hand=hand)
    r = env.rollout()
    assert r["t"] == T == rec.t
    assert r["obs"].shape == (T, n, K, C) and r["obs"].dtype == dtype and r["reward"].dtype == torch.float64 and r["ended"].dtype == torch.uint8
    got = {k: (None if v is None else _np(v)) for k, v in r.items() if k != "t"}
    taken = set()
    for t, h in enumerate(hand):
        _same(got["obs"][t], h["obs"], ("obs", t))                          # a clone of env.features() taken before step t
        if controls:
            _same(got["act"][t], h["act"], ("act", t))
        _same(got["extra"][t], h["extra"], ("extra", t))
        _same(got["reward"][t], h["reward"], ("reward", t))                 # the returned reward: the task's with a task
        assert np.array_equal(got["ended"][t], h["done"] * 1 + h["truncated"] * 2), t
        assert not (h["done"] & h["truncated"]).any()
        assert np.array_equal(got["episode"][t], h["episode"]), t
        assert np.array_equal(got["final_row"][t] >= 0, h["truncated"]), t   # a row for every truncated (t, p), -1 everywhere else
        for p in np.flatnonzero(h["truncated"]):
            row = int(got["final_row"][t, p])
            assert p * spec["final_rows"] <= row < (p + 1) * spec["final_rows"] and row not in taken, (t, p, row)
            taken.add(row)
            _same(got["final_obs"][row], h["final"][p], ("final_obs", t, int(p)))
    assert got["act"] is None if not controls else got["act"].shape == (T, n, len(AXES))
    want = rec.arrays()
    for name in ("obs", "act", "extra", "reward", "ended", "episode", "final_row", "final_obs"):
        if want[name] is not None:
            _same(got[name], want[name], name)
    _assert_outcomes_covered(got["ended"], np.stack([h["due"] for h in hand]))
    if L == 2:
        assert rec.n_final.max() == spec["final_rows"]                       # the bound, met with equality
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.fixture(scope="module")
def recorded():
    """130 plants, 12 slots of which 11 are recorded (more than one group of the kernel's loads, the last one ragged), E = 3"""
    env = _env(130, 3)
    env.set_rollout(12, extras=3)
    rec, hand = _recorder(env), []
    _record(env, rec, 11, 3, by_hand=hand)
    yield env, rec, hand
    env.close()


def test_advantages_bit_for_bit_with_the_numpy_statement(recorded):
    from nuclear_sim_amd import rollout
    env, rec, hand = recorded
    r = env.rollout()
    t, n, R = r["t"], env.n, env.rollout_spec()["final_rows"]
    assert t == 11 and R == 4
    ended, reward, final_row = _np(r["ended"])[:t], _np(r["reward"])[:t], _np(r["final_row"])[:t]
    _assert_outcomes_covered(ended, np.stack([h["due"] for h in hand]))
    g = torch.Generator().manual_seed(7)
    values = (torch.rand((12, n), generator=g) - 0.5).to(torch.float32)
    last = (torch.rand(n, generator=g) - 0.5).to(torch.float32)
    final = (torch.rand(n * R, generator=g) - 0.5).to(torch.float32)
    extra = _np(r["extra"])
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0)):
        for dtype, np_dtype in ((torch.float32, np.float32), (torch.float64, np.float64)):
            for how in ("tensor", "extra", "none"):
                given = {"tensor": values, "extra": ("extra", 1), "none": None}[how]
                v = {"tensor": _np(values)[:t], "extra": extra[:t, :, 1], "none": None}[how]
                adv, ret = env.rollout_advantages(gamma, lam, values=given, last_value=last, final_values=final, dtype=dtype)
                assert adv.shape == (t, n) and adv.dtype == dtype and ret.dtype == dtype
                want_adv, want_ret = rollout.advantages(reward, ended, final_row, v, _np(last), _np(final), gamma, lam, np_dtype)
                _same(adv, want_adv, ("adv", gamma, lam, how, str(dtype)))
                _same(ret, want_ret, ("ret", gamma, lam, how, str(dtype)))
    # the truncated slots bootstrapped from the value of their terminal stack: another final value, another advantage there
    adv0 = _np(env.rollout_advantages(0.99, 0.95, values=values, last_value=last, final_values=final)[0])
    adv1 = _np(env.rollout_advantages(0.99, 0.95, values=values, last_value=last, final_values=final + 1.0)[0])
    assert (adv0 != adv1)[ended == 2].all() and not (adv0 != adv1)[ended == 1].any()
    # no last value, no values: the discounted return-to-go, by bits of the plain loop
    _, ret = env.rollout_advantages(0.9, 1.0, final_values=torch.zeros(n * R), dtype=torch.float64)
    go, want = np.zeros(n), np.zeros((t, n))
    for s in range(t - 1, -1, -1):
        go = reward[s] + 0.9 * np.where(ended[s] != 0, 0.0, go)
        want[s] = go
    _same(ret, want, "return-to-go")
    # refusals on the live handle
    for kw, why in (({"gamma": 1.5}, "gamma and lam"), ({"lam": float("nan")}, "gamma and lam"), ({"final_values": None}, "final_value")):
        args = dict({"gamma": 0.9, "lam": 0.9, "final_values": final}, **kw)
        with pytest.raises(Exception, match=why):
            env.rollout_advantages(**args)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_a_callers_restart_between_two_steps_cuts_the_masked_plants():
    from nuclear_sim_amd import rollout
    n, L, E = 70, 3, 1
    env = _env(n, L, bank=True)
    env.set_rollout(T, extras=E)
    rec = _recorder(env)
    env.restore(torch.as_tensor(np.arange(n) % 2 == 0))                       # nothing recorded yet: nothing in front of slot 0
    rec.cut(np.arange(n) % 2 == 0)
    assert env.rollout()["t"] == 0 and not _np(env.rollout()["ended"]).any()
    masks = {1: ("reset", np.arange(n) % 3 == 0), 3: ("restore", np.arange(n) % 5 == 1), 4: ("restore_from_bank", np.arange(n) % 7 == 2)}
    for t in range(6):
        _record(env, rec, 1, E, t0=t)
        if t in masks:
            what, mask = masks[t]
            before = _np(env.rollout()["ended"])
            getattr(env, what)(torch.as_tensor(mask))
            rec.cut(mask)
            after = _np(env.rollout()["ended"])
            changed = after != before
            assert changed[t][mask].all() and not changed[t][~mask].any() and not np.delete(changed, t, axis=0).any(), what
            assert ((after[t] & 4) != 0).tolist() == mask.tolist(), what
    r = env.rollout()
    _same(r["ended"], rec.ended, "ended")
    _same(r["final_row"], rec.final_row, "final_row")
    _same(r["episode"], rec.episode, "episode")
    t = r["t"]
    ended, reward, final_row = _np(r["ended"])[:t], _np(r["reward"])[:t], _np(r["final_row"])[:t]
    g = torch.Generator().manual_seed(3)
    values, last = torch.rand((T, n), generator=g), torch.rand(n, generator=g)
    final = torch.rand(n * env.rollout_spec()["final_rows"], generator=g)
    adv, ret = env.rollout_advantages(0.99, 0.95, values=values, last_value=last, final_values=final, dtype=torch.float64)
    want_adv, want_ret = rollout.advantages(reward, ended, final_row, _np(values)[:t], _np(last), _np(final), 0.99, 0.95, np.float64)
    _same(adv, want_adv, "adv"); _same(ret, want_ret, "ret")
    # the advantages stop there: a slot that is cut and nothing else is its own delta without a bootstrap
    only_cut = ended == 4
    assert only_cut.any()
    delta = reward - _np(values)[:t].astype(np.float64)
    assert np.array_equal(_bits(_np(adv)[only_cut]), _bits(delta[only_cut] + 0.0))
    uncut, _ = rollout.advantages(reward, ended & 3, final_row, _np(values)[:t], _np(last), _np(final), 0.99, 0.95, np.float64)
    assert (uncut[only_cut] != want_adv[only_cut]).all()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_lifecycle_and_refusals_on_a_live_handle():
    n, L = 70, 2
    env = _make(n, autoreset=True, max_episode_steps=L)
    with pytest.raises(Exception, match="features"):
        env.set_rollout(4)                                                     # without features
    with pytest.raises(Exception, match="set_rollout"):
        env.rollout()
    env.set_features(COLUMNS[:4], stack=2, final=True)
    env.set_controls(AXES)
    env.set_rollout(4, extras=1)
    rec = _recorder(env)
    _record(env, rec, 4, 1)
    assert env.rollout()["t"] == 4
    state = [x.clone() for x in env.state_arrays()]
    kept = {k: v.clone() for k, v in env.rollout().items() if isinstance(v, torch.Tensor)}
    feats = env.features().clone()
    with pytest.raises(Exception, match="npb_rollout_begin"):
        env.step(power_setpoint=_setpoint(4, n))                               # t == T: refused
    assert env.rollout()["t"] == 4                                             # ... and nothing recorded or stepped
    for a, b in zip(state, env.state_arrays()):
        _same(a, b, "the state after the refused step")
    _same(feats, env.features(), "the features after the refused step")
    for k, v in kept.items():
        _same(v, env.rollout()[k], (k, "after the refused step"))
    env.rollout_begin()                                                        # rewinds
    assert env.rollout()["t"] == 0 and (_np(env.rollout()["final_row"]) == -1).all()
    rec.begin()
    _record(env, rec, 2, 1, t0=4)
    assert env.rollout()["t"] == 2
    _same(env.rollout()["final_row"], rec.final_row, "final_row after the rewind")
    _same(env.rollout()["final_obs"], rec.final_obs, "final_obs after the rewind")
    _same(env.rollout()["ended"][:2], rec.ended[:2], "ended after the rewind")
    for call in (lambda: env.set_features(COLUMNS[:2]), lambda: env.set_features(None), lambda: env.set_controls(AXES[:1]), lambda: env.set_controls(None)):
        with pytest.raises(Exception, match="rollout"):
            call()
    from nuclear_sim_amd import _lib
    assert env.L.npb_set_features(env._h, None) != 0 and b"rollout" in env.L.npb_last_error(env._h)      # the library's own refusal
    assert env.L.npb_set_controls(env._h, None) != 0 and b"rollout" in env.L.npb_last_error(env._h)
    env.set_rollout(4, final_rows=1)                                           # R below ceil(4 / 2): refused by the step
    with pytest.raises(_lib.NpbError, match="final_rows"):
        env.step(power_setpoint=_setpoint(6, n))
    assert env.rollout()["t"] == 0
    with pytest.raises(Exception, match="t == 0"):
        env.rollout_advantages(0.9, 0.9)
    env.set_rollout(None)                                                      # off: everything as before
    with pytest.raises(Exception, match="set_rollout"):
        env.rollout()
    env.step(power_setpoint=_setpoint(6, n))
    env.set_controls(None)
    env.set_features(COLUMNS[:2])
    env.step(power_setpoint=_setpoint(7, n))
    env.set_rollout(None)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_off_is_off_and_on_changes_nothing_else():
    """obs, reward, done, info, the features and the whole state after 8 steps, with the rollout on, are those of a twin without it"""
    n, L = 130, 3
    env, twin = _env(n, L, task=True), _env(n, L, task=True)
    env.set_rollout(T, extras=2)
    for e in (env, twin):
        e.features()                                                           # both primed: the rollout primes before its first step
    for t in range(T):
        outs = []
        for e in (env, twin):
            _poke(e, t)
            _inputs(e, t, 2 if e is env else 0)
            outs.append(e.step(power_setpoint=_setpoint(t, n)))
        (obs, rew, done, info), (t_obs, t_rew, t_done, t_info) = outs
        _same(obs, t_obs, ("obs", t)); _same(rew, t_rew, ("reward", t))
        assert torch.equal(done, t_done), t
        assert set(info) == set(t_info)
        for k, v in info.items():
            if isinstance(v, torch.Tensor):
                _same(v, t_info[k], (k, t))
    _same(env.features(), twin.features(), "features")
    for a, b in zip(env.state_arrays(), twin.state_arrays()):
        _same(a, b, "state")
    assert (_np(env.rollout()["ended"]) != 0).any()
    env.close(); twin.close()
