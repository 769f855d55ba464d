"""GPU: running observation and reward normalisation on the device (npb_set_normalizer, BatchedPlantEnv.set_normalizer).

The reference is nuclear_sim_amd.normalizer, the numpy statement, fed with the rows the features read (env.features_samples: the existing
field and buffer paths) and with the step's reward, done and episode index columns.  Differences, squares, sums in a pinned order, IEEE
divisions and roots: the state, the stacks (and through them the features' table) and the normalised reward match by bits, with no
tolerance anywhere.

The run is the features suite's: BatchedPlantEnv.action_test("oil_top_off", seeds=range(n), dt=5.0), every plant with a setpoint of its
own, stepped with random actions.  Every test fails without the feature: set_normalizer does not exist."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DT = 5.0
BANK = tuple(range(500, 507))
STAMP = ("mpump.last_violation_time", 3, 15)      # a carried member nothing reads on these runs: it takes a NaN or an infinity unharmed
# eight columns, six of them eligible ("all"): members carried, output and int32, the observation, an info column, the reward
COLUMNS = [(("pump.oil_level", 0), {"ref": 50.0, "scale": 0.1, "clip": (-5.0, 5.0)}),
           ("obs", 3),
           (("info", "electrical_power"), {"ref": 900.0, "scale": 0.01, "fresh": 900.0}),
           (("sg.tube_wall_temp", 1), {"clip": (-10.0, 10.0)}),
           ("reward", {"nan_to": 0.0}),
           ("maintenance", {"scale": 0.25}),
           ("flags", {"bits": 0xF00}),
           (("obs", 5), {"ref": ("obs", 6)})]
ELIGIBLE = [0, 1, 2, 3, 4, 5]


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(a):
    a = np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a)
    return a.view(np.int32) if a.dtype == np.float32 else a.view(np.int64) if a.dtype == np.float64 else a


def _same(got, want, where):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (where, g.shape, w.shape, g.dtype, w.dtype)
    assert np.array_equal(g, w), (where, np.argwhere(g != w)[:4].tolist())


def _make(n, **kw):
    from nuclear_sim_amd.env import BatchedPlantEnv
    return BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, **kw)


def _inputs(t, n):
    """what step t is given: random actions and magnitudes, a setpoint and a noise draw per plant -- reproducible, the same for every env"""
    rng = np.random.default_rng(4000 + t)
    return dict(action=rng.integers(0, 11, n).astype(np.int32), magnitude=rng.random(n),
                power_setpoint=90.0 + 8.0 * np.sin(2.0 * np.pi * t / (20.0 + np.arange(n) % 7)), noise_z=rng.standard_normal(n))


def _reference(env):
    from nuclear_sim_amd import features
    return env.normalizer_spec(), features.Stack(env.features_spec()["spec"], env.n)


def _follow(env, Z, ref, out, where, index=None):
    """the statement behind one step of env: the fold, the table into the stack's spec, pass A; then state, stack and reward by bits"""
    obs, rew, done, info = out
    samples = _np(env.features_samples())
    nr = Z.step(samples, _np(rew), _np(done), index)
    ref.spec = Z.apply()
    ref.step(samples, index)
    state = env.normalizer_state()
    for name, want in Z.state().items():
        _same(state[name], want, (where, name))
    _same(info["features"], ref.out, (where, "features"))
    if nr is not None:
        _same(info["norm_reward"], nr, (where, "norm_reward"))
    else:
        assert "norm_reward" not in info
    return nr


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 64, 257, 300])
def test_bit_for_bit_with_the_numpy_statement(n, storage):
    """n = 1, a full wave, one group of the tree plus one plant, one group plus a partial wave; both storage types; the six eligible
    columns and the return stream: one pass of the partials kernel; K = 3, float32"""
    env = _make(n, storage=storage)
    env.set_features(COLUMNS, stack=3, dtype=torch.float32)
    env.set_normalizer("all", reward={"gamma": 0.99, "clip": 5.0})
    Z, ref = _reference(env)
    assert Z.columns == ELIGIBLE and Z.S == 7
    for t in range(12):
        _follow(env, Z, ref, env.step(**_inputs(t, n)), t)
    stats = env.normalizer_stats()
    assert stats["count"].tolist() == [12.0 * n] * 7
    if n > 1:
        assert (stats["var"][[0, 1, 2, 3]] > 0).all()      # the plants differ: something was summed
    env.close()


@pytest.mark.parametrize("n, storage", [(192, "f64"), (300, "f32")])
def test_arena_segments_smaller_than_a_group_of_the_tree(monkeypatch, n, storage):
    """NPB_ARENA_SEGMENT=64: the four waves of a workgroup of the partials kernel lie in four segments of the arena (three, and five with
    a ragged one); a reader that took the segment once per workgroup would read other plants' other columns"""
    monkeypatch.setenv("NPB_ARENA_SEGMENT", "64")
    env = _make(n, storage=storage)
    assert int(env.L.npb_state_arena_segment(env._h)) == 64
    env.set_features(COLUMNS, stack=2, dtype=torch.float64)
    env.set_normalizer("all", reward={"gamma": 0.99, "clip": 5.0})
    Z, ref = _reference(env)
    for t in range(4):
        _follow(env, Z, ref, env.step(**_inputs(t, n)), t)
    rows = _np(env.features_samples())
    for r in (0, 3):      # the member columns differ from plant to plant, in every wave: a reader on the wrong plant could not pass
        assert all(len(np.unique(rows[r, w:w + 64])) > 1 for w in range(0, n, 64)), r
    assert env.normalizer_state()["count"].tolist() == [4.0 * n] * 7
    env.close()


def test_more_streams_than_a_pass_and_than_a_chunk():
    """19 columns and the return stream: 20 streams, three passes of eight through LDS, two chunks of sixteen loads; a ragged n"""
    from nuclear_sim_amd.env import INFO_COLUMNS
    n = 300
    cols = COLUMNS[:6] + [("info", name) for name in INFO_COLUMNS[:7]] + [("obs", i) for i in range(6, 12)]
    env = _make(n, storage="f32")
    env.set_features(cols, stack=1, dtype=torch.float64)
    env.set_normalizer("all", reward={"gamma": 0.95, "clip": 3.0})
    Z, ref = _reference(env)
    assert Z.S == 20
    for t in range(4):
        _follow(env, Z, ref, env.step(**_inputs(t, n)), t)
    env.close()


def test_a_second_level_of_the_tree():
    """65 536 + 300 plants: 258 partials, the smallest n at which the finish kernel has a level of its own to run"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 65536 + 300
    env = BatchedPlantEnv(n)
    env.set_features([("prim.control_rod_position", {"ref": 50.0, "scale": 0.1}), "prim.coolant_flow_rate"], stack=1, dtype=torch.float32)      # what the actions move
    env.set_normalizer("all")
    Z, ref = _reference(env)
    for t in range(2):
        rng = np.random.default_rng(70 + t)
        _follow(env, Z, ref, env.step(action=rng.integers(0, 11, n).astype(np.int32), magnitude=rng.random(n), power_setpoint=rng.uniform(80.0, 100.0, n)), t)
    assert env.normalizer_stats()["count"].tolist() == [2.0 * n] * 2 and (env.normalizer_stats()["var"] > 0).all()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def test_a_nan_and_an_infinity_are_left_out_and_poison_nothing():
    n, bad, expected = 300, {5: np.nan, 256: np.inf, 299: -np.inf}, 0
    env = _make(n)
    env.set_features([(STAMP, {"nan_to": 0.0}), ("obs", 3)], stack=2, dtype=torch.float64)
    env.set_normalizer("all")
    Z, ref = _reference(env)
    other = env.normalizer_spec()      # a run in which those plants hold another bad value: they never count either way
    for t in range(5):
        if t == 2:
            v = _np(env.get_field(*STAMP))
            for p, x in bad.items():
                v[p] = x
            env.set_field(STAMP[0], v, STAMP[1], STAMP[2])
        _follow(env, Z, ref, env.step(**_inputs(t, n)), t)
        swapped = _np(env.features_samples())
        out = ~np.isfinite(swapped[0])
        if t == 2:
            assert np.isnan(swapped[0, 5]) and np.isinf(swapped[0, 256]) and np.isinf(swapped[0, 299]) and out.sum() == 3
        expected += n - int(out.sum())
        swapped[0, out] = np.where(np.isnan(swapped[0, out]), 1e200, np.nan)
        other.step(swapped)
    state = env.normalizer_state()
    assert state["count"].tolist() == [float(expected), 5.0 * n] and expected < 5 * n      # those samples are left out, of that stream alone
    assert np.isfinite(state["mean"]).all() and np.isfinite(state["M2"]).all()
    for name, want in other.state().items():
        _same(state[name], want, name)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_the_return_restarts_with_the_episode_and_the_rollout_records_the_normalised_reward():
    n, T = 70, 8
    kw = dict(autoreset=True, max_episode_steps=4, bank_seeds=BANK)
    env, twin = _make(n, **kw), _make(n, **kw)      # the twin never has a normaliser: what the episodes sum
    for e in (env, twin):
        e.set_features(COLUMNS[:4], stack=2, dtype=torch.float32)
    env.set_normalizer(None, reward={"gamma": 0.99, "clip": 5.0})
    env.set_rollout(T)
    twin.set_rollout(T)
    Z = env.normalizer_spec()
    recorded, previous, restarted, carried = [], None, 0, 0
    for t in range(T):
        for e in (env, twin):
            if t == 2:      # three plants scram on this step: terminated, beside the truncations every fourth step
                v = _np(e.get_field("prim.fuel_temperature"))
                v[[3, 40, 69]] = 1500.0
                e.set_field("prim.fuel_temperature", v)
        obs, rew, done, info = env.step(**_inputs(t, n))
        _, _, _, twin_info = twin.step(**_inputs(t, n))
        index = _np(info["episode_index"])
        nr = Z.step(None, _np(rew), _np(done), index)
        state = env.normalizer_state()
        for name, want in Z.state().items():
            _same(state[name], want, (t, name))
        _same(info["norm_reward"], nr, (t, "norm_reward"))
        recorded.append(nr)
        if previous is not None:
            moved = index != previous
            assert np.array_equal(_bits(state["ret"][moved]), _bits(_np(rew)[moved]))      # a new episode: the return is this step's reward
            restarted += int(moved.sum())
            carried += int((state["ret"][~moved] != _np(rew)[~moved]).sum())
        previous = index
        _same(info["episode_return"], twin_info["episode_return"], (t, "episode_return"))      # the raw sum
        _same(rew, twin.rollout()["reward"][t], (t, "raw reward"))
    assert restarted >= n + 3 and carried > 0
    assert (_np(env.rollout()["ended"])[2] & 1).any() and (_np(env.rollout()["ended"])[3] & 2).any()      # terminations and truncations both
    got = env.rollout()
    assert got["t"] == T
    _same(got["reward"], np.stack(recorded), "rollout reward")
    assert not np.array_equal(_bits(got["reward"]), _bits(twin.rollout()["reward"]))
    _same(got["ended"], twin.rollout()["ended"], "ended")
    for e in (env, twin):
        e.close()


def _follow_return(env, Z, out, where, index=None):
    obs, rew, done, info = out
    nr = Z.step(None, _np(rew), _np(done), None if index is None else _np(info["episode_index"]))
    state = env.normalizer_state()
    for name, want in Z.state().items():
        _same(state[name], want, (where, name))
    _same(info["norm_reward"], nr, (where, "norm_reward"))
    return state


def test_a_restart_of_the_callers_restarts_the_return():
    """clear_normalizer(mask); reset(mask) without autoreset, where no episode index is carried and the env unprimes the plants; restore(mask)
    with autoreset, where the bumped index does the work"""
    n = 130
    third, fifth = np.arange(n) % 3 == 0, np.arange(n) % 5 == 1
    env = _make(n)
    env.set_normalizer(None, reward={"gamma": 0.9, "clip": 5.0})
    Z = env.normalizer_spec()
    for t in range(3):
        _follow_return(env, Z, env.step(**_inputs(t, n)), t)
    env.clear_normalizer(torch.as_tensor(third.astype(np.uint8)))
    Z.clear(third)
    out = env.step(**_inputs(3, n))
    state = _follow_return(env, Z, out, "cleared")
    rew = _np(out[1])
    assert np.array_equal(_bits(state["ret"][third]), _bits(rew[third])) and (state["ret"][~third] != rew[~third]).any()
    env.reset(torch.as_tensor(fifth.astype(np.uint8)))      # no autoreset: no index; _after_restart unprimes the plants it reset
    Z.clear(fifth)
    out = env.step(**_inputs(4, n))
    state = _follow_return(env, Z, out, "reset")
    rew = _np(out[1])
    assert np.array_equal(_bits(state["ret"][fifth]), _bits(rew[fifth])) and (state["ret"][~fifth] != rew[~fifth]).any()
    assert not state["seen"].any()
    env.close()
    env = _make(n, autoreset=True)      # the index is carried: nothing is cleared, in the env or in the statement
    env.set_normalizer(None, reward={"gamma": 0.9, "clip": 5.0})
    Z = env.normalizer_spec()
    for t in range(3):
        _follow_return(env, Z, env.step(**_inputs(t, n)), t, index=True)
    env.restore(torch.as_tensor(fifth.astype(np.uint8)))
    out = env.step(**_inputs(3, n))
    state = _follow_return(env, Z, out, "restored", index=True)
    rew = _np(out[1])
    assert (state["seen"][fifth] != 0).all() and not (state["seen"][~fifth] != 0).all()      # the restore bumped their index
    assert np.array_equal(_bits(state["ret"][fifth]), _bits(rew[fifth])) and (state["ret"][~fifth] != rew[~fifth]).any()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_frozen():
    n = 130
    env = _make(n)
    env.set_features(COLUMNS, stack=3, dtype=torch.float32)
    env.set_normalizer(ELIGIBLE[:4], reward={"gamma": 0.9, "clip": 5.0})
    Z, ref = _reference(env)
    for t in range(4):
        _follow(env, Z, ref, env.step(**_inputs(t, n)), t)
    before = env.normalizer_state()
    env.normalizer_training(False)
    Z.training = False
    for t in range(4, 9):
        nr = _follow(env, Z, ref, env.step(**_inputs(t, n)), t)      # the frozen table, the reward still normalised
        assert np.abs(nr).max() > 0
    after = env.normalizer_state()
    for name in ("count", "mean", "M2"):
        _same(after[name], before[name], name)
    assert not np.array_equal(after["ret"], before["ret"])      # the return is still carried
    env.normalizer_training(True)
    Z.training = True
    _follow(env, Z, ref, env.step(**_inputs(9, n)), 9)
    assert env.normalizer_state()["count"][0] == 5.0 * n
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_checkpoint():
    """6 steps straight against 3 steps, a round trip into a fresh env -- arena, features state and stack, normaliser state -- and 3 more"""
    n = 130

    def fresh():
        env = _make(n)
        env.set_features(COLUMNS, stack=3, dtype=torch.float32)
        env.set_normalizer("all", reward={"gamma": 0.99, "clip": 5.0})
        return env

    def run(env, first, last):
        out = []
        for t in range(first, last):
            _, _, _, info = env.step(**_inputs(t, n))
            out.append((info["features"].clone(), info["norm_reward"].clone()))
        return out
    a = fresh()
    run(a, 0, 3)
    f, i = a.state_arrays()
    fstate, stack, nstate = a.features_state(), _np(a.features()), a.normalizer_state()
    rest = run(a, 3, 6)
    b = fresh()
    b.load_state_arrays(f, i)
    b.load_features_state(fstate, stack)
    b.load_normalizer_state(nstate)
    again = run(b, 3, 6)
    for t, ((fa, ra), (fb, rb)) in enumerate(zip(rest, again)):
        _same(fb, fa, (t, "features"))
        _same(rb, ra, (t, "norm_reward"))
    sa, sb = a.normalizer_state(), b.normalizer_state()
    for name in sa:
        _same(sb[name], sa[name], name)
    # the table follows a loaded state at once: a fresh frame is normalised with it before any step
    c = fresh()
    c.load_state_arrays(f, i)
    c.load_normalizer_state(nstate)
    from nuclear_sim_amd import features
    Z = c.normalizer_spec()
    Z.load_state(nstate)
    want = features.Stack(Z.apply(), n)
    c.get_observation()
    want.prime(_np(c.features_samples()))
    _same(c.features(), want.out, "primed with the loaded table")
    for e in (a, b, c):
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_off_gives_the_features_their_own_ref_and_scale_back():
    n, K = 70, 3
    a, b = _make(n), _make(n)
    for e in (a, b):
        e.set_features(COLUMNS, stack=K, dtype=torch.float32)
    a.set_normalizer("all")
    for t in range(3):
        fa = a.step(**_inputs(t, n))[3]["features"]
        fb = b.step(**_inputs(t, n))[3]["features"]
    assert not np.array_equal(_bits(fa[:, -1]), _bits(fb[:, -1]))
    a.set_normalizer(None)
    with pytest.raises(Exception):
        a.normalizer_state()
    for t in range(3, 3 + K):
        fa = a.step(**_inputs(t, n))[3]["features"]
        fb = b.step(**_inputs(t, n))[3]["features"]
        _same(fa[:, -1], fb[:, -1], (t, "the newest frame"))
    _same(fa, fb, "the whole stack, K steps on")
    for e in (a, b):
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_the_refusals_that_need_a_handle():
    from nuclear_sim_amd import _lib
    n = 70
    env = _make(n)
    with pytest.raises(ValueError, match="no features are set"):
        env.set_normalizer([0])
    env.set_task(reward=[("reward", 1.0)], terminate=[("done",)])
    env.set_features(COLUMNS, stack=2)
    env.set_normalizer("all", reward={"gamma": 0.99, "clip": 5.0})
    with pytest.raises(_lib.NpbError, match="normaliser"):      # set_features under it, set and None alike
        env.set_features(COLUMNS[:2])
    with pytest.raises(_lib.NpbError, match="normaliser"):
        env.set_features(None)
    assert env.features_spec()["spec"]["stack"] == 2
    with pytest.raises(_lib.NpbError, match="the normaliser"):      # set_task under the return stream, set and None alike
        env.set_task(None)
    with pytest.raises(_lib.NpbError, match="the normaliser"):
        env.set_task(reward=[("reward", 2.0)])
    assert env.L.npb_set_task(env._h, None) != 0 and b"return stream reads the task's reward" in env.L.npb_last_error(env._h)
    out = env.step(**_inputs(0, n))
    Z = env.normalizer_spec()
    _same(out[3]["norm_reward"], Z.step(_np(env.features_samples()), _np(out[1]), _np(out[2])), "the task's reward is the one normalised")
    env.set_rollout(4)
    with pytest.raises(_lib.NpbError, match="rollout"):      # set_normalizer under a rollout, set and None alike
        env.set_normalizer(None)
    with pytest.raises(_lib.NpbError, match="rollout"):
        env.set_normalizer("all")
    assert env.L.npb_set_normalizer(env._h, None) != 0 and b"set the normaliser, then the rollout" in env.L.npb_last_error(env._h)
    env.set_rollout(None)
    env.set_normalizer(None)
    env.set_features(None)
    env.set_task(None)
    env.close()
