"""GPU: the policy on the device (npb_set_policy, BatchedPlantEnv.set_policy) -- an MLP actor-critic, the Gaussian draw, the
log-probability and the value in one launch in front of every step -- against nuclear_sim_amd.policy, the numpy statement, fed the
device's own features.  A relu net is compared by bits (view(int32) / view(int64)), with no tolerance anywhere; a tanh net within a bound
the test computes from its own weights; the noise within 1e-12 of the statement's (the device library's double log, sin and cos are the
one thing that may differ) and its Philox words exactly.

The run is the features suite's: BatchedPlantEnv.action_test("oil_top_off", seeds=range(n), dt=5.0), every plant with a setpoint of its
own, a handful of steps.  Weights come from a seeded generator, every row's L1 norm between 1 and 4.  The shapes are chosen for where
tiles go wrong: one plant, one more than a tile of 32, two tiles, 257; 15, 64 and 256 cells (no multiple of 4, the small build's
limit, the maximum); widths 7, (33, 17), (64, 64) and (128, 128, 128); 1, 3 and 8 axes; float and double features and controls.

Every case here lies wholly at or under the small build's limits (64 cells, widths of 64) or at the maximum.  The shapes BETWEEN them are
test_policy_shapes_gpu.py's table, run through this file's helpers by the same contracts, each row the smallest case of something the
launcher or the layer routine decides: a 65 cells with widths of 64 (cells alone one past the small build; in_pad 68); b 64 cells, actor
(65,), critic (7,) (the actor alone one past; out_pad 96); c the same with the nets swapped (the widest layer is taken over BOTH nets);
d 100 cells, (100, 96) / (127,), 5 axes (a last k-block with 4 live columns, 127 -> 128, a half-used Box-Muller pair); e 255 cells,
(128,) / (1,), 7 axes (255 -> 256, a hidden width of 1); f 66 cells, (31, 32, 33) / (3, 2, 1), 6 axes (three layers around 32)."""
import numpy as np
import pytest
import torch

from nuclear_sim_amd import policy, rollout

pytestmark = pytest.mark.gpu

DT = 5.0
STAMP = ("mpump.last_violation_time", 3, 15)      # a carried member nothing reads on these runs: it takes a NaN or an infinity unharmed
AXES = [("rod", "rate"), ("valve", "rate", {"scale": 0.5}), (None, "value"), ("flow", "rate"), ("boron", "rate"), (None, "value"), (None, "value"),
        (None, "value", {"scale": 2.0})]
F32, F64 = torch.float32, torch.float64


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(a):
    a = np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a)
    return a.view(np.int32) if a.dtype == np.float32 else a.view(np.int64) if a.dtype == np.float64 else a


def _same(got, want, where):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (where, g.shape, w.shape, g.dtype, w.dtype)
    assert np.array_equal(g, w), (where, np.argwhere(g != w)[:4].tolist())


def _columns(C, stamp=False):
    """C columns, each at a scale of its own that keeps the cells of order 1: the observation and, last, a pump's oil level; ``stamp``: the
    first is the STAMP member"""
    cols = [(("obs", j % 22), {"scale": 1e-3 * (1 + j // 22)}) for j in range(C)]
    cols[-1] = (("pump.oil_level", 0), {"ref": 50.0, "scale": 0.02})      # (randomised per plant: the plants differ from the first frame on)
    if stamp:
        cols[0] = (STAMP, {"scale": 1e-3, "nan_to": float("nan")})
    return cols


def _setpoint(t, n, first=0):
    return 90.0 + 8.0 * np.sin(2.0 * np.pi * t / (20.0 + (first + np.arange(n)) % 7))


def _env(n, C, K, fdtype, A, cdtype, storage="f64", first=0, stamp=False, **kw):
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(first, first + n), dt=DT, storage=storage, **kw)
    env.set_features(_columns(C, stamp), stack=K, dtype=fdtype)
    env.set_controls(AXES[:A], dtype=cdtype)
    return env


def _weights(seed, cells, A, actor, critic):
    rng = np.random.default_rng(seed)

    def net(dims):
        out = []
        for i, o in dims:
            W = rng.standard_normal((o, i))
            W *= rng.uniform(1.0, 3.9, (o, 1)) / np.abs(W).sum(axis=1, keepdims=True)
            out.append((W.astype(np.float32), (0.1 * rng.standard_normal(o)).astype(np.float32)))
        return out
    a, c = policy.sizes(cells, A, actor, critic)
    return net(a), net(c), (0.3 * rng.standard_normal(A) - 0.7).astype(np.float32)


def _statement(env):
    """the numpy statement of the env's policy, loaded with the parameters the device holds (its std is the one torch formed)"""
    S = env.policy_spec()
    P = policy.Policy(S["cells"], S["n_axes"], S["actor"], S["critic"], S["activation"], S["seed"], S["deterministic"], S["first_plant"],
                      getattr(np, S["act_dtype"]))
    P.load(_np(env.policy_theta()))
    P.t = int(env.policy_state()["t"])
    return P


def _step(env, t, first=0):
    return env.step(power_setpoint=_setpoint(t, env.n, first))


# ---------------------------------------------------------------------------------------------------------------- 1
CASES = [(1, 5, 3, F32, (7,), (7,), 1, F32, "f64"), (33, 16, 4, F64, (64, 64), (33, 17), 3, F64, "f64"),
         (64, 16, 4, F32, (128, 128, 128), (128, 128, 128), 8, F32, "f64"), (257, 64, 4, F32, (33, 17), (64, 64), 3, F32, "f32"),
         (257, 5, 3, F64, (7,), (64, 64), 8, F64, "f64")]


@pytest.mark.parametrize("n, C, K, fdtype, actor, critic, A, cdtype, storage", CASES)
def test_relu_deterministic_bit_for_bit(n, C, K, fdtype, actor, critic, A, cdtype, storage):
    """controls_input(), value and logp are the statement's bits, and the rollout's act and extra slots hold the same.
    Fails without the feature: set_policy does not exist"""
    env = _env(n, C, K, fdtype, A, cdtype, storage)
    env.set_rollout(4, extras=3)
    a, c, log_std = _weights(n + C, K * C, A, actor, critic)
    env.set_policy(a, c, log_std, activation="relu", deterministic=True, extras={"value": 2, "logp": 0})
    theta = _np(env.policy_theta())
    _same(theta, policy.pack(a, c, log_std, std=theta[-A:]), "theta")
    assert np.allclose(theta[-A:], np.exp(log_std), rtol=1e-6, atol=0)
    P, kept = _statement(env), []
    for t in range(3):
        before = _np(env.features())
        obs, rew, done, info = _step(env, t)
        act, value, logp = P.step(before)
        assert np.isfinite(act).all() and np.isfinite(value).all() and np.isfinite(logp).all()
        _same(env.controls_input(), act, (t, "act")); _same(info["value"], value, (t, "value")); _same(info["logp"], logp, (t, "logp"))
        _same(env.policy_outputs()["value"], value, (t, "outputs"))
        kept.append((act, value, logp))
    assert env.policy_state()["t"] == 0      # nothing was drawn
    if n > 1:
        assert np.ptp(kept[-1][0], axis=0).min() > 0 and np.ptp(kept[-1][1]) > 0      # the plants differ: the nets do read their features
    r = env.rollout()
    assert r["t"] == 3
    for t, (act, value, logp) in enumerate(kept):
        _same(r["act"][t], act, (t, "rollout act")); _same(r["extra"][t, :, 2], value, (t, "extra value")); _same(r["extra"][t, :, 0], logp, (t, "extra logp"))
        assert not _np(r["extra"][t, :, 1]).any()      # the caller's slot is left alone
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def _hold_sampling(env, seed):
    """three sampling steps of an env whose policy was set with ``seed``: the Philox words exactly, z within 1e-12 of the statement's, and
    action, value and logp the statement's bits when it is fed the device's own z"""
    n, A = env.n, env.policy_spec()["n_axes"]
    P = _statement(env)
    for t in range(3):
        z, words = env.policy_noise(t, words=True)
        want_words = policy.noise_words(seed, t, n, A)
        assert np.array_equal(_np(words).astype(np.uint32), want_words), t
        want_z = policy.noise_from_words(want_words, A)
        assert np.abs(_np(z) - want_z).max() <= 1e-12 and np.abs(_np(z)).max() <= policy.Z_MAX, (t, np.abs(_np(z) - want_z).max())
        before = _np(env.features())
        assert env.policy_state()["t"] == t
        obs, rew, done, info = _step(env, t)
        act, value, logp = P.step(before, z=_np(z))
        _same(env.controls_input(), act, (t, "act")); _same(info["value"], value, (t, "value")); _same(info["logp"], logp, (t, "logp"))
    assert env.policy_state()["t"] == 3 and P.t == 3
    assert not np.array_equal(_np(env.policy_noise(0)), _np(env.policy_noise(1)))


@pytest.mark.parametrize("n, A, cdtype, seed", [(33, 3, F32, 7), (257, 8, F64, 2 ** 64 - 3), (64, 1, F32, 0)])
def test_relu_sampling_the_words_the_noise_and_the_outputs(n, A, cdtype, seed):
    """The Philox words exactly, z within 1e-12 of the statement's, and action and logp the statement's bits when it is fed the device's own
    z -- which also pins that the step's launch and npb_policy_noise draw the same numbers.  The axes counts 1, 3 and 8 are here; 2, 5
    and 7 (with 5 and 7 the last pair is half used) run on the shape table's rows in test_policy_shapes_gpu.py, through the same body"""
    env = _env(n, 5, 3, F32, A, cdtype)
    a, c, log_std = _weights(n, 15, A, (33, 17), (7,))
    env.set_policy(a, c, log_std, activation="relu", seed=seed)
    _hold_sampling(env, seed)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def _tanh_bound(net):
    """U = 5 * 2^-24, the float tanh's bound; L_i the largest row L1 norm of layer i: e_1 = U, e_i = L_i * e_(i - 1) + U over the hidden
    layers, and the head's outputs are within L_head * e_last"""
    U = 5.0 * 2.0 ** -24
    L = [float(np.abs(W.astype(np.float64)).sum(axis=1).max()) for W, _ in net]
    assert max(L) <= 4.0
    e = U
    for Li in L[1:-1]:
        e = Li * e + U
    return L[-1] * e


@pytest.mark.parametrize("n, C, K, fdtype, actor, critic", [(64, 16, 4, F32, (64, 64), (33, 17)), (33, 5, 3, F64, (7,), (128, 128, 128))])
def test_tanh_within_the_bound_of_its_own_weights(n, C, K, fdtype, actor, critic):
    """The one licensed difference: the device's float tanh.  A wrong index, bias or activation errs by about 0.1; the bound is about 6e-6
    for two hidden layers.  And the plants whose outputs are finite are exactly the plants whose features are finite."""
    A = 3
    env = _env(n, C, K, fdtype, A, F32, stamp=True)
    a, c, log_std = _weights(5 * n, K * C, A, actor, critic)
    env.set_policy(a, c, log_std, activation="tanh", deterministic=True)
    bound_a, bound_c = _tanh_bound(a), _tanh_bound(c)
    assert bound_a < 4e-5 and bound_c < 4e-5
    P = _statement(env)
    bad = [p for p in (0, 31, 40) if p < n]
    for t in range(3):
        if t == 1:
            v = _np(env.get_field(*STAMP))
            v[bad] = [np.nan, np.inf, -np.inf][:len(bad)]
            env.set_field(STAMP[0], v, STAMP[1], STAMP[2])
        if t == 2:      # the poked frame is in the stack now (the step wrote it behind itself)
            assert (~np.isfinite(_np(env.features())).reshape(n, -1).all(axis=1)).sum() == len(bad)
        before = _np(env.features())
        finite = np.isfinite(before.astype(np.float32)).reshape(n, -1).all(axis=1)
        obs, rew, done, info = _step(env, t)
        act, value, logp = P.step(before)
        got_act, got_value, got_logp = _np(env.controls_input()), _np(info["value"]), _np(info["logp"])
        assert np.array_equal(np.isfinite(got_act).all(axis=1), finite) and np.array_equal(np.isfinite(got_value), finite)
        assert np.array_equal(np.isfinite(got_logp), finite)
        assert np.isnan(got_act[~finite]).all() and np.isnan(got_value[~finite]).all() and np.isnan(got_logp[~finite]).all()
        err_a = np.abs(got_act[finite].astype(np.float64) - act[finite]).max()
        err_c = np.abs(got_value[finite].astype(np.float64) - value[finite]).max()
        print("tanh t=%d: actor err %.3e (bound %.3e), critic err %.3e (bound %.3e)" % (t, err_a, bound_a, err_c, bound_c))
        assert err_a <= bound_a and err_c <= bound_c, (t, err_a, bound_a, err_c, bound_c)
        _same(got_logp[finite], logp[finite], (t, "logp"))      # (deterministic: the nets do not enter it)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def _sampling_env(n, first=0, first_plant=0, seed=11, **kw):
    env = _env(n, 5, 3, F32, 3, F32, first=first, **kw)
    a, c, log_std = _weights(99, 15, 3, (33, 17), (7,))
    env.set_policy(a, c, log_std, activation="relu", seed=seed, first_plant=first_plant)
    return env


def _run(env, steps, t0=0, first=0):
    out = []
    for t in range(t0, t0 + steps):
        _, _, _, info = _step(env, t, first)
        out.append((_np(env.controls_input()), _np(info["value"]), _np(info["logp"])))
    return out


def _same_runs(got, want, where):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        for name, x, y in zip(("act", "value", "logp"), g, w):
            _same(x, y, (where, t, name))


def test_equal_seeds_agree_and_the_state_resumes_the_stream():
    one, two = _sampling_env(70), _sampling_env(70)
    want = _run(one, 5)
    _same_runs(_run(two, 5), want, "equal seeds")
    assert not np.array_equal(want[0][0], want[1][0])
    other = _sampling_env(70, seed=12)
    assert not np.array_equal(_run(other, 1)[0][0], want[0][0])      # the seed does enter
    three = _sampling_env(70)
    _same_runs(_run(three, 2), want[:2], "first part")
    state = three.policy_state()
    assert state["t"] == 2
    three.load_policy_state({"t": 1000})
    assert three.policy_state()["t"] == 1000
    three.load_policy_state(state)
    _same_runs(_run(three, 3, t0=2), want[2:], "resumed")
    for e in (one, two, other, three):
        e.close()


def test_a_batch_equals_its_shards():
    whole, left, right = _sampling_env(96), _sampling_env(40), _sampling_env(56, first=40, first_plant=40)
    want = _run(whole, 3)
    a, b = _run(left, 3), _run(right, 3, first=40)
    for t in range(3):
        for k, name in enumerate(("act", "value", "logp")):
            _same(np.concatenate([a[t][k], b[t][k]]), want[t][k], (t, name))
    for e in (whole, left, right):
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def _modules(net, activation=torch.nn.ReLU):
    layers = []
    for k, (W, b) in enumerate(net):
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.as_tensor(W)); lin.bias.copy_(torch.as_tensor(b))
        layers += [lin] + ([activation()] if k < len(net) - 1 else [])
    return torch.nn.Sequential(*layers)


def test_policy_load_changes_the_outputs_without_a_new_set_policy():
    n, A = 70, 3
    env = _env(n, 5, 3, F32, A, F32)
    a, c, log_std = _weights(1, 15, A, (33, 17), (7,))
    env.set_policy(_modules(a), _modules(c), torch.nn.Parameter(torch.as_tensor(log_std)), activation="relu", seed=3)      # (torch modules)
    P = _statement(env)
    _same(_np(env.policy_theta())[:-A], policy.pack(a, c, log_std)[:-A], "theta from modules")
    first = None
    for t in range(4):
        if t == 2:      # new parameters of the same shapes: a host vector in the statement's order
            a2, c2, log_std2 = _weights(2, 15, A, (33, 17), (7,))
            env.policy_load(policy.pack(a2, c2, log_std2))
            _same(env.policy_theta(), policy.pack(a2, c2, log_std2), "loaded theta")
            P.load(_np(env.policy_theta()))
        if t == 3:      # and modules again, on the device
            env.policy_load((_modules(a), _modules(c), torch.as_tensor(log_std)))
            P.load(_np(env.policy_theta()))
        z = _np(env.policy_noise(t))
        before = _np(env.features())
        _, _, _, info = _step(env, t)
        act, value, logp = P.step(before, z=z)
        _same(env.controls_input(), act, (t, "act")); _same(info["value"], value, (t, "value")); _same(info["logp"], logp, (t, "logp"))
        if t == 2:
            old = policy.Policy(15, A, (33, 17), (7,), "relu"); old.load(first); old.t = 2
            assert not np.array_equal(old.step(before, z=z)[1], value)      # the old parameters would have given something else
        first = first if first is not None else _np(env.policy_theta())
    assert env.policy_state()["t"] == 4      # the draw counter went on through the loads
    with pytest.raises(ValueError):
        env.policy_load(np.zeros(5, dtype=np.float32))
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_policy_values_feed_the_advantages():
    """last_value from the current features, final_values from the rollout's final_obs (autoreset, max_episode_steps 3, T = 8): the
    statement's bits, and rollout_advantages fed with them is rollout.advantages"""
    n, A, T = 70, 3, 8
    env = _env(n, 5, 3, F32, A, F32, autoreset=True, max_episode_steps=3)
    env.set_rollout(T, extras=2)
    a, c, log_std = _weights(4, 15, A, (33, 17), (64, 64))
    env.set_policy(a, c, log_std, activation="relu", seed=5, extras=("value", "logp"))
    P = _statement(env)
    for t in range(T):
        _step(env, t)
    r = env.rollout()
    assert r["t"] == T and (_np(r["ended"]) & 2).any() and r["final_obs"].shape[0] == n * 3
    last, final = env.policy_values(), env.policy_values(r["final_obs"])
    _same(last, P.values(_np(env.features())), "last_value")
    _same(final, P.values(_np(r["final_obs"])), "final_values")
    _same(env.policy_values(r["obs"][2].to(torch.float64)), P.values(_np(r["obs"][2])), "a double tensor, narrowed")
    _same(r["extra"][3, :, 0], P.values(_np(r["obs"][3])), "the recorded value is the critic of the recorded features")
    adv, ret = env.rollout_advantages(0.99, 0.95, values=("extra", 0), last_value=last, final_values=final)
    want_adv, want_ret = rollout.advantages(_np(r["reward"]), _np(r["ended"]), _np(r["final_row"]), values=_np(r["extra"][:, :, 0]), last_value=_np(last),
                                            final_values=_np(final), gamma=0.99, lam=0.95)
    _same(adv, want_adv, "adv"); _same(ret, want_ret, "ret")
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def _plain(n, streams=False, **kw):
    from nuclear_sim_amd.env import BatchedPlantEnv
    if streams:      # the runner's noise and profile, driven on the device per episode: no step input comes from the caller
        env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, autoreset=True, max_episode_steps=3, noise_generator="device", episode_streams=True,
                                          power_profile_steps=16)
    else:
        env = BatchedPlantEnv(n, dt=DT, **kw)
    env.set_features(_columns(5), stack=3, dtype=F32)
    env.set_controls(AXES[:3])
    return env


def _with_policy(env, T, **kw):
    env.set_rollout(T, extras=2)
    a, c, log_std = _weights(8, 15, 3, (33, 17), (7,))
    env.set_policy(a, c, log_std, activation="relu", seed=21, extras=("value", "logp"), **kw)
    return env


@pytest.mark.parametrize("streams", [False, True])
def test_collect_is_t_steps(streams):
    n, T = 70, 6
    kw = {} if streams else dict(autoreset=True, max_episode_steps=3)
    env, twin = _with_policy(_plain(n, streams, **kw), T), _with_policy(_plain(n, streams, **kw), T)
    got = env.collect(T)
    for t in range(T):
        twin.step()
    want = twin.rollout()
    assert got["t"] == want["t"] == T and env.policy_state()["t"] == twin.policy_state()["t"] == T
    for name in ("obs", "act", "extra", "reward", "ended", "episode", "final_row", "final_obs"):
        _same(got[name], want[name], name)
    assert (_np(got["ended"]) & 2).any() and _np(got["act"]).std() > 0
    _same(env.features(), twin.features(), "features behind the last step")
    _same(env.policy_outputs()["logp"], twin.policy_outputs()["logp"], "logp")
    from nuclear_sim_amd._lib import NpbError
    with pytest.raises(NpbError, match="no room"):
        env.collect(1)
    env.rollout_begin()
    with pytest.raises(NpbError, match="no room"):
        env.collect(T + 1)
    with pytest.raises(NpbError, match="policy"):
        env.step(controls=env.controls_input())
    for what in ("set_features", "set_controls"):
        with pytest.raises(NpbError, match="policy"):
            getattr(env, what)(None)
    with pytest.raises(NpbError, match="policy"):
        env.set_rollout(None)
    assert env.collect(2)["t"] == 2
    env.close(); twin.close()


def test_collect_names_its_refusals():
    from nuclear_sim_amd._lib import NpbError
    external = _with_policy(_plain(8, heat_source="external"), 4)
    with pytest.raises(NpbError, match="external"):
        external.collect(2)
    noisy = _with_policy(_plain(8, noise_enabled=True), 4)
    with pytest.raises(NpbError, match="noise"):
        noisy.collect(2)
    bare = _plain(8)
    with pytest.raises(NpbError, match="no policy"):
        bare.collect(2)
    for e in (external, noisy, bare):
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_a_nan_feature_poisons_its_plant_alone():
    """relu turns a NaN into +0.0: the rule is the statement's own, and the other plants keep their bits"""
    n, A, bad = 70, 3, 37
    env, twin = (_env(n, 5, 3, F64, A, F64, stamp=True) for _ in range(2))
    a, c, log_std = _weights(6, 15, A, (33, 17), (7,))
    for e in (env, twin):
        e.set_policy(a, c, log_std, activation="relu", seed=9)
    v = _np(env.get_field(*STAMP))
    v[bad] = np.nan
    env.set_field(STAMP[0], v, STAMP[1], STAMP[2])
    others = np.arange(n) != bad
    for t in range(2):
        _step(env, t); _step(twin, t)
    # the poked frame entered the stack behind step 0: step 1's launch read it
    assert np.isnan(_np(env.features())[bad]).any() and np.isfinite(_np(env.features())[others]).all()
    for name, g, w in (("act", env.controls_input(), twin.controls_input()), ("value", env.policy_outputs()["value"], twin.policy_outputs()["value"]),
                       ("logp", env.policy_outputs()["logp"], twin.policy_outputs()["logp"])):
        g, w = _np(g), _np(w)
        assert np.isnan(g[bad]).all() and np.isfinite(w).all(), name
        _same(g[others], w[others], name)
    env.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- 9
def test_a_handle_without_a_policy_steps_as_before():
    """a golden replay of the parity suite on this build, and a twin that takes the policy's actions by hand: the step does not know who
    wrote the controls"""
    from test_gpu_parity import _replay_golden
    _replay_golden("s2_reactor_actions", 0)
    n, A = 70, 3
    env, twin = _env(n, 5, 3, F32, A, F32), _env(n, 5, 3, F32, A, F32)
    a, c, log_std = _weights(6, 15, A, (33, 17), (7,))
    env.set_policy(a, c, log_std, activation="tanh", seed=9)
    twin.features()      # (a step with a policy primes the features first, as one with a rollout does: the twin's stack starts the same way)
    for t in range(3):
        obs, rew, done, info = _step(env, t)
        two = twin.step(power_setpoint=_setpoint(t, n), controls=env.controls_input().clone())
        _same(obs, two[0], (t, "obs")); _same(rew, two[1], (t, "reward")); _same(info["features"], two[3]["features"], (t, "features"))
        assert "value" not in two[3]
    env.close(); twin.close()
