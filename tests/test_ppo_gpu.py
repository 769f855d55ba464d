"""GPU: training the policy on the device (npb_policy_grad, npb_policy_adam, npb_policy_update; BatchedPlantEnv.policy_grad, policy_adam,
policy_train) against nuclear_sim_amd.ppo, the numpy statement.  A relu net is compared by bits: logp_new and value_new as they are, the
ratio within 4 ulp of numpy's (OpenCL's 3 ulp for a double exp and numpy's own 1), and gradient and statistics by bits once the statement
is fed the device's ratio.  Adam's m, v and theta by bits when fed the device's gradient, std within 1 float ulp (the device's exp).  A tanh
net's gradient may stand 8 times as far from the float64 evaluation as the statement's does: the device's float tanh is licensed 5 ulp
where the statement's is 0.5.  Measured on an MI355X: the factors are in DESIGN.md.

The minibatches are explicit tensors, so the row count is free of the env's size; the shapes are the forward suite's: counts 1, 33, 257 and
300 with chains of 32, 64 and 256 (one row, one more than a tile, several chains with a short last one); 15, 64 and 256 cells; widths (7,),
(33, 17), (64, 64) and (128, 128, 128); 1, 3 and 8 axes; float and double obs, act and adv.

These layers have one ragged 32 x 32 block at most, every setting is the default (HYPER) and Adam runs its first two steps from zero.
test_policy_shapes_gpu.py goes where the kernels have further logic, through this file's bodies (_hold_relu, _hold_tanh) and its
contracts: the shape table -- a 65 cells, widths 64 (the large build by the cells alone); b 64 cells, (65,) / (7,) and c (7,) / (65,)
(by one net's width alone; out_pad 96, the back pass writing k up to 68); d 100 cells, (100, 96) / (127,), 5 axes (four k-blocks, the
last with 4 live columns, three full j-blocks, odd A); e 255 cells, (128,) / (1,), 7 axes (A4 = 8, a width of 1); f 66 cells, (31, 32,
33) / (3, 2, 1), 6 axes -- each at 70 rows in chains of 32 and 97 rows in chains of 64; and on row b other values of clip, vf_coef
and ent_coef, both branches of the norm clip, poisoned rows at the tile seams, and Adam from loaded states (steps 0 to 10 000 000),
with other betas, eps and lr, on exact zeros and three times in a row."""
import numpy as np
import pytest
import torch

from nuclear_sim_amd import policy, ppo
from test_policy_gpu import F32, F64, _env, _np, _plain, _same, _weights
from test_ppo_cpu import CLIP, ENT, VF, autograd, pooled, split

pytestmark = pytest.mark.gpu

HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5)
_NP = {F32: np.float32, F64: np.float64}


def _batch(seed, theta, count, S, activation, obs_dtype, act_dtype, adv_dtype):
    """rows whose actions scatter around the policy's own means and whose logp_old is that of the unscattered draw: the ratios scatter
    around 1 and some rows are clipped"""
    rng = np.random.default_rng(seed)
    a_net, _, log_std, std = policy.unpack(theta, S["cells"], S["n_axes"], S["actor"], S["critic"])
    obs = rng.standard_normal((count, S["cells"])).astype(_NP[obs_dtype])
    z = rng.standard_normal((count, S["n_axes"]))
    mean = policy.forward(a_net, obs, activation)
    _, _, logp = policy.outputs(mean, np.zeros(count, np.float32), log_std, std, z, obs)
    act = (mean.astype(np.float64) + std.astype(np.float64) * (z + 0.15 * rng.standard_normal(z.shape))).astype(_NP[act_dtype])
    return {"obs": obs, "act": act, "logp_old": logp, "adv": rng.standard_normal(count).astype(_NP[adv_dtype]),
            "ret": rng.standard_normal(count).astype(_NP[adv_dtype])}


def _to(env, batch):
    return {k: torch.as_tensor(v).to(env.device) for k, v in batch.items()}


def _statement(env, batch, chain, ratio=None, **hyper):
    S = env.policy_spec()
    kw = dict(HYPER, **hyper)
    return ppo.gradient(_np(env.policy_theta()), S["cells"], S["n_axes"], S["actor"], S["critic"], S["activation"], rows_per_chain=chain, ratio=ratio,
                        **batch, **kw)


def _stats(out):
    return np.array([out["stats"][k] for k in ppo.STATS])


def _policy(C, K, fdtype, actor, critic, A, cdtype, activation, seed, n=4):
    env = _env(n, C, K, fdtype, A, cdtype)
    a, c, log_std = _weights(seed, K * C, A, actor, critic)
    env.set_policy(a, c, log_std, activation=activation, deterministic=True)
    return env


# ---------------------------------------------------------------------------------------------------------------- 1
CASES = [(1, 32, 5, 3, F32, (7,), (7,), 1, F32, F32), (33, 32, 16, 4, F64, (64, 64), (33, 17), 3, F64, F64),
         (257, 64, 64, 4, F32, (128, 128, 128), (128, 128, 128), 8, F32, F32), (300, 256, 5, 3, F32, (33, 17), (64, 64), 3, F32, F64),
         (257, 32, 16, 4, F64, (7,), (64, 64), 8, F64, F32), (300, 64, 16, 4, F32, (64, 64), (64, 64), 1, F32, F32)]


def _hold_relu(env, batch, chain, **hyper):
    """the relu contract on one minibatch: logp_new and value_new by bits, the ratio within 4 ulp of numpy's, gradient and statistics by
    bits once the statement is fed the device's ratio; returns the device's outputs, that statement and the largest ratio ulp"""
    A = env.policy_spec()["n_axes"]
    got = env.policy_grad(_to(env, batch), rows_per_chain=chain, diagnostics=True, **dict(HYPER, **hyper))
    own = _statement(env, batch, chain, **hyper)
    _same(got["logp_new"], own["logp_new"], "logp_new"); _same(got["value_new"], own["value_new"], "value_new")
    ratio = _np(got["ratio"])
    ulps = np.abs(ratio - own["ratio"]) / np.spacing(own["ratio"])
    print("the ratio: at most %.1f ulp from numpy's" % ulps.max())
    assert ulps.max() <= 4
    want = _statement(env, batch, chain, ratio=ratio, **hyper)
    _same(got["grad"], want["grad"], "grad"); _same(got["stats"], _stats(want), "stats")
    assert np.isfinite(want["grad"]).all() and want["grad"][:-A].any() and want["stats"]["skipped"] == 0
    if len(batch["adv"]) > 32:
        assert 0.02 < want["stats"]["clip_fraction"] < 0.98      # (both branches of the clip are taken)
    return got, want, ulps.max()


@pytest.mark.parametrize("count, chain, C, K, fdtype, actor, critic, A, cdtype, adtype", CASES)
def test_relu_gradient_and_statistics_bit_for_bit(count, chain, C, K, fdtype, actor, critic, A, cdtype, adtype):
    """Fails without the feature: policy_grad does not exist"""
    env = _policy(C, K, fdtype, actor, critic, A, cdtype, "relu", count + C)
    batch = _batch(count, _np(env.policy_theta()), count, env.policy_spec(), "relu", fdtype, cdtype, adtype)
    _hold_relu(env, batch, chain)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def test_no_bit_depends_on_the_launch_geometry():
    env = _policy(5, 3, F32, (33, 17), (64, 64), 3, F32, "relu", 5)
    batch = _to(env, _batch(2, _np(env.policy_theta()), 300, env.policy_spec(), "relu", F32, F32, F32))
    outs = [env.policy_grad(batch, rows_per_chain=32, max_blocks=b, diagnostics=True, **HYPER) for b in (1, 2, 0)]
    for o in outs[1:]:
        for k in ("grad", "stats", "ratio", "logp_new", "value_new"):
            _same(o[k], outs[0][k], k)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_a_whole_iteration_on_70_plants():
    """collect, advantages, one epoch of two minibatches through policy_train: m, v and theta are ppo.adam's bits fed the device's own
    gradients, std within 1 float ulp, and the next step runs the new parameters (the repack ran)"""
    n, A, T = 70, 3, 4
    env = _plain(n)      # (no step input comes from the caller: collect() runs)
    env.set_rollout(T, extras=2)
    a, c, log_std = _weights(8, 15, A, (33, 17), (7,))
    env.set_policy(a, c, log_std, activation="relu", seed=21, extras=("value", "logp"))
    S = env.policy_spec()
    theta0 = _np(env.policy_theta())
    env.collect(T)
    env.rollout_advantages(0.99, 0.95, values=("extra", 0), last_value=env.policy_values())
    lr, B = 1e-3, 140
    # the two minibatches by hand: gradient and Adam on the device, and Adam in numpy fed the device's gradient and its std
    theta, m, v, step = theta0, np.zeros_like(theta0), np.zeros_like(theta0), 0
    by_hand = []
    for batch in env.rollout_minibatches(B, 1, seed=3):
        host = {k: _np(batch[k]) for k in ("act", "adv", "ret")}
        host["obs"], host["logp_old"] = _np(batch["obs"]).reshape(len(host["adv"]), -1), _np(batch["extra"])[:, 1]
        got = env.policy_grad(batch, rows_per_chain=64, diagnostics=True, **HYPER)
        want = ppo.gradient(theta, S["cells"], A, S["actor"], S["critic"], "relu", rows_per_chain=64, ratio=_np(got["ratio"]), **host, **HYPER)
        _same(got["grad"], want["grad"], "grad of a gathered minibatch")
        env.policy_adam(lr=lr)
        now = _np(env.policy_theta())
        std_want = np.exp(now[-2 * A:-A].astype(np.float64)).astype(np.float32)
        assert (np.abs(now[-A:] - std_want) <= np.spacing(std_want)).all()
        theta, m, v, step = ppo.adam(theta, m, v, step, _np(got["grad"]), A, lr=lr, std=now[-A:])
        _same(now, theta, "theta behind Adam")
        by_hand.append(_np(got["stats"]))
    state = env.policy_optimizer_state()
    assert state["step"] == 2
    _same(state["m"], m, "m"); _same(state["v"], v, "v")
    assert not np.array_equal(theta[:-2 * A], theta0[:-2 * A])
    # and policy_train from the same start is those two updates
    env.policy_load(theta0)
    env.load_policy_optimizer_state({"m": np.zeros_like(m), "v": np.zeros_like(v), "step": 0})
    stats = env.policy_train(B, 1, seed=3, rows_per_chain=64, lr=lr, **HYPER)
    assert stats.shape == (2, 8) and stats.device == env.device
    _same(stats, np.stack(by_hand), "the updates' stats")
    state = env.policy_optimizer_state()
    now = _np(env.policy_theta())
    assert state["step"] == 2
    _same(state["m"], m, "m"); _same(state["v"], v, "v"); _same(now, theta, "theta")
    # the next deterministic step is the statement's with the new theta
    env.rollout_begin()
    P = policy.Policy(S["cells"], A, S["actor"], S["critic"], "relu", S["seed"], False, 0, np.float32)
    P.load(now)
    P.t = int(env.policy_state()["t"])
    before, z = _np(env.features()), _np(env.policy_noise(P.t))
    env.step()
    act, value, logp = P.step(before, z=z)
    _same(env.controls_input(), act, "act"); _same(env.policy_outputs()["value"], value, "value"); _same(env.policy_outputs()["logp"], logp, "logp")
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def _hold_tanh(env, batch, chain):
    """the tanh contract on one minibatch, max_grad_norm 0: the device's pooled distance from float64 autograd is at most 8 times the
    statement's own; returns (the device's, the statement's)"""
    S, theta = env.policy_spec(), _np(env.policy_theta())
    A = S["n_axes"]
    hyper = dict(HYPER, max_grad_norm=0.0)
    got = env.policy_grad(_to(env, batch), rows_per_chain=chain, diagnostics=True, **hyper)
    own = _statement(env, batch, chain, max_grad_norm=0.0)
    assert (HYPER["clip"], HYPER["vf_coef"], HYPER["ent_coef"]) == (CLIP, VF, ENT)      # (the loss `autograd` differentiates)
    g64, r = autograd(theta, S["cells"], A, S["actor"], S["critic"], "tanh", batch, torch.float64)
    near = min(np.abs(r - 1.2).min(), np.abs(r - 0.8).min())
    print("nearest ratio to a clip boundary: %.2e" % near)
    assert near > 1e-4
    cut = lambda g: split(g, S["cells"], A, S["actor"], S["critic"])
    mine, yard = pooled(cut(_np(got["grad"])), g64), pooled(cut(own["grad"]), g64)
    print("pooled distance from float64: the device %.3e, the statement %.3e, factor %.2f" % (mine, yard, mine / yard))
    assert mine <= 8 * yard
    return mine, yard


@pytest.mark.parametrize("count, chain, C, K, actor, critic, A", [(300, 64, 5, 3, (33, 17), (33, 17), 3), (257, 256, 16, 4, (64, 64), (128, 128, 128), 8)])
def test_tanh_gradient_within_8_times_the_statements_distance_from_float64(count, chain, C, K, actor, critic, A):
    env = _policy(C, K, F32, actor, critic, A, F32, "tanh", 3 * count)
    batch = _batch(count + 1, _np(env.policy_theta()), count, env.policy_spec(), "tanh", F32, F32, F32)
    _hold_tanh(env, batch, chain)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_poisoned_rows_are_skipped_and_counted():
    env = _policy(5, 3, F64, (33, 17), (7,), 3, F64, "relu", 9)
    batch = _batch(4, _np(env.policy_theta()), 100, env.policy_spec(), "relu", F64, F64, F64)
    clean = env.policy_grad(_to(env, batch), rows_per_chain=32, diagnostics=True, **HYPER)
    value = _np(clean["value_new"])
    dirty = {k: v.copy() for k, v in batch.items()}
    rows = {"obs": 3, "act": 34, "logp_old": 35, "adv": 64, "ret": 99}
    dirty["obs"][3, 7], dirty["act"][34, 2], dirty["logp_old"][35], dirty["adv"][64], dirty["ret"][99] = np.nan, np.inf, np.nan, -np.inf, np.nan
    got = env.policy_grad(_to(env, dirty), rows_per_chain=32, diagnostics=True, **HYPER)
    stats = _np(got["stats"])
    assert stats[ppo.STATS.index("skipped")] == 5 and stats[ppo.STATS.index("count")] == 100
    assert np.isfinite(_np(got["grad"])).all() and np.isfinite(stats).all()
    bad = sorted(rows.values())
    for k in ("ratio", "logp_new", "value_new"):
        x = _np(got[k])
        assert np.isnan(x[bad]).all() and np.isfinite(np.delete(x, bad)).all(), k
    want = _statement(env, dirty, 32, ratio=_np(got["ratio"]))
    _same(got["grad"], want["grad"], "grad"); _same(got["stats"], _stats(want), "stats")
    # the same bits as the batch with those rows' seeds zeroed: no advantage, and the return the critic's own value
    zeroed = {k: v.copy() for k, v in batch.items()}
    zeroed["adv"][bad], zeroed["ret"][bad] = 0.0, value[bad].astype(np.float64)
    same = env.policy_grad(_to(env, zeroed), rows_per_chain=32, **HYPER)
    _same(got["grad"], same["grad"], "the gradient with the seeds zeroed")
    assert not np.array_equal(_np(got["grad"]), _np(clean["grad"]))
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_a_twin_that_forms_gradients_between_steps_steps_to_the_same_bits():
    n, A = 70, 3
    env, twin = _env(n, 5, 3, F32, A, F32), _env(n, 5, 3, F32, A, F32)
    a, c, log_std = _weights(6, 15, A, (33, 17), (7,))
    for e in (env, twin):
        e.set_policy(a, c, log_std, activation="relu", seed=9)
    batch = _to(env, _batch(1, _np(env.policy_theta()), 70, env.policy_spec(), "relu", F32, F32, F32))
    for t in range(3):
        one, two = env.step(), twin.step()
        env.policy_grad(batch, **HYPER)
        _same(one[0], two[0], (t, "obs")); _same(one[1], two[1], (t, "reward"))
        _same(env.controls_input(), twin.controls_input(), (t, "act")); _same(env.policy_outputs()["logp"], twin.policy_outputs()["logp"], (t, "logp"))
    _same(env.policy_theta(), twin.policy_theta(), "theta")
    env.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_lifecycle_and_refusals():
    from nuclear_sim_amd._lib import NpbError
    env = _policy(5, 3, F32, (7,), (7,), 3, F32, "relu", 2)
    batch = _to(env, _batch(1, _np(env.policy_theta()), 40, env.policy_spec(), "relu", F32, F32, F32))
    with pytest.raises(NpbError, match="no gradient formed yet"):
        env.policy_adam()
    theta0 = _np(env.policy_theta())
    env.policy_grad(batch, **HYPER)
    _same(env.policy_theta(), theta0, "a gradient moves nothing")
    env.policy_adam(lr=1e-2)
    env.policy_grad(batch, **HYPER)
    env.policy_adam(lr=1e-2)
    state = env.policy_optimizer_state()
    assert state["step"] == 2 and state["m"].any() and state["v"].any() and not np.array_equal(_np(env.policy_theta()), theta0)
    env.load_policy_optimizer_state({"m": state["m"] * 2, "v": state["v"] * 3, "step": 7})
    back = env.policy_optimizer_state()
    _same(back["m"], state["m"] * 2, "m"); _same(back["v"], state["v"] * 3, "v")
    assert back["step"] == 7
    for kw, words in ((dict(rows_per_chain=48), "multiple of 32"), (dict(clip=1.0), r"\(0, 1\)"), (dict(clip=0.0), r"\(0, 1\)")):
        with pytest.raises(NpbError, match=words):
            env.policy_grad(batch, **dict(HYPER, **kw))
    # a policy set again starts from nothing: the optimiser's state went with the old one
    a, c, log_std = _weights(2, 15, 3, (7,), (7,))
    env.set_policy(None)
    with pytest.raises(NpbError, match="no policy"):
        env.policy_grad(batch, **HYPER)
    with pytest.raises(NpbError, match="no policy"):
        env.policy_adam()
    with pytest.raises(NpbError, match="no policy"):
        env.policy_optimizer_state()
    assert env.L.npb_policy_adam(env._h, 1e-3, 0.9, 0.999, 1e-5, None) != 0 and b"npb_policy_adam: no policy set" in env.L.npb_last_error(env._h)
    env.set_policy(a, c, log_std, activation="relu", deterministic=True)
    fresh = env.policy_optimizer_state()
    assert fresh["step"] == 0 and not fresh["m"].any() and not fresh["v"].any()
    env.close()
