"""GPU: the options of the policy's training step on the device (npb_policy_grad_more, npb_policy_update_more, npb_policy_train_begin /
_end, npb_policy_get_stats_more; BatchedPlantEnv.policy_grad(clip_vf=, value_old=) and policy_train(clip_vf=, target_kl=, more=, lr=))
against nuclear_sim_amd.ppo, the numpy statement, by the contracts of tests/test_ppo_gpu.py: a relu net by bits once the statement is fed
the device's ratio; a tanh net's gradient at most 8 times as far from the float64 evaluation as the statement's own (that file's rule and
its factor, _hold_tanh).

The value-clip inputs are those of tests/test_ppo_options_cpu.py (vf_inputs: every class of the clipped epilogue, far from its
boundaries), with the class counts asserted on the statement before the device runs.  The shapes: 24 cells, (64, 64) / (33, 17), 3 axes
(the small LDS build) and 65 cells, (64,) / (64,), 2 axes (one cell past it: the large build); counts 1, 33, 70 and 257 in chains of 32
and 64 (one row; one more than a tile; a short last chain; several chains)."""
import ctypes

import numpy as np
import pytest
import torch

from nuclear_sim_amd import _lib, ppo
from test_policy_gpu import F32, F64, _np, _plain, _same, _weights
from test_ppo_cpu import pooled, split
from test_ppo_gpu import HYPER, _batch, _policy, _statement, _stats, _to
from test_ppo_options_cpu import CLIP_VF, autograd_vf, forward_value, hold_classes, vf_inputs

pytestmark = pytest.mark.gpu

SMALL = dict(C=8, K=3, actor=(64, 64), critic=(33, 17), A=3)      # 24 cells
LARGE = dict(C=13, K=5, actor=(64,), critic=(64,), A=2)           # 65 cells
_NP = {F32: np.float32, F64: np.float64}


def _more(out):
    return np.array([out["more"][k] for k in ppo.STATS_MORE])


def _clip_case(shape, count, activation, adtype, seed, poison=True):
    """the env with its policy, the batch with returns of every class, the old values (two of them not finite when ``poison``)"""
    env = _policy(shape["C"], shape["K"], F32, shape["actor"], shape["critic"], shape["A"], F32, activation, seed)
    S, theta = env.policy_spec(), _np(env.policy_theta())
    batch = _batch(seed + 1, theta, count, S, activation, F32, F32, adtype)
    v = forward_value(theta, S["cells"], S["n_axes"], S["actor"], S["critic"], activation, batch["obs"])
    value_old, batch["ret"] = vf_inputs(np.random.default_rng(seed + 2), v, CLIP_VF, _NP[adtype])
    bad = []
    if poison and count >= 33:
        bad = [7, count - 1]
        value_old[7], value_old[count - 1] = np.nan, np.inf
    return env, batch, value_old, bad


# ---------------------------------------------------------------------------------------------------------------- 1: value-loss clipping
RELU_CASES = [(1, 32, SMALL, F32), (33, 32, LARGE, F64), (70, 64, SMALL, F64), (70, 32, LARGE, F32), (257, 64, LARGE, F32), (257, 32, SMALL, F32),
              (33, 64, SMALL, F32), (257, 64, SMALL, F64)]


@pytest.mark.parametrize("count, chain, shape, adtype", RELU_CASES, ids=["%d-%d-%s-%s" % (c, r, "small" if s is SMALL else "large", str(a)[-2:])
                                                                         for c, r, s, a in RELU_CASES])
def test_relu_clipped_value_loss_bit_for_bit(count, chain, shape, adtype):
    """Fails without the feature: policy_grad takes no clip_vf"""
    env, batch, value_old, bad = _clip_case(shape, count, "relu", adtype, 3 * count + chain)
    own = _statement(env, batch, chain, value_old=value_old, clip_vf=CLIP_VF)
    counts = hold_classes(own["rows"], value_old, batch["ret"])
    print("rows per class:", counts)
    assert own["stats"]["skipped"] == len(bad)
    got = env.policy_grad(_to(env, batch), rows_per_chain=chain, diagnostics=True, clip_vf=CLIP_VF, value_old=torch.as_tensor(value_old), **HYPER)
    _same(got["value_new"], own["value_new"], "value_new")
    assert np.flatnonzero(np.isnan(_np(got["value_new"]))).tolist() == bad
    want = _statement(env, batch, chain, ratio=_np(got["ratio"]), value_old=value_old, clip_vf=CLIP_VF)
    _same(got["grad"], want["grad"], "grad"); _same(got["stats"], _stats(want), "stats")
    _same(got["more"][:2], _more(want)[:2], "vf_clip_fraction and explained_variance")
    assert _np(got["more"])[2:].tolist() == [1.0, 0.0]
    live = count - len(bad)
    assert want["more"]["vf_clip_fraction"] == (live - counts["inside"]) / count and np.isfinite(want["grad"]).all()
    # the clipping did something: with rows whose clipped square is the larger, the plain call's gradient differs
    plain = env.policy_grad(_to(env, batch), rows_per_chain=chain, **HYPER)
    assert np.array_equal(_np(plain["grad"]), _np(got["grad"])) == (counts["below_use"] + counts["above_use"] == 0) and _np(plain["more"])[0] == 0.0
    env.close()


def test_clipped_value_loss_no_bit_depends_on_the_launch_geometry():
    env, batch, value_old, _ = _clip_case(SMALL, 257, "relu", F32, 11)
    dev, vo = _to(env, batch), torch.as_tensor(value_old)
    outs = [env.policy_grad(dev, rows_per_chain=32, max_blocks=b, diagnostics=True, clip_vf=CLIP_VF, value_old=vo, **HYPER) for b in (1, 2, 0)]
    for o in outs[1:]:
        for k in ("grad", "stats", "more", "ratio", "logp_new", "value_new"):
            _same(o[k], outs[0][k], k)
    env.close()


@pytest.mark.parametrize("count, chain, shape, adtype", [(70, 32, SMALL, F32), (257, 64, LARGE, F64)], ids=["70-32-small", "257-64-large"])
def test_tanh_clipped_value_loss_within_8_times_the_statements_distance_from_float64(count, chain, shape, adtype):
    env, batch, value_old, _ = _clip_case(shape, count, "tanh", adtype, 5 * count, poison=False)
    S, theta = env.policy_spec(), _np(env.policy_theta())
    A = S["n_axes"]
    own = _statement(env, batch, chain, max_grad_norm=0.0, value_old=value_old, clip_vf=CLIP_VF)
    hold_classes(own["rows"], value_old, batch["ret"])
    got = env.policy_grad(_to(env, batch), rows_per_chain=chain, diagnostics=True, clip_vf=CLIP_VF, value_old=torch.as_tensor(value_old),
                          **dict(HYPER, max_grad_norm=0.0))
    g64, r = autograd_vf(theta, S["cells"], A, S["actor"], S["critic"], "tanh", batch, value_old, CLIP_VF, torch.float64)
    assert min(np.abs(r - 1.2).min(), np.abs(r - 0.8).min()) > 1e-4
    cut = lambda g: split(g, S["cells"], A, S["actor"], S["critic"])
    mine, yard = pooled(cut(_np(got["grad"])), g64), pooled(cut(own["grad"]), g64)
    print("pooled distance from float64: the device %.3e, the statement %.3e, factor %.2f" % (mine, yard, mine / yard))
    assert mine <= 8 * yard
    # the device's value stands within the float tanh's licence of the statement's, far inside the classes' margins: the same rows are clipped
    assert _np(got["more"])[0] == own["more"]["vf_clip_fraction"]
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2: off is off
def test_with_clip_vf_zero_the_old_values_are_not_read():
    env, batch, value_old, _ = _clip_case(SMALL, 70, "relu", F32, 2, poison=False)
    dev = _to(env, batch)
    plain = env.policy_grad(dev, rows_per_chain=32, diagnostics=True, **HYPER)
    off = env.policy_grad(dev, rows_per_chain=32, diagnostics=True, clip_vf=0.0, value_old=torch.full((70,), float("nan")), **HYPER)
    for k in ("grad", "stats", "more", "ratio", "logp_new", "value_new"):
        _same(off[k], plain[k], k)
    # and the library's own entry point with the options' struct: clip_vf 0 and a pointer to NaNs
    d, held = env._ppo_desc(dev, rows_per_chain=32, max_blocks=0, **HYPER)
    nans = torch.full((70,), float("nan"), dtype=F32, device=env.device)
    more = _lib.NpbPpoMore()
    more.value_old, more.clip_vf, more.kl_limit = nans.data_ptr(), 0.0, 0.0
    grad, stats, extra = torch.zeros_like(plain["grad"]), torch.zeros_like(plain["stats"]), torch.zeros_like(plain["more"])
    _lib.check(env.L.npb_policy_grad_more(env._h, ctypes.byref(d), ctypes.byref(more), env._stream()), env._h)
    for call, out in ((env.L.npb_policy_get_grad, grad), (env.L.npb_policy_get_stats, stats), (env.L.npb_policy_get_stats_more, extra)):
        _lib.check(call(env._h, ctypes.c_void_p(out.data_ptr()), env._stream()), env._h)
    _same(grad, plain["grad"], "grad"); _same(stats, plain["stats"], "stats"); _same(extra, plain["more"], "more")
    del held
    want = _statement(env, batch, 32, ratio=_np(plain["ratio"]))
    _same(plain["grad"], want["grad"], "grad"); _same(plain["stats"], _stats(want), "stats")
    _same(plain["more"], _more(want), "more")
    assert np.isfinite(want["more"]["explained_variance"]) and want["more"]["vf_clip_fraction"] == 0.0
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3: the gate
# The settings under which approx_kl rises from update to update.  Under Adam's default eps every parameter moves by about lr an update
# whatever its gradient, the minibatches' noise included, and approx_kl goes up and down (measured on an MI355X at lr 1e-3: 3.4e-3, 2.5e-3,
# 3.4e-3; no lr from 3e-4 to 1e-2 made it rise).  With eps = 1 Adam is momentum SGD on the norm-clipped gradient, and ent_coef = 2 gives
# log_std a gradient of one sign in every update: the policy moves one way (measured: 5e-15, 1.6e-2, 2.2e-2, 5.2e-2).
N, A, T, B, LR, PLAIN_LR = 70, 3, 8, 280, 1.0, 1e-3
GATE = dict(ent_coef=2.0, eps=1.0)


def _rolled():
    """70 plants, relu, one rollout of 8 steps with its advantages: the same bits on every call"""
    env = _plain(N)
    env.set_rollout(T, extras=2)
    a, c, log_std = _weights(8, 15, A, (33, 17), (7,))
    env.set_policy(a, c, log_std, activation="relu", seed=21, extras=("value", "logp"))
    env.collect(T)
    env.rollout_advantages(0.99, 0.95, values=("extra", 0), last_value=env.policy_values())
    return env


def _train(env, epochs=2, **kw):
    stats, more = env.policy_train(B, epochs, seed=3, more=True, **dict(dict(HYPER, lr=LR, **GATE), **kw))
    return _np(stats), _np(more)


def _state(env):
    s = env.policy_optimizer_state()
    return _np(env.policy_theta()), s["m"], s["v"], int(s["step"])


_UNGATED = {}


def _ungated():
    """the ungated run of four updates, once: its stats, more and final state"""
    if not _UNGATED:
        env = _rolled()
        stats, more = _train(env)
        _UNGATED.update(stats=stats, more=more, state=_state(env))
        env.close()
        kl = stats[:, ppo.STATS.index("approx_kl")]
        print("approx_kl of the four updates:", kl)
        assert stats.shape == (4, 8) and more.shape == (4, 4)
        assert (np.diff(kl) > 0).all() and (np.diff(kl) > 1e-3 * kl[1:]).all(), kl
        assert more[:, 2].tolist() == [1, 1, 1, 1] and more[:, 3].tolist() == [0, 0, 0, 0] and _UNGATED["state"][3] == 4
    return _UNGATED


def test_the_gate_stops_the_third_update_and_the_step_counts_two():
    """Fails without the feature: policy_train takes no target_kl"""
    free = _ungated()
    kl = free["stats"][:, ppo.STATS.index("approx_kl")]
    target_kl = (0.5 * (kl[1] + kl[2])) / 1.5
    assert kl[1] < 1.5 * target_kl < kl[2]
    env = _rolled()
    stats, more = _train(env, target_kl=target_kl)
    assert more[:, 2].tolist() == [1, 1, 0, 0] and more[:, 3].tolist() == [0, 0, 1, 1]
    _same(stats[:3], free["stats"][:3], "the stats of the updates up to the one that stopped")
    assert np.isfinite(stats[3]).all() and not np.array_equal(stats[3], free["stats"][3])      # (formed, at the theta that was kept)
    theta, m, v, step = _state(env)
    assert step == 2
    two = _rolled()      # the ungated run stopped behind its second update: one epoch
    _train(two, epochs=1)
    theta2, m2, v2, step2 = _state(two)
    two.close()
    assert step2 == 2
    _same(theta, theta2, "theta"); _same(m, m2, "m"); _same(v, v2, "v")
    assert not np.array_equal(theta, free["state"][0])
    # an ungated update behind it is Adam's step 3
    batch = next(iter(env.rollout_minibatches(N * T, 1, seed=9)))
    grad = _np(env.policy_grad(batch, **HYPER)["grad"])
    _same(env.policy_theta(), theta, "a gradient moves nothing")
    one = env.policy_train(N * T, 1, seed=9, lr=PLAIN_LR, **HYPER)
    assert one.shape == (1, 8)
    now, m3, v3, step3 = _state(env)
    want = ppo.adam(theta, m, v, 2, grad, A, lr=PLAIN_LR, std=now[-A:])
    assert step3 == 3 == want[3]
    _same(now, want[0], "theta behind step 3"); _same(m3, want[1], "m"); _same(v3, want[2], "v")
    env.close()


def test_a_target_kl_above_every_approx_kl_changes_no_bit():
    free = _ungated()
    kl = free["stats"][:, ppo.STATS.index("approx_kl")]
    env = _rolled()
    stats, more = _train(env, target_kl=10.0 * kl.max())
    _same(stats, free["stats"], "stats"); _same(more, free["more"], "more")
    state = _state(env)
    assert state[3] == 4
    for got, want, name in zip(state[:3], free["state"][:3], ("theta", "m", "v")):
        _same(got, want, name)
    env.close()


def test_a_learning_rate_schedule_as_a_sequence_and_as_a_callable():
    free = _ungated()
    rates = [LR, LR / 2, LR / 4, LR / 8]
    asked = []

    def schedule(i, updates):
        asked.append((i, updates))
        return rates[i]
    outs = []
    for lr in (rates, schedule, np.array(rates), [LR] * 4):
        env = _rolled()
        stats, _ = _train(env, lr=lr)
        outs.append((stats,) + _state(env))
        env.close()
    assert asked == [(i, 4) for i in range(4)]
    for o in outs[1:3]:
        for got, want, name in zip(o, outs[0], ("stats", "theta", "m", "v")):
            _same(got, want, name)
        assert o[4] == 4
    assert not np.array_equal(outs[0][1], free["state"][0])      # (the schedule was followed)
    _same(outs[3][1], free["state"][0], "a constant sequence is the constant"); _same(outs[3][0], free["stats"], "stats")
    env = _rolled()
    with pytest.raises(ValueError, match="3 values and the call makes 4 updates"):
        env.policy_train(B, 2, seed=3, lr=rates[:3], **HYPER)
    env.close()


def test_value_clipping_through_policy_train_reads_the_rollouts_value_slot():
    """policy_train(clip_vf=) is policy_grad(clip_vf=) on the gathered minibatch with the extras' value column, then Adam.  One plain
    update first: at the rollout's own parameters every value IS its old value and nothing would be clipped"""
    env = _rolled()
    env.policy_train(N * T, 1, seed=1, lr=PLAIN_LR, **HYPER)
    theta0, m0, v0, step0 = _state(env)
    assert step0 == 1
    S = env.policy_spec()
    c = 1e-3
    batch = next(iter(env.rollout_minibatches(N * T, 1, seed=4)))
    host = {k: _np(batch[k]) for k in ("act", "adv", "ret")}
    host["obs"], host["logp_old"], old = _np(batch["obs"]).reshape(N * T, -1), _np(batch["extra"])[:, 1], _np(batch["extra"])[:, 0]
    got = env.policy_grad(batch, diagnostics=True, clip_vf=c, **HYPER)
    want = ppo.gradient(theta0, S["cells"], A, S["actor"], S["critic"], "relu", ratio=_np(got["ratio"]), value_old=old, clip_vf=c, **host, **HYPER)
    _same(got["grad"], want["grad"], "grad"); _same(got["more"][:2], _more(want)[:2], "more")
    print("vf_clip_fraction %.3f" % want["more"]["vf_clip_fraction"])
    assert 0.0 < want["more"]["vf_clip_fraction"] <= 1.0 and want["rows"]["vf_use"].any()      # (the clipped branch is taken)
    explicit = env.policy_grad(batch, clip_vf=c, value_old=batch["extra"][:, 0].clone(), **HYPER)
    _same(explicit["grad"], got["grad"], "value_old given is the slot's")
    stats, more = env.policy_train(N * T, 1, seed=4, lr=PLAIN_LR, clip_vf=c, more=True, **HYPER)
    _same(stats[0], got["stats"], "stats"); _same(more[0], got["more"], "more")
    now = _np(env.policy_theta())
    _same(now, ppo.adam(theta0, m0, v0, 1, _np(got["grad"]), A, lr=PLAIN_LR, std=now[-A:])[0], "theta")
    assert env.policy_optimizer_state()["step"] == 2
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4: refusals
def test_refusals_on_a_live_handle_leave_nothing_armed():
    from nuclear_sim_amd._lib import NpbError
    env = _policy(5, 3, F32, (7,), (7,), 3, F32, "relu", 2)      # (no rollout: the policy has no value slot)
    batch = _to(env, _batch(1, _np(env.policy_theta()), 40, env.policy_spec(), "relu", F32, F32, F32))
    env.policy_grad(batch, **HYPER)
    env.policy_adam(lr=1e-3)
    theta, m, v, step = _state(env)
    assert step == 1

    def untouched(what):
        now = _state(env)
        assert now[3] == step, what
        for got, want in zip(now[:3], (theta, m, v)):
            _same(got, want, what)
    # clip_vf > 0 with neither a value slot nor value_old: by name, in Python and in the library
    with pytest.raises(ValueError, match="clip_vf > 0 and no value_old"):
        env.policy_grad(batch, clip_vf=0.2, **HYPER)
    d, held = env._ppo_desc(batch, rows_per_chain=256, max_blocks=0, **HYPER)
    more = _lib.NpbPpoMore()
    more.clip_vf = 0.2
    assert env.L.npb_policy_grad_more(env._h, ctypes.byref(d), ctypes.byref(more), env._stream()) != 0
    assert b"npb_policy_grad_more: clip_vf > 0 and value_old is NULL" in env.L.npb_last_error(env._h)
    untouched("clip_vf without value_old")
    # a gated update outside begin / end
    more = _lib.NpbPpoMore()
    more.kl_limit = 0.03
    assert env.L.npb_policy_update_more(env._h, ctypes.byref(d), ctypes.byref(more), 1e-3, 0.9, 0.999, 1e-5, env._stream()) != 0
    assert b"npb_policy_update_more: kl_limit > 0 outside npb_policy_train_begin" in env.L.npb_last_error(env._h)
    assert env.L.npb_policy_grad_more(env._h, ctypes.byref(d), ctypes.byref(more), env._stream()) != 0
    assert b"npb_policy_grad_more: kl_limit > 0: the gate is an update's" in env.L.npb_last_error(env._h)
    applied = ctypes.c_uint32(99)
    assert env.L.npb_policy_train_end(env._h, ctypes.byref(applied), env._stream()) != 0
    assert b"npb_policy_train_end: no npb_policy_train_begin" in env.L.npb_last_error(env._h)
    untouched("a gated update outside a pair")
    # inside a pair: the optimiser's state, a lone Adam step, an ungated update and a second begin are refused; end reads 0 applied
    _lib.check(env.L.npb_policy_train_begin(env._h, env._stream()), env._h)
    with pytest.raises(NpbError, match="npb_policy_optimizer_get_state: between npb_policy_train_begin and npb_policy_train_end"):
        env.policy_optimizer_state()
    with pytest.raises(NpbError, match="npb_policy_optimizer_set_state: between"):
        env.load_policy_optimizer_state({"m": m, "v": v, "step": 5})
    with pytest.raises(NpbError, match="npb_policy_adam: between"):
        env.policy_adam()
    assert env.L.npb_policy_update(env._h, ctypes.byref(d), 1e-3, 0.9, 0.999, 1e-5, env._stream()) != 0
    assert b"npb_policy_update: kl_limit == 0 between" in env.L.npb_last_error(env._h)
    assert env.L.npb_policy_train_begin(env._h, env._stream()) != 0 and b"npb_policy_train_begin: between" in env.L.npb_last_error(env._h)
    _lib.check(env.L.npb_policy_train_end(env._h, ctypes.byref(applied), env._stream()), env._h)
    assert applied.value == 0
    untouched("an empty pair")
    env.policy_grad(batch, **HYPER)
    env.policy_adam(lr=1e-3)      # (nothing is armed: a lone step is taken again)
    assert env.policy_optimizer_state()["step"] == 2
    del held
    env.close()
    # a refusal in the middle of policy_train closes the pair
    env = _rolled()
    for kw, words in ((dict(target_kl=0.01, rows_per_chain=48), "multiple of 32"), (dict(target_kl=0.0), "target_kl"), (dict(target_kl=-1.0), "target_kl"),
                      (dict(target_kl=float("nan")), "target_kl")):
        with pytest.raises((NpbError, ValueError), match=words):
            env.policy_train(B, 1, seed=3, **dict(HYPER, **kw))
    state = env.policy_optimizer_state()
    assert state["step"] == 0 and not state["m"].any()
    env.close()
