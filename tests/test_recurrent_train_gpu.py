"""GPU: training the recurrent policy through time on the device (npb_policy_grad_seq, npb_policy_update_seq, npb_policy_shard_sums_seq;
BatchedPlantEnv.policy_grad_sequences, policy_shard_sums_sequences, policy_train(unit="plant")) against nuclear_sim_amd.recurrent's
statement.  Hard gates with relu nets are compared by bits: logp_new, value_new and hidden as they are, the ratio within 4 ulp of numpy's,
and the gradient, stats and more by bits once the statement is fed the device's ratio.  Soft gates with tanh nets may stand 8 times as far
from float64 autograd as the statement does (test_ppo_gpu.py's licence for the 5-ulp float tanh).

The minibatches are hand-made (recurrent_train_support.problem), so their shapes are free of the env's size, and every one holds an
episode-change restart, a cut restart, a restart in front of slot 0 (already in ``first``), a poisoned cell mid-sequence and a cell skipped
by a NaN adv.  Shapes: t = 5 with 33 plants (a ragged second tile) and with 70 plants in chains of 64 (two chains, the last tile 6 wide);
H in {5, 33}; once H = 65 with K * C = 65 (the large build); a shuffled index against the identity."""
import ctypes

import numpy as np
import pytest
import torch

from nuclear_sim_amd import _lib, ppo, recurrent
from recurrent_train_support import autograd, distance, problem, statement
from test_policy_gpu import AXES, DT, F32, _columns, _np, _same, _weights
from test_recurrent_gpu import _core

pytestmark = pytest.mark.gpu

HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5)
T = 5


def _setup(seed, count, C, K, H, actor, critic, gates="hard", activation="relu", n=4, A=3, t=T, cdtype=F32, P=None):
    """an env whose policy has the problem's shapes and parameters, and the problem with the device's own theta (torch formed its std).
    ``A`` axes, ``t`` slots, controls of ``cdtype`` (the type ``act`` must have); ``P``: a problem made elsewhere, in place of the seed's"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    if P is None:
        P = problem(seed, t, count, C * K, H, A, actor, critic, gates, activation)
    A = P["n_axes"]
    core, a, c, log_std, _ = recurrent.unpack(P["theta"], C * K, A, actor, critic, H)
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT)
    env.set_features(_columns(C), stack=K, dtype=F32)
    env.set_controls(AXES[:A], dtype=cdtype)
    env.set_policy(a, c, log_std, activation=activation, deterministic=True, core=core, gates=gates)
    P["theta"] = _np(env.policy_theta())
    assert np.array_equal(P["theta"][:-A].view(np.int32), recurrent.pack(a, c, log_std, core=core)[:-A].view(np.int32))
    return env, P


def _batch(env, P, shuffle=None, extra_plants=0):
    """the problem as the device takes it: the minibatch's tensors, and the 'rollout' the sequences came from -- its plants in another
    order, and more of them, when ``shuffle`` (a seed) is given: ``index`` then says where each sequence's restart words and first lie"""
    count, n, T = P["count"], P["count"] + extra_plants, P["t"]
    where = np.arange(count) if shuffle is None else np.random.default_rng(shuffle).permutation(n)[:count]
    episode, ended, first = np.full((T, n), 7, np.int32), np.full((T, n), 4, np.uint8), np.full((n, P["core"]), 0.5, np.float32)
    episode[:, where], ended[:, where], first[where] = P["episode"], P["ended"], P["first"]
    batch = {k: P[k] for k in ("obs", "act", "logp_old", "adv", "ret", "value_old")}
    batch.update(episode=episode, ended=ended, first=first)
    if shuffle is not None:
        batch["index"] = where.astype(np.int32)
    return {k: torch.as_tensor(v).to(env.device) for k, v in batch.items()}


def _array(d, names):
    return np.array([d[k] for k in names])


def _hold(env, P, chain, batch=None, valid=None, keep=False, **hyper):
    """the bit contract on one minibatch; returns the device's outputs and the statement's (``keep``: with its gate deltas)"""
    kw = dict(HYPER, **hyper)
    got = env.policy_grad_sequences(_batch(env, P) if batch is None else batch, plants_per_chain=chain, diagnostics=True, **kw)
    extra = dict(value_old=P["value_old"]) if kw.get("clip_vf") else {}
    own = statement(P, plants_per_chain=chain, valid=valid, **kw, **extra)
    _same(got["logp_new"], own["logp_new"], "logp_new"); _same(got["value_new"], own["value_new"], "value_new"); _same(got["hidden"], own["hidden"], "hidden")
    ratio = _np(got["ratio"])
    live = np.isfinite(own["ratio"])
    assert np.array_equal(np.isfinite(ratio), live)
    ulps = np.abs(ratio[live] - own["ratio"][live]) / np.spacing(own["ratio"][live])
    print("the ratio: at most %.1f ulp from numpy's" % ulps.max())
    assert ulps.max() <= 4
    want = statement(P, plants_per_chain=chain, ratio=ratio, valid=valid, keep=keep, **kw, **extra)
    _same(got["grad"], want["grad"], "grad"); _same(got["stats"], _array(want["stats"], ppo.STATS), "stats"); _same(got["more"], _array(want["more"], ppo.STATS_MORE), "more")
    n_core = recurrent.core_size(P["cells"], P["core"])
    assert np.isfinite(want["grad"]).all() and want["grad"][:n_core].any() and want["grad"][n_core:-P["n_axes"]].any()
    return got, want


CASES = [(33, 32, 5, 1, 5, (7,), (9, 6), None, 0.0), (70, 64, 5, 1, 33, (33, 17), (7,), 3, 0.0), (33, 32, 13, 5, 65, (7,), (33, 17), None, 0.2),
         (70, 64, 13, 1, 5, (64, 64), (7,), 4, 0.2)]


@pytest.mark.parametrize("count, chain, C, K, H, actor, critic, shuffle, clip_vf", CASES, ids=["33-5", "70-33-shuffled", "33-65-65-large-clipvf", "70-5-shuffled-clipvf"])
def test_hard_gates_and_relu_nets_bit_for_bit(count, chain, C, K, H, actor, critic, shuffle, clip_vf):
    """Fails without the feature: policy_grad_sequences does not exist"""
    env, P = _setup(count + H, count, C, K, H, actor, critic)
    batch = _batch(env, P, shuffle, extra_plants=0 if shuffle is None else 9)
    got, want = _hold(env, P, chain, batch, clip_vf=clip_vf)
    assert want["stats"]["skipped"] == 2 and want["stats"]["count"] == T * count
    fresh = recurrent.restarts(P["episode"], P["ended"])
    assert fresh[3, 1] and fresh[2, 2] and not P["first"][3].any() and np.isnan(_np(got["value_new"])[2, 4]) and np.isnan(_np(got["ratio"])[1, 5])
    assert not _np(got["hidden"])[2, 4].any()      # the poisoned cell's h'
    if shuffle is not None:      # the identity over the gathered words gives the same bits: the index is how they are found, nothing else
        plain = env.policy_grad_sequences(_batch(env, P), plants_per_chain=chain, diagnostics=True, **dict(HYPER, clip_vf=clip_vf))
        for k in ("grad", "stats", "more", "logp_new", "value_new", "ratio", "hidden"):
            _same(plain[k], got[k], k)
    env.close()


def test_an_index_outside_the_rollout_poisons_its_plant_and_reads_nothing():
    env, P = _setup(3, 33, 5, 1, 5, (7,), (9, 6))
    batch = _batch(env, P, 5, extra_plants=3)
    index = _np(batch["index"])
    index[[6, 32]] = [-1, 36]      # (the rollout has 36 plants: 0 .. 35)
    batch["index"] = torch.as_tensor(index).to(env.device)
    valid = np.ones(33, dtype=bool)
    valid[[6, 32]] = False
    got, want = _hold(env, P, 32, batch, valid=valid)
    assert want["stats"]["skipped"] == 2 + 2 * T and np.isnan(_np(got["logp_new"])[:, [6, 32]]).all() and not _np(got["hidden"])[:, [6, 32]].any()
    env.close()


def test_no_bit_depends_on_the_launch_geometry():
    env, P = _setup(8, 70, 5, 1, 5, (7,), (9, 6))
    batch = _batch(env, P)
    outs = [env.policy_grad_sequences(batch, plants_per_chain=32, max_blocks=b, diagnostics=True, **HYPER) for b in (1, 0)]
    for k in ("grad", "stats", "more", "ratio", "logp_new", "value_new", "hidden"):
        _same(outs[1][k], outs[0][k], k)
    other = env.policy_grad_sequences(batch, plants_per_chain=64, **HYPER)
    assert not np.array_equal(_np(other["grad"]), _np(outs[0]["grad"]))      # (the chains are the statement's: they do pin the sums)
    env.close()


def test_soft_gates_and_tanh_nets_within_8_times_the_statements_distance_from_float64():
    env, P = _setup(11, 40, 6, 1, 5, (7,), (9, 6), gates="soft", activation="tanh")
    hyper = dict(HYPER, max_grad_norm=0.0)
    got = env.policy_grad_sequences(_batch(env, P), diagnostics=True, **hyper)
    own = statement(P, **hyper)
    g64 = autograd(P, ent_coef=HYPER["ent_coef"])
    mine, yard = distance(_np(got["grad"]), g64), distance(own["grad"], g64)
    print("pooled distance from float64: the device %.3e, the statement %.3e, factor %.2f" % (mine, yard, mine / yard))
    assert mine <= 8 * yard
    env.close()


def test_adam_moves_the_cell_and_the_next_step_runs_it():
    """theta, m and v are ppo.adam's bits fed the device's gradient (std within 1 float ulp: the device's exp), and the next step's hidden
    state is the statement's under the new parameters: the repack ran for the gate layers"""
    env, P = _setup(21, 33, 5, 1, 5, (7,), (9, 6))
    got = env.policy_grad_sequences(_batch(env, P), **HYPER)
    theta0 = P["theta"]
    env.policy_adam(lr=1e-2)
    now = _np(env.policy_theta())
    std_want = np.exp(now[-6:-3].astype(np.float64)).astype(np.float32)
    assert (np.abs(now[-3:] - std_want) <= np.spacing(std_want)).all()
    theta, m, v, step = ppo.adam(theta0, np.zeros_like(theta0), np.zeros_like(theta0), 0, _np(got["grad"]), 3, lr=1e-2, std=now[-3:])
    state = env.policy_optimizer_state()
    _same(now, theta, "theta"); _same(state["m"], m, "m"); _same(state["v"], v, "v")
    n_core = recurrent.core_size(5, 5)
    assert state["step"] == 1 and (now[:n_core] != theta0[:n_core]).mean() > 0.9
    S = env.policy_spec()
    Q = recurrent.Policy(S["cells"], 3, S["actor"], S["critic"], "relu", S["seed"], True, 0, np.float32, core=5, gates="hard", n=env.n)
    Q.load(now)
    before = _np(env.features())
    env.step()
    act, value, _ = Q.step(before)
    _same(env.policy_hidden(), Q.h, "hidden under the new cell"); _same(env.controls_input(), act, "act"); _same(env.policy_outputs()["value"], value, "value")
    stale = recurrent.Policy(S["cells"], 3, S["actor"], S["critic"], "relu", S["seed"], True, 0, np.float32, core=5, gates="hard", n=env.n)
    stale.load(theta0)
    stale.step(before)
    assert not np.array_equal(stale.h, Q.h)
    env.close()


def _collected(n=70, T_=6, H=6, first_plant=0, seed=21):
    """a recurrent policy that collected T_ slots under autoreset (max_episode_steps 3), some plants reset before the rollout began"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv(n, dt=DT, autoreset=True, max_episode_steps=3)
    env.set_features(_columns(5), stack=3, dtype=F32)
    env.set_controls(AXES[:3])
    env.set_rollout(T_, extras=2)
    a, c, log_std = _weights(8, H, 3, (33, 17), (7,))
    env.set_policy(a, c, log_std, activation="relu", seed=seed, extras=("value", "logp"), core=_core(3, 15, H), gates="hard", first_plant=first_plant)
    env.step()
    env.reset(torch.as_tensor(np.arange(n) % 3 == 1))
    env.rollout_begin()
    r = env.collect(T_)
    rh = env.policy_rollout_hidden()
    env.rollout_advantages(0.99, 0.95, values=("extra", 0), last_value=env.policy_values(), final_values=env.policy_values(r["final_obs"], hidden=rh["final"]))
    return env


def test_policy_train_over_sequences_is_the_hand_loop_after_a_real_collect():
    env = _collected()
    S, A = env.policy_spec(), 3
    r = env.rollout()
    episode, ended, first = _np(r["episode"]), _np(r["ended"]), _np(env.policy_rollout_hidden()["first"])
    assert recurrent.restarts(episode, ended)[1:].any() and first.any()
    theta0 = _np(env.policy_theta())
    lr, B, kw = 3e-3, 35, dict(HYPER, clip_vf=0.2)
    theta, stats = theta0, []
    for i, batch in enumerate(env.rollout_minibatches(B, 2, seed=3, unit="plant")):
        got = env.policy_grad_sequences(batch, plants_per_chain=32, diagnostics=True, **kw)
        if i == 0:      # the gathered minibatch against the statement, its words found through the batch's index
            index = _np(batch["index"])
            extra = _np(batch["extra"])
            want = recurrent.gradient(theta, S["cells"], A, S["actor"], S["critic"], "relu", S["core"], "hard", _np(batch["obs"]).reshape(6, B, -1), _np(batch["act"]),
                                      extra[..., 1], _np(batch["adv"]), _np(batch["ret"]), episode[:, index], ended[:, index], first[index],
                                      ratio=_np(got["ratio"]), value_old=extra[..., 0], **kw)
            _same(got["grad"], want["grad"], "grad of a gathered minibatch"); _same(got["hidden"], want["hidden"], "hidden")
            # under the collecting parameters the sequences replay what was recorded: the ratio is 1 where no restart was missed
            _same(got["value_new"], extra[..., 0], "value_new is the recorded value")
        stats.append((_np(got["stats"]), _np(got["more"])))
        env.policy_adam(lr=lr)
        theta = _np(env.policy_theta())
    by_hand, state = theta, env.policy_optimizer_state()
    assert len(stats) == 4 and state["step"] == 4
    # policy_train from the same start, with a gate that never stops: the same four updates
    env.policy_load(theta0)
    env.load_policy_optimizer_state({"m": np.zeros_like(theta0), "v": np.zeros_like(theta0), "step": 0})
    out, more = env.policy_train(B, 2, seed=3, lr=lr, target_kl=1e9, more=True, unit="plant", **kw)
    _same(out, np.stack([s for s, _ in stats]), "stats")
    assert np.array_equal(_np(more)[:, :2].view(np.int64), np.stack([m for _, m in stats])[:, :2].view(np.int64)) and (_np(more)[:, 2] == 1).all()
    after = env.policy_optimizer_state()
    _same(env.policy_theta(), by_hand, "theta"); _same(after["m"], state["m"], "m"); _same(after["v"], state["v"], "v")
    assert after["step"] == 4
    # one shard of one (exchange, shard_cells): shard sums, the combine and the gated Adam step are the same four updates, bit for bit
    env.policy_load(theta0)
    env.load_policy_optimizer_state({"m": np.zeros_like(theta0), "v": np.zeros_like(theta0), "step": 0})
    sharded = env.policy_train(B, 2, seed=3, lr=lr, target_kl=1e9, unit="plant", exchange=lambda vec: vec[None], shard_cells=[env.n], **kw)
    _same(sharded, out, "stats through one shard"); _same(env.policy_theta(), by_hand, "theta through one shard")
    # and a gate that stops at once applies nothing
    env.policy_load(theta0)
    out, more = env.policy_train(B, 1, seed=3, lr=lr, target_kl=1e-12, more=True, unit="plant", **kw)
    assert (_np(more)[1:, 3] == 1).all() and env.policy_optimizer_state()["step"] <= 5
    env.close()


def test_two_handles_train_one_policy_over_sequences():
    """two shards of 33 and 37 plants: each exports its sums over its own sequences, both apply both vectors, and the replicas hold the
    same theta, bit for bit -- the one ppo.combine gives of the two statements' vectors"""
    envs = [_collected(33), _collected(37, first_plant=33)]
    theta0 = _np(envs[0].policy_theta())
    _same(envs[1].policy_theta(), theta0, "the replicas start alike")
    total = 6 * 70
    vecs = []
    for env in envs:
        batch = next(env.rollout_minibatches(env.n, 1, seed=5, unit="plant"))
        vecs.append(env.policy_shard_sums_sequences(batch, total, clip_vf=0.2))
    both = torch.stack(vecs).contiguous()
    for env in envs:
        env.policy_apply_shards(both.to(env.device), total, ent_coef=0.01, lr=1e-2)
    a, b = (_np(env.policy_theta()) for env in envs)
    _same(a, b, "the replicas' theta")
    n_core = recurrent.core_size(15, 6)
    assert (a[:n_core] != theta0[:n_core]).mean() > 0.9      # the cell moved
    grads = [env.policy_combine_shards(both.to(env.device), total, ent_coef=0.01) for env in envs]
    _same(grads[0]["grad"], grads[1]["grad"], "grad"); _same(grads[0]["stats"], grads[1]["stats"], "stats")
    assert _np(grads[0]["stats"])[ppo.STATS.index("count")] == total and _np(grads[0]["grad"])[:n_core].any()
    for env in envs:
        env.close()


def test_refusals_by_name():
    from nuclear_sim_amd._lib import NpbError
    from nuclear_sim_amd.env import BatchedPlantEnv
    env, P = _setup(2, 33, 5, 1, 5, (7,), (9, 6))
    batch = _batch(env, P)
    flat = {k: batch[k].reshape((-1,) + tuple(batch[k].shape[2:])) for k in ("obs", "act", "logp_old", "adv", "ret")}
    with pytest.raises(NpbError, match="training through time is not built"):      # the row-wise calls, with a core: still refused
        env.policy_grad(flat)
    with pytest.raises(NpbError, match="npb_policy_grad_seq"):
        env.policy_shard_sums(flat, 165)
    for kw, words in ((dict(plants_per_chain=48), "multiple of 32"), (dict(clip=1.0), r"\(0, 1\)")):
        with pytest.raises(NpbError, match=words):
            env.policy_grad_sequences(batch, **kw)
    with pytest.raises(ValueError, match="time-major"):
        env.policy_grad_sequences(flat)
    env.close()
    off = BatchedPlantEnv.action_test("oil_top_off", range(4), dt=DT)
    off.set_features(_columns(5), stack=1, dtype=F32)
    off.set_controls(AXES[:3])
    a, c, log_std = _weights(1, 5, 3, (7,), (7,))
    off.set_policy(a, c, log_std, activation="relu", deterministic=True)
    with pytest.raises(NpbError, match="no core"):
        off.policy_grad_sequences(batch)
    with pytest.raises(NpbError, match="no core"):
        off.policy_shard_sums_sequences(batch, 165)
    d, s = off._ppo_desc({k: batch[k] for k in ("obs", "act", "logp_old", "adv", "ret")}, 0.2, 0.5, 0.0, 0.5, 32)[0], _lib.NpbPpoSeq()
    assert off.L.npb_policy_update_seq(off._h, ctypes.byref(d), None, ctypes.byref(s), 1e-3, 0.9, 0.999, 1e-5, None) != 0
    assert b"npb_policy_update_seq: the policy has no core" in off.L.npb_last_error(off._h)
    off.close()


@pytest.mark.parametrize("gates, activation", [("hard", "relu"), ("soft", "tanh")], ids=["hard-relu", "soft-tanh"])
def test_the_three_statements_of_the_cell_agree_device_against_device(gates, activation):
    """The step's launch, the training kernel's forward sweep and the refresh kernel run one cell: after a collect under unchanged parameters
    the hidden states they produce are the same bits, soft gates included (no tolerance: the device against itself).  33 plants (two tiles,
    the second one row wide), 5 feature cells (the k extension to 8), H = 5 (padded to 8), 4 slots, a stored state in front of every slot,
    no autoreset: no restart, so the state in front of slot s + 1 is h' of slot s"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    n, t, H = 33, 4, 5
    env = BatchedPlantEnv(n, dt=DT)
    env.set_features(_columns(5), stack=1, dtype=F32)
    env.set_controls(AXES[:3])
    env.set_rollout(t, extras=2)
    a, c, log_std = _weights(12, H, 3, (7,), (9, 6))
    env.set_policy(a, c, log_std, activation=activation, seed=21, extras=("value", "logp"), core=_core(13, 5, H), gates=gates)
    env.policy_segments(1)
    env.rollout_begin()
    env.collect(t)
    r = env.rollout()
    assert r["t"] == t and np.isfinite(_np(r["obs"])[:t]).all() and not recurrent.restarts(_np(r["episode"])[:t], _np(r["ended"])[:t])[1:].any()
    zeros = torch.zeros((t, n), dtype=torch.float32, device=env.device)
    batch = {"obs": r["obs"][:t], "act": r["act"][:t], "logp_old": r["extra"][:t, :, 1].contiguous(), "adv": zeros, "ret": zeros}
    hidden = _np(env.policy_grad_sequences(batch, diagnostics=True)["hidden"])
    starts = _np(env.policy_rollout_hidden()["starts"])
    assert hidden.shape == (t, n, H) and starts.shape == (t, n, H) and hidden.any(axis=2).all()
    for s in range(t - 1):
        _same(hidden[s], starts[s + 1], "the forward sweep's h' of slot %d against the state the step read in front of slot %d" % (s, s + 1))
    _same(hidden[t - 1], env.policy_hidden(), "the forward sweep's last h' against the live state")
    env.policy_rollout_hidden()["starts"][1:].fill_(7.25)
    env.policy_refresh_segments()
    _same(env.policy_rollout_hidden()["starts"], starts, "the refresh kernel's rows against the recorded ones")
    env.close()


def test_one_table_over_the_update_and_shard_entry_points():
    """Refusals only, no kernel runs: the gate rule of the five update calls, the three shard-sum calls' own refusals, and rows against
    sequences on a handle with a core and on one without.  Every row names its entry point"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    env, P = _setup(2, 33, 5, 1, 5, (7,), (9, 6))
    batch = _batch(env, P)
    off = BatchedPlantEnv.action_test("oil_top_off", range(4), dt=DT)
    off.set_features(_columns(5), stack=1, dtype=F32)
    off.set_controls(AXES[:3])
    a, c, log_std = _weights(1, 5, 3, (7,), (7,))
    off.set_policy(a, c, log_std, activation="relu", deterministic=True)
    flat = {k: batch[k].reshape((-1,) + tuple(batch[k].shape[2:])) for k in ("obs", "act", "logp_old", "adv", "ret")}
    ref, adam = ctypes.byref, (1e-3, 0.9, 0.999, 1e-5)
    rows_d, held_rows = off._ppo_desc(flat, 0.2, 0.5, 0.0, 0.5, 32)
    seq_d, held_d = env._ppo_desc(batch, 0.2, 0.5, 0.0, 0.5, 32)
    s, none, held_s = env._ppo_seq(batch, seq_d)
    g = _lib.NpbPpoSegments()
    g.every, g.chunks = s.t, 1
    assert none is None and rows_d.count == seq_d.count == T * 33
    gated, plain, shards = _lib.NpbPpoMore(), _lib.NpbPpoMore(), {k: _lib.NpbPpoShards() for k in (0.0, 0.03)}
    gated.kl_limit = 0.03
    for k, v in shards.items():
        v.kl_limit = k
    outs = {h: torch.zeros(h.policy_shard_size(), dtype=torch.float64, device=h.device) for h in (env, off)}

    def refused(h, name, words, *args, by=None):
        """the call is refused in these words, under its own name (by: the exported check's name, where a shared check speaks)"""
        assert getattr(h.L, name)(h._h, *args, None) != 0, name
        why = h.L.npb_last_error(h._h)
        assert why.startswith((by or name).encode() + b": ") and words in why, (name, words, why)

    def update(name, m, seq=ref(s)):
        """the arguments of an update call that takes options m; seq: the sequence calls' descriptor (None: a NULL one)"""
        return {"npb_policy_update_more": (ref(rows_d), m), "npb_policy_update_seq": (ref(seq_d), m, seq),
                "npb_policy_update_segments": (ref(seq_d), m, seq, ref(g))}[name] + adam

    def shard(name, m, total, out, seq=ref(s)):
        d = rows_d if name == "npb_policy_shard_sums" else seq_d
        tail = (total, None if out is None else ctypes.c_void_p(out.data_ptr()))
        return {"npb_policy_shard_sums": (ref(d), m), "npb_policy_shard_sums_seq": (ref(d), m, seq), "npb_policy_shard_sums_segments": (ref(d), m, seq, ref(g))}[name] + tail
    total = T * 33
    # ---- rows against sequences: the row-wise calls on the handle with a core, the sequence calls on the one without
    order, no_core = b"rows carry no order", b"the policy has no core"
    refused(env, "npb_policy_grad", order, ref(seq_d))
    refused(env, "npb_policy_grad_more", order, ref(seq_d), ref(plain))
    refused(env, "npb_policy_update", order, ref(seq_d), *adam)
    refused(env, "npb_policy_update_more", order, ref(seq_d), ref(plain), *adam)
    refused(env, "npb_policy_shard_sums", order, ref(seq_d), None, total, ctypes.c_void_p(outs[env].data_ptr()))
    refused(off, "npb_policy_grad_seq", no_core, ref(seq_d), None, ref(s))
    refused(off, "npb_policy_grad_segments", no_core, ref(seq_d), None, ref(s), ref(g))
    for name in ("npb_policy_update_seq", "npb_policy_update_segments"):
        refused(off, name, no_core, *update(name, None))
    for name in ("npb_policy_shard_sums_seq", "npb_policy_shard_sums_segments"):
        refused(off, name, no_core, *shard(name, None, total, outs[off]))
    # ---- a NULL sequence descriptor is never read as rows: without a core "no core" under the call's own name, with one the check's words
    null_seq = b"a NULL sequence descriptor"
    for h, words, by in ((off, no_core, None), (env, null_seq, "npb_policy_grad_seq")):
        refused(h, "npb_policy_grad_seq", words, ref(seq_d), None, None, by=by)
        refused(h, "npb_policy_grad_segments", words, ref(seq_d), None, None, ref(g), by=by)
        for name in ("npb_policy_update_seq", "npb_policy_update_segments"):
            refused(h, name, words, *update(name, None, seq=None), by=by)
        for name in ("npb_policy_shard_sums_seq", "npb_policy_shard_sums_segments"):
            refused(h, name, words, *shard(name, None, total, outs[h], seq=None), by=by)
    # ---- the shard-sum calls' own refusals, each on the handle of its kind
    for h, name in ((off, "npb_policy_shard_sums"), (env, "npb_policy_shard_sums_seq"), (env, "npb_policy_shard_sums_segments")):
        refused(h, name, b"the gate belongs to the combine", *shard(name, ref(gated), total, outs[h]))
        refused(h, name, b"count_total < desc->count", *shard(name, None, total - 1, outs[h]))
        refused(h, name, b"a NULL or misaligned out", *shard(name, None, total, None))
    # ---- the gate rule: kl_limit > 0 outside the pair, kl_limit == 0 inside it
    outside, inside = b"kl_limit > 0 outside npb_policy_train_begin", b"kl_limit == 0 between"
    refused(off, "npb_policy_update_more", outside, *update("npb_policy_update_more", ref(gated)))
    for name in ("npb_policy_update_seq", "npb_policy_update_segments"):
        refused(env, name, outside, *update(name, ref(gated)))
    for h in (env, off):
        refused(h, "npb_policy_apply_shards", outside, ref(shards[0.03]), *adam)
        assert h.L.npb_policy_train_begin(h._h, None) == 0
    refused(off, "npb_policy_update", inside, ref(rows_d), *adam)
    refused(off, "npb_policy_update_more", inside, *update("npb_policy_update_more", ref(plain)))
    for name in ("npb_policy_update_seq", "npb_policy_update_segments"):
        refused(env, name, inside, *update(name, None))
    for h in (env, off):
        refused(h, "npb_policy_apply_shards", inside, ref(shards[0.0]), *adam)
        applied = ctypes.c_uint32(7)
        assert h.L.npb_policy_train_end(h._h, ref(applied), None) == 0 and applied.value == 0
        refused(h, "npb_policy_train_end", b"no npb_policy_train_begin before it", None)      # nothing stays armed
        refused(h, "npb_policy_apply_shards", outside, ref(shards[0.03]), *adam)
        h.close()
