"""GPU: truncated segments on the device -- the stored start states recorded while collecting (npb_policy_core_segments), segment minibatches
(npb_rollout_minibatch_segments), their gradient, update and shard sums (npb_policy_grad_segments and companions) and the refresh of the
stored states (npb_policy_segment_starts) -- through BatchedPlantEnv.policy_segments, rollout_minibatches(unit="segment"),
policy_grad_sequences, policy_shard_sums_sequences, policy_train(unit="segment") and policy_refresh_segments, against
nuclear_sim_amd.recurrent's and rollout's numpy statements and against the whole-sequence entry points.

Hard gates with relu nets are compared by bits, the ratio within the 4 ulp the whole-sequence suite allows, and gradient, stats and more by
bits once the statement is fed the device's ratio.  Device against device (a segment batch against the equivalent whole-sequence call) is by
bits for soft gates and tanh nets too.  Soft gates with tanh nets may stand 8 times as far from float64 autograd as the statement does.

The hand-made rollouts (segments_support.rollout_problem) have T = 6 slots and n = 33 or 35 plants, so that g / n is never a shift; every in
{1, 2, 3, 6}; 33 and 70 segments a minibatch (a ragged second tile; two chains of 64, the last tile 6 wide); K * C = 5, or 65 with H = 65 for
the large LDS build; H in {5, 33, 65}.  One restart lies on a segment boundary, one inside a segment, one poisoned cell is the last slot of a
segment, one cell is skipped."""
import numpy as np
import pytest
import torch

from nuclear_sim_amd import ppo, recurrent, rollout
from recurrent_train_support import distance
from segments_support import autograd_truncated, rollout_problem, segment_batch, statement_segments
from test_policy_gpu import AXES, DT, F32, F64, _columns, _np, _same
from test_recurrent_gpu import _cell_bound, _env

pytestmark = pytest.mark.gpu

HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5)
T = 6
KEYS = ("grad", "stats", "more", "logp_new", "value_new", "ratio", "hidden")


def _setup(seed, n, every, C, K, H, actor, critic, gates="hard", activation="relu", A=3, cdtype=F32, R=None):
    """an env whose policy has the rollout problem's shapes and parameters, and the problem with the device's own theta.  ``A`` axes,
    controls of ``cdtype`` (the type ``act`` must have); ``R``: a rollout problem made elsewhere, in place of the seed's"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    if R is None:
        R = rollout_problem(seed, T, n, C * K, H, A, actor, critic, gates, activation, every)
    A = R["n_axes"]
    core, a, c, log_std, _ = recurrent.unpack(R["theta"], C * K, A, actor, critic, H)
    env = BatchedPlantEnv.action_test("oil_top_off", range(4), dt=DT)
    env.set_features(_columns(C), stack=K, dtype=F32)
    env.set_controls(AXES[:A], dtype=cdtype)
    env.set_policy(a, c, log_std, activation=activation, deterministic=True, core=core, gates=gates)
    R["theta"] = _np(env.policy_theta())
    return env, R


def _ids(R, count, seed):
    """``count`` shuffled segment ids that hold every special cell's segment: the boundary restart's two sides (plant 1), the inner restart
    (plant 2), the poisoned cell and the segment behind it (plant 4), the skipped cell (plant 5)"""
    n, L, chunks = R["n"], R["every"], R["chunks"]
    must = {1, 2, 4, 5 + ((T - 2) // L) * n} | ({n + 1, n + 4} if chunks > 1 else set())
    rng = np.random.default_rng(seed)
    rest = [g for g in rng.permutation(chunks * n) if g not in must][:count - len(must)]
    return rng.permutation(np.array(sorted(must) + rest, dtype=np.int32))


def _batch(env, R, Q):
    """the segment minibatch Q as the device takes it, beside the rollout's own words and stored states"""
    batch = {k: Q[k] for k in ("obs", "act", "logp_old", "adv", "ret", "value_old", "index")}
    batch.update(episode=R["episode"], ended=R["ended"], first=R["starts"])
    batch = {k: torch.as_tensor(v).to(env.device) for k, v in batch.items()}
    batch["every"] = R["every"]
    return batch


def _array(d, names):
    return np.array([d[k] for k in names])


def _hold(env, R, Q, chain, **hyper):
    """the bit contract on one segment minibatch; returns the device's outputs and the statement's"""
    kw = dict(HYPER, **hyper)
    got = env.policy_grad_sequences(_batch(env, R, Q), plants_per_chain=chain, diagnostics=True, **kw)
    extra = dict(value_old=Q["value_old"]) if kw.get("clip_vf") else {}
    own = statement_segments(R, Q, plants_per_chain=chain, **kw, **extra)
    _same(got["logp_new"], own["logp_new"], "logp_new"); _same(got["value_new"], own["value_new"], "value_new"); _same(got["hidden"], own["hidden"], "hidden")
    ratio = _np(got["ratio"])
    live = np.isfinite(own["ratio"])
    assert np.array_equal(np.isfinite(ratio), live)
    ulps = np.abs(ratio[live] - own["ratio"][live]) / np.spacing(own["ratio"][live])
    print("the ratio: at most %.1f ulp from numpy's" % ulps.max())
    assert ulps.max() <= 4
    want = statement_segments(R, Q, plants_per_chain=chain, ratio=ratio, **kw, **extra)
    _same(got["grad"], want["grad"], "grad"); _same(got["stats"], _array(want["stats"], ppo.STATS), "stats"); _same(got["more"], _array(want["more"], ppo.STATS_MORE), "more")
    n_core = recurrent.core_size(R["cells"], R["core"])
    assert np.isfinite(want["grad"]).all() and want["grad"][:n_core].any() and want["grad"][n_core:-R["n_axes"]].any()
    return got, want


# ---------------------------------------------------------------------------------------------------------------- 1
# n, every, segments of the minibatch, chain, C, K, H, actor, critic, clip_vf
CASES = [(33, 6, 33, 32, 5, 1, 5, (7,), (9, 6), 0.0), (35, 3, 70, 64, 5, 1, 33, (33, 17), (7,), 0.0), (33, 2, 70, 64, 13, 5, 65, (7,), (33, 17), 0.2),
         (35, 1, 33, 32, 5, 1, 5, (64, 64), (7,), 0.2)]


@pytest.mark.parametrize("n, every, count, chain, C, K, H, actor, critic, clip_vf", CASES, ids=["33x6-33", "35x3-70-33", "33x2-70-65-65-large-clipvf", "35x1-33-clipvf"])
def test_hard_gates_and_relu_nets_bit_for_bit(n, every, count, chain, C, K, H, actor, critic, clip_vf):
    """Fails without the feature: a batch's "every" selects entry points that do not exist"""
    env, R = _setup(n + H + every, n, every, C, K, H, actor, critic)
    Q = segment_batch(R, _ids(R, count, seed=every))
    assert Q["count"] == count and len(set(Q["index"].tolist())) == count
    got, want = _hold(env, R, Q, chain, clip_vf=clip_vf)
    assert want["stats"]["skipped"] == 2 and want["stats"]["count"] == every * count
    S = R["starts"]
    if every < T:      # the boundary restart and the poisoned last slot: +0.0 rows of the stored states, which the segments behind them read
        assert not S[1, 1].any() and not S[1, 4].any() and S[1, 0].any()
    j = {int(g): k for k, g in enumerate(Q["index"])}
    assert np.isnan(_np(got["value_new"])[every - 1, j[4]]) and not _np(got["hidden"])[every - 1, j[4]].any()      # the poisoned cell and its h'
    s5, g5 = (T - 2) % every, 5 + ((T - 2) // every) * n
    assert np.isnan(_np(got["ratio"])[s5, j[g5]]) and _np(got["hidden"])[s5, j[g5]].any()      # the skipped one still ran
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("gates, activation", [("hard", "relu"), ("soft", "tanh")])
def test_a_segment_batch_is_the_equivalent_whole_sequence_call_by_bits(gates, activation):
    """device against device, so soft gates and tanh nets too.  (a) every == t: the bits of the whole-sequence call on the same rollout.
    (b) every = 3: the bits of the whole-sequence call on the hand-made problem whose 'rollout' is [L][chunks * n] and whose first is the
    stored states flattened -- section 5's equivalence, on the device"""
    kw = dict(HYPER, clip_vf=0.2)
    env, R = _setup(17, 33, T, 5, 1, 5, (7,), (9, 6), gates, activation)
    Q = segment_batch(R)
    seg = env.policy_grad_sequences(_batch(env, R, Q), plants_per_chain=32, diagnostics=True, **kw)
    whole = {k: torch.as_tensor(R[k]).to(env.device) for k in ("obs", "act", "logp_old", "adv", "ret", "value_old", "episode", "ended", "first")}
    plant = env.policy_grad_sequences(whole, plants_per_chain=32, diagnostics=True, **kw)
    for k in KEYS:
        _same(seg[k], plant[k], ("every == t", k))
    env.close()
    env, R = _setup(18, 35, 3, 5, 1, 33, (33, 17), (7,), gates, activation)
    Q = segment_batch(R, _ids(R, 70, seed=2))
    seg = env.policy_grad_sequences(_batch(env, R, Q), plants_per_chain=64, diagnostics=True, **kw)
    made = {k: torch.as_tensor(Q[k]).to(env.device) for k in ("obs", "act", "logp_old", "adv", "ret", "value_old", "episode", "ended", "first")}
    plant = env.policy_grad_sequences(made, plants_per_chain=64, diagnostics=True, **kw)
    for k in KEYS:
        _same(seg[k], plant[k], ("every = 3", k))
    n_core = recurrent.core_size(5, 33)
    assert _np(seg["grad"])[:n_core].any() and _np(seg["grad"])[n_core:-3].any() and _np(seg["stats"])[ppo.STATS.index("skipped")] == 2
    # and the shard sums, the same way
    a = env.policy_shard_sums_sequences(_batch(env, R, Q), 1000, plants_per_chain=64, clip_vf=0.2)
    b = env.policy_shard_sums_sequences(made, 1000, plants_per_chain=64, clip_vf=0.2)
    _same(a, b, "shard sums")
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_a_segment_id_outside_the_rollout_poisons_its_sequence_and_reads_nothing():
    env, R = _setup(3, 33, 2, 5, 1, 5, (7,), (9, 6))
    index = _ids(R, 33, seed=5)
    free = [k for k, g in enumerate(index) if int(g) % 33 not in (1, 2, 4, 5)][:2]
    index[free] = [-1, R["chunks"] * 33]      # (the rollout has 3 x 33 segments: 0 .. 98)
    Q = segment_batch(R, index)
    assert list(np.flatnonzero(~Q["valid"])) == sorted(free)
    got, want = _hold(env, R, Q, 32)
    assert want["stats"]["skipped"] == 2 + 2 * 2 and np.isnan(_np(got["logp_new"])[:, free]).all() and not _np(got["hidden"])[:, free].any()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_no_bit_depends_on_the_launch_geometry():
    env, R = _setup(8, 35, 3, 5, 1, 5, (7,), (9, 6))
    batch = _batch(env, R, segment_batch(R, _ids(R, 70, seed=1)))
    outs = [env.policy_grad_sequences(batch, plants_per_chain=32, max_blocks=b, diagnostics=True, **HYPER) for b in (1, 0)]
    for k in KEYS:
        _same(outs[1][k], outs[0][k], k)
    other = env.policy_grad_sequences(batch, plants_per_chain=64, **HYPER)
    assert not np.array_equal(_np(other["grad"]), _np(outs[0]["grad"]))      # (the chains are the statement's: they do pin the sums)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("every", [2, 3])
def test_soft_gates_and_tanh_nets_within_8_times_the_statements_distance_from_float64(every):
    env, R = _setup(11, 35, every, 6, 1, 5, (7,), (9, 6), gates="soft", activation="tanh")
    Q = segment_batch(R)      # every segment: the loss of the truncated autograd, which walks the whole rollout
    hyper = dict(HYPER, max_grad_norm=0.0)
    got = env.policy_grad_sequences(_batch(env, R, Q), **hyper)
    own = statement_segments(R, Q, **hyper)
    g64 = autograd_truncated(R, ent_coef=HYPER["ent_coef"])
    mine, yard = distance(_np(got["grad"]), g64), distance(own["grad"], g64)
    print("pooled distance from float64: the device %.3e, the statement %.3e, factor %.2f" % (mine, yard, mine / yard))
    assert mine <= 8 * yard
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 6
SENTINEL = 7.25


def _collecting(n, steps, gates="hard", activation="relu", every=3, H=6, first=0, fdtype=F32, C=5, K=3, **nets):
    """a recurrent policy with stored segment states, some plants reset just before the rollout begins, so that the step limit restarts
    some in front of a boundary slot and others inside a segment; the stored states filled with a sentinel.  ``nets``: actor=, critic="""
    env = _env(n, C, K, fdtype, H, gates=gates, activation=activation, steps=steps, rollout=T, first=first, **nets)
    env.policy_segments(every)
    env.step()
    env.reset(torch.as_tensor(np.arange(first, first + n) % 3 == 1))
    env.rollout_begin()
    env.policy_rollout_hidden()["starts"].fill_(SENTINEL)
    return env


def _steps(env, k):
    """k recorded steps (the run's heat-source noise comes from the host every step: collect() is not for it)"""
    for _ in range(k):
        env.step()


def _advantages(env):
    r, rh = env.rollout(), env.policy_rollout_hidden()
    env.rollout_advantages(0.99, 0.95, values=("extra", 0), last_value=env.policy_values(), final_values=env.policy_values(r["final_obs"], hidden=rh["final"]))


def _core_of(env):
    S = env.policy_spec()
    return recurrent.unpack(_np(env.policy_theta()), S["cells"], 3, S["actor"], S["critic"], S["core"])[0]


@pytest.mark.parametrize("steps, gates, activation", [(3, "hard", "relu"), (4, "hard", "relu"), (3, "soft", "tanh")], ids=["limit3-hard", "limit4-hard", "limit3-soft"])
def test_the_stored_states_after_a_real_collect(steps, gates, activation):
    """every = 3 under autoreset from a start bank.  With a step limit of 3 the plants reset before the rollout restart in front of slot 3,
    a boundary, and the others in front of slots 2 and 5, inside segments; with 4 it is the other way round.  starts[0] is first by bits;
    starts[1] is recurrent.replay's state in front of slot 3 -- hard gates by bits; soft gates by test_recurrent_gpu.py's contract: the
    device's own h fed back, so the row is the restart rule over the live hidden state BY BITS, and that state is one cell from the state
    before it within the bound of the cell's own weights"""
    n, L = 70, 3
    env = _collecting(n, steps, gates, activation)
    live = []
    for s in range(T):
        live.append(_np(env.policy_hidden()))
        env.step()
        if s == 2:      # three slots recorded: row 1 is not reached yet and keeps the sentinel
            rh = env.policy_rollout_hidden()
            assert rh["every"] == L and rh["starts"].shape == (2, n, 6)
            assert (_np(rh["starts"])[1] == SENTINEL).all() and not (_np(rh["starts"])[0] == SENTINEL).any()
    r, rh = env.rollout(), env.policy_rollout_hidden()
    assert r["t"] == T
    obs, episode, ended, first, starts = _np(r["obs"]), _np(r["episode"]), _np(r["ended"]), _np(rh["first"]), _np(rh["starts"])
    _same(starts[0], first, "starts[0] is first")
    fresh = recurrent.restarts(episode, ended)
    assert fresh[3].any() and not fresh[3].all() and (fresh[2] | fresh[4] | fresh[5]).any()      # restarts on the boundary, and inside segments
    assert not starts[1][fresh[3]].any() and starts[1][~fresh[3]].any(axis=1).all()
    want = np.where(fresh[3][:, None], np.float32(0.0), live[3])
    _same(starts[1], want, "starts[1] is the restart rule over the live state the step read")
    core = _core_of(env)
    if gates == "hard":
        _same(starts, recurrent.starts(first, obs, episode, ended, core, "hard", L), "starts against replay")
    else:
        before = np.where(fresh[2][:, None], np.float32(0.0), live[2])
        h2, _ = recurrent.advance(core, obs[2], before, "soft")
        bound = _cell_bound(core, float(np.abs(obs[2].astype(np.float32)).max()))
        err = np.abs(live[3].astype(np.float64) - h2).max()
        print("soft: the live state in front of slot 3 errs by %.3e (bound %.3e)" % (err, bound))
        assert err <= bound < 3e-5
    # the refresh under the collecting parameters reproduces the recorded rows, by bits, soft gates included; row 0 is not touched
    rh["starts"][0].fill_(SENTINEL)
    env.policy_refresh_segments()
    now = _np(env.policy_rollout_hidden()["starts"])
    assert (now[0] == SENTINEL).all()
    _same(now[1], starts[1], "the refresh before any update")
    env.close()


def test_policy_train_over_segments_is_the_hand_loop():
    """policy_train(unit="segment") is rollout_minibatches(unit="segment"), policy_grad_sequences and policy_adam, by bits -- and with
    refresh="epoch" the same loop with policy_refresh_segments() between the epochs, which after an update moves the stored states to
    recurrent.starts under the new theta, by bits with hard gates"""
    env = _collecting(70, 3)
    _steps(env, T)
    _advantages(env)
    S, A, L = env.policy_spec(), 3, 3
    r, rh = env.rollout(), env.policy_rollout_hidden()
    obs, episode, ended, first = _np(r["obs"]), _np(r["episode"]), _np(r["ended"]), _np(rh["first"])
    recorded = _np(rh["starts"])
    theta0 = _np(env.policy_theta())
    lr, B, kw = 3e-3, 50, dict(HYPER, clip_vf=0.2)
    zero = {"m": np.zeros_like(theta0), "v": np.zeros_like(theta0), "step": 0}

    def by_hand(refresh):
        env.policy_load(theta0)
        env.load_policy_optimizer_state(zero)
        rh["starts"].copy_(torch.as_tensor(recorded))
        stats, epoch = [], 0
        for i, batch in enumerate(env.rollout_minibatches(B, 2, seed=3, unit="segment")):
            if refresh and batch["epoch"] != epoch:
                epoch = batch["epoch"]
                env.policy_refresh_segments()
                core = recurrent.unpack(_np(env.policy_theta()), S["cells"], A, S["actor"], S["critic"], S["core"])[0]
                now = _np(rh["starts"])
                _same(now, recurrent.starts(first, obs, episode, ended, core, "hard", L), "the refreshed states under the new theta")
                assert not np.array_equal(now[1], recorded[1])
                _same(now[0], recorded[0], "row 0")
            assert batch["every"] == L and batch["obs"].shape[:2] == (L, batch["index"].numel())
            got = env.policy_grad_sequences(batch, plants_per_chain=32, diagnostics=True, **kw)
            if i == 0:      # the gathered minibatch against the statement, its words found through the batch's segment ids
                extra = _np(batch["extra"])
                want = recurrent.gradient_segments(theta0, S["cells"], A, S["actor"], S["critic"], "relu", S["core"], "hard", _np(batch["obs"]).reshape(L, B, -1),
                                                   _np(batch["act"]), extra[..., 1], _np(batch["adv"]), _np(batch["ret"]), episode, ended, recorded,
                                                   _np(batch["index"]), env.n, L, ratio=_np(got["ratio"]), value_old=extra[..., 0], **kw)
                _same(got["grad"], want["grad"], "grad of a gathered segment minibatch"); _same(got["hidden"], want["hidden"], "hidden")
                # under the collecting parameters every segment replays what was recorded, from its stored state
                _same(got["value_new"], extra[..., 0], "value_new is the recorded value")
            stats.append(_np(got["stats"]))
            env.policy_adam(lr=lr)
        return np.stack(stats), _np(env.policy_theta()), env.policy_optimizer_state()

    for refresh in (None, "epoch"):
        stats, theta, state = by_hand(refresh)
        assert len(stats) == 6 and state["step"] == 6      # 2 x 70 segments in batches of 50: 50, 50, 40, twice
        env.policy_load(theta0)
        env.load_policy_optimizer_state(zero)
        rh["starts"].copy_(torch.as_tensor(recorded))
        out = env.policy_train(B, 2, seed=3, lr=lr, unit="segment", refresh=refresh, **kw)
        _same(out, stats, ("stats", refresh)); _same(env.policy_theta(), theta, ("theta", refresh))
        after = env.policy_optimizer_state()
        _same(after["m"], state["m"], "m"); _same(after["v"], state["v"], "v")
        if refresh is None:
            plain = theta
    assert not np.array_equal(plain, theta)      # (the refreshed states do move the second epoch)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("fdtype, adv_dtype", [(F32, torch.float32), (F64, torch.float64)], ids=["f32", "f64"])
def test_segment_minibatches_bit_for_bit_with_the_numpy_statement(fdtype, adv_dtype):
    """n = 33, every in {1, 2, 3, 6}, with and without the moments, batches of 40: a short last batch wherever 40 does not divide"""
    n = 33
    env = _env(n, 5, 1, fdtype, 6, rollout=T)
    _steps(env, T)
    g = torch.Generator().manual_seed(7)
    R_ = env.rollout_spec()["final_rows"]
    adv, ret = env.rollout_advantages(0.99, 0.95, values=(torch.rand((T, n), generator=g) - 0.5).to(torch.float32),
                                      last_value=(torch.rand(n, generator=g) - 0.5).to(torch.float32),
                                      final_values=(torch.rand(n * R_, generator=g) - 0.5).to(torch.float32), dtype=adv_dtype)
    r = env.rollout()
    arrays = {k: (None if r[k] is None else _np(r[k])) for k in ("obs", "act", "extra")}
    a, b = _np(adv), _np(ret)
    for every in (1, 2, 3, 6):
        env.policy_segments(every)
        N = (T // every) * n
        for normalise in (True, False):
            m = rollout.moments(a[:T]) if normalise else None
            keys = rollout.permutation_keys(3, every)
            first, seen = 0, []
            for mb in env.rollout_minibatches(40, seed=3, first_epoch=every, normalize=normalise, unit="segment"):
                count = min(40, N - first)
                assert mb["every"] == every and mb["index"].shape == (count,) and mb["index"].dtype == torch.int32
                want = rollout.minibatch(arrays, T, a, b, keys, first, count, "segment", moments=m, eps=1e-8, every=every)
                for name in ("index", "obs", "act", "extra", "adv", "ret"):
                    _same(mb[name], want[name], (name, every, first, normalise))
                assert mb["obs"].shape[:2] == (every, count)
                seen.append(want["index"])
                first += count
            assert first == N and np.array_equal(np.sort(np.concatenate(seen)), np.arange(N, dtype=np.int32))
            assert len(seen) == -(-N // 40) and (N % 40 == 0 or len(seen[-1]) == N % 40)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 9
def test_two_handles_train_one_policy_over_segments():
    """two shards of 33 and 37 plants train one policy through exchange / shard_cells, each over its own segments; both end with the
    parameter bits of ONE handle that accumulates both shards' vectors itself"""
    L = 3
    envs = [_collecting(33, 3), _collecting(37, 3, first=33)]
    for env in envs:
        _steps(env, T)
        _advantages(env)
    theta0 = _np(envs[0].policy_theta())
    _same(envs[1].policy_theta(), theta0, "the replicas start alike")
    cells = [2 * 33, 2 * 37]
    lr, kw = 1e-2, dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5, clip_vf=0.2)
    # the hand loop of one accumulating handle: both shards' vectors of every update, applied by shard 0's handle
    total = L * sum(cells)
    vecs = [env.policy_shard_sums_sequences(next(env.rollout_minibatches(c, 1, seed=5, unit="segment")), total, clip_vf=0.2) for env, c in zip(envs, cells)]
    both = torch.stack([v.to(envs[0].device) for v in vecs]).contiguous()
    envs[0].policy_apply_shards(both, total, ent_coef=0.01, lr=lr)
    one = _np(envs[0].policy_theta())
    n_core = recurrent.core_size(15, 6)
    assert (one[:n_core] != theta0[:n_core]).mean() > 0.9      # the cell moved
    stats = _np(envs[0].policy_combine_shards(both, total, ent_coef=0.01)["stats"])
    assert stats[ppo.STATS.index("count")] == total
    # policy_train on both shards from the same start
    zero = {"m": np.zeros_like(theta0), "v": np.zeros_like(theta0), "step": 0}
    envs[0].policy_load(theta0)
    envs[0].load_policy_optimizer_state(zero)
    def exchange(i):      # (this shard's vector is the hand loop's, by bits: the all-gather of the two is then `both`)
        def gather(vec):
            _same(vec, vecs[i], ("the vector of shard", i))
            return both.to(vec.device)
        return gather
    for i, env in enumerate(envs):      # (a batch of the larger shard's size: one update on each)
        out = env.policy_train(max(cells), 1, seed=5, lr=lr, unit="segment", exchange=exchange(i), shard_cells=cells, **kw)
        assert out.shape == (1, 8) and _np(out)[0, ppo.STATS.index("count")] == total
    a, b = (_np(env.policy_theta()) for env in envs)
    _same(a, b, "the replicas' theta"); _same(a, one, "and the accumulating handle's")
    for env in envs:
        env.close()


# ---------------------------------------------------------------------------------------------------------------- 10
def test_lifecycle_and_refusals_by_name():
    from nuclear_sim_amd._lib import NpbError
    from nuclear_sim_amd.env import BatchedPlantEnv
    n = 33
    env = _env(n, 5, 1, F32, 6, rollout=T)
    with pytest.raises(NpbError, match="policy_segments"):      # unit="segment" without the stored states
        env.rollout_minibatches(8, unit="segment")
    with pytest.raises(NpbError, match="policy_segments"):
        env.policy_refresh_segments()
    for every in (0, 7):
        with pytest.raises(ValueError, match="every must be"):
            env.policy_segments(every)
    assert "starts" not in env.policy_rollout_hidden()
    env.policy_segments(2)
    rh = env.policy_rollout_hidden()
    assert rh["every"] == 2 and rh["starts"].shape == (3, n, 6)
    # t = 4 recorded of T = 6 trains on two chunks; t = 5 is refused
    _steps(env, 4)
    g = torch.Generator().manual_seed(7)
    R_ = env.rollout_spec()["final_rows"]

    def advantages():
        return env.rollout_advantages(0.99, 0.95, values=(torch.rand((T, n), generator=g) - 0.5).to(torch.float32),
                                      last_value=(torch.rand(n, generator=g) - 0.5).to(torch.float32),
                                      final_values=(torch.rand(n * R_, generator=g) - 0.5).to(torch.float32))
    advantages()
    batches = list(env.rollout_minibatches(2 * n, unit="segment"))
    assert len(batches) == 1 and sorted(_np(batches[0]["index"]).tolist()) == list(range(2 * n)) and batches[0]["obs"].shape[:2] == (2, 2 * n)
    out = env.policy_train(2 * n, 1, lr=1e-3, unit="segment")
    assert out.shape == (1, 8) and _np(out)[0, ppo.STATS.index("count")] == 4 * n and env.policy_optimizer_state()["step"] == 1
    env.policy_refresh_segments()
    env.step()
    advantages()
    for call in (lambda: env.rollout_minibatches(8, unit="segment"), lambda: env.policy_train(8, 1, unit="segment"), env.policy_refresh_segments):
        with pytest.raises((NpbError, ValueError), match="ragged last segments|not a multiple of every"):
            call()
    with pytest.raises(ValueError, match="refresh"):
        env.policy_train(8, 1, unit="plant", refresh="epoch")
    # rollout_begin re-records from row 0
    env.policy_rollout_hidden()["starts"].fill_(SENTINEL)
    env.rollout_begin()
    env.step()
    rh = env.policy_rollout_hidden()
    _same(rh["starts"][0], rh["first"], "row 0 after rollout_begin")
    assert (_np(rh["starts"])[1:] == SENTINEL).all()
    # clearing it restores the behaviour without it: nothing is written any more, and the unit is refused again
    env.policy_segments(None)
    kept = rh["starts"]
    kept.fill_(SENTINEL)
    env.rollout_begin()
    _steps(env, 3)
    assert (_np(kept) == SENTINEL).all() and "starts" not in env.policy_rollout_hidden()
    with pytest.raises(NpbError, match="policy_segments"):
        env.rollout_minibatches(8, unit="segment")
    whole = list(env.rollout_minibatches(n, unit="plant", advantages=(torch.zeros((T, n), device=env.device), torch.zeros((T, n), device=env.device))))
    assert len(whole) == 1 and "every" not in whole[0] and whole[0]["obs"].shape[:2] == (3, n)
    # the library's own words, through the handle
    L_ = env.L
    assert L_.npb_policy_segment_starts(env._h, 2, None) != 0 and b"npb_policy_segment_starts: no stored states set" in L_.npb_last_error(env._h)
    env.policy_segments(2)
    assert L_.npb_policy_segment_starts(env._h, 3, None) != 0 and b"every is not the one" in L_.npb_last_error(env._h)
    env.set_policy(None)      # the policy takes the stored states with it
    assert L_.npb_policy_core_segments(env._h, 2, kept.data_ptr(), 3) != 0 and b"npb_policy_core_segments: the policy has no core" in L_.npb_last_error(env._h)
    env.close()
    # without a core, and without a rollout
    off = BatchedPlantEnv.action_test("oil_top_off", range(4), dt=DT)
    off.set_features(_columns(5), stack=1, dtype=F32)
    off.set_controls(AXES[:3])
    from test_policy_gpu import _weights
    a, c, log_std = _weights(1, 5, 3, (7,), (7,))
    off.set_policy(a, c, log_std, activation="relu", deterministic=True)
    with pytest.raises(NpbError, match="no core"):
        off.policy_segments(2)
    from test_recurrent_gpu import _core
    a, c, log_std = _weights(1, 6, 3, (7,), (7,))
    off.set_policy(a, c, log_std, activation="relu", deterministic=True, core=_core(1, 5, 6), gates="hard")
    with pytest.raises(NpbError, match="rollout"):
        off.policy_segments(2)
    dummy = torch.zeros((3, 4, 6), dtype=torch.float32, device=off.device)
    assert off.L.npb_policy_core_segments(off._h, 2, dummy.data_ptr(), 3) != 0 and b"npb_policy_core_segments: no rollout set" in off.L.npb_last_error(off._h)
    off.close()
