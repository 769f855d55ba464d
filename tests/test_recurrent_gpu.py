"""GPU: the recurrent policy on the device (npb_set_policy_core, BatchedPlantEnv.set_policy(core=...)) -- a GRU cell in front of actor and
critic, its hidden state carried per plant with the episode's lifecycle -- against nuclear_sim_amd.recurrent, the numpy statement, fed the
device's own features.  Hard gates with relu nets are compared by bits (view(int32) / view(int64)), with no tolerance anywhere; soft gates
within a bound the test derives from its own weights.

The run is the policy suite's: BatchedPlantEnv.action_test("oil_top_off", ...), dt = 5 s, every plant with a setpoint of its own, under
autoreset with max_episode_steps = 3 from a start bank and the training-loop suite's oil-level / scram task, which ends some episodes
while the step limit truncates others.  Shapes: n in {33, 70} (a ragged last tile; more than two tiles), K * C in {5, 65} (no multiple of
4; one past the small LDS build), H in {6, 33, 65} (a k extension; one past a chunk of 32 outputs; one past the small build), and one case
at n = 64, K * C = 256, H = 128 for the large build's LDS plan; float32 and float64 features."""
import copy

import numpy as np
import pytest
import torch

from nuclear_sim_amd import policy, recurrent
from test_policy_gpu import AXES, DT, F32, F64, _bits, _columns, _np, _same, _setpoint, _step, _weights

pytestmark = pytest.mark.gpu

L = 3
BANK = tuple(range(100, 110))
TASK = dict(reward=[("reward", 1.0), (("pump.oil_level", 0), -0.25, "beyond", "<", 10.0)],
            terminate=[("done", -100.0), (("pump.oil_level", 0), "<", 10.0, -7.0)])
# before step t: an oil level of 4 (the task's limit rule fires) or a fuel temperature of 1500 (a scram) for these plants
POKES = {1: ("oil", [2, 9, 40]), 3: ("fuel", [5, 32]), 6: ("oil", [9, 31, 64]), 10: ("oil", [0, 69])}
U, R = 5.0 * 2.0 ** -24, 2.0 ** -24      # the float tanh's bound; the relative half-ulp of one float rounding


def _core(seed, cells, H):
    """GRUCell's four tensors in its own order, every row's L1 norm between 0.5 and 2: the gates work and do not saturate"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for k in (cells, H):
        W = rng.standard_normal((3 * H, k))
        W *= rng.uniform(0.5, 2.0, (3 * H, 1)) / np.abs(W).sum(axis=1, keepdims=True)
        out.append(W.astype(np.float32))
    return out[0], out[1], (0.1 * rng.standard_normal(3 * H)).astype(np.float32), (0.1 * rng.standard_normal(3 * H)).astype(np.float32)


def _env(n, C, K, fdtype, H, gates="hard", activation="relu", A=3, cdtype=F32, actor=(33, 17), critic=(7,), first=0, autoreset=True, steps=L, bank=True,
         rollout=None, deterministic=False, seed=21, storage="f64"):
    from nuclear_sim_amd.env import BatchedPlantEnv
    kw = dict(autoreset=True, max_episode_steps=steps) if autoreset else {}
    env = BatchedPlantEnv.action_test("oil_top_off", range(first, first + n), dt=DT, storage=storage, bank_seeds=BANK if bank and autoreset else None, **kw)
    env.set_task(**TASK)
    env.set_features(_columns(C), stack=K, dtype=fdtype)
    env.set_controls(AXES[:A], dtype=cdtype)
    if rollout:
        env.set_rollout(rollout, extras=2)
    a, c, log_std = _weights(7 * H + C, H, A, actor, critic)
    env.set_policy(a, c, log_std, activation=activation, seed=seed, deterministic=deterministic, extras=("value", "logp") if rollout else None,
                   first_plant=first, core=_core(H + K * C, K * C, H), gates=gates)
    return env


def _statement(env):
    """the numpy statement of the env's policy, loaded with the parameters the device holds"""
    S = env.policy_spec()
    P = recurrent.Policy(S["cells"], S["n_axes"], S["actor"], S["critic"], S["activation"], S["seed"], S["deterministic"], S["first_plant"],
                         getattr(np, S["act_dtype"]), core=S["core"], gates=S["gates"], n=env.n)
    P.load(_np(env.policy_theta()))
    P.t = int(env.policy_state()["t"])
    return P


def _poke(env, t):
    what, plants = POKES.get(t, (None, []))
    plants = [p for p in plants if p < env.n]
    if plants:
        name, value = ("prim.fuel_temperature", 1500.0) if what == "fuel" else ("pump.oil_level", 4.0)
        v = _np(env.get_field(name))
        v[plants] = value
        env.set_field(name, v)


def _one(env, P, t, first=0, feed_h=False):
    """one step of env and statement: (info, the statement's outputs, the device's hidden state in front of the step)"""
    z = None if P.deterministic else _np(env.policy_noise(int(env.policy_state()["t"])))
    before, h_before = _np(env.features()), _np(env.policy_hidden())
    obs, rew, done, info = _step(env, t, first)
    episode = _np(info["episode_index"]) if "episode_index" in info else None      # the index of the episode the step belonged to
    info["done_"] = done
    return info, P.step(before, episode=episode, z=z, h=h_before if feed_h else None), h_before


def _hold(env, P, info, out, where):
    act, value, logp = out
    _same(env.policy_hidden(), P.h, (where, "hidden")); _same(env.controls_input(), act, (where, "act"))
    _same(info["value"], value, (where, "value")); _same(info["logp"], logp, (where, "logp"))


# ---------------------------------------------------------------------------------------------------------------- 1
CASES = [(33, 5, 1, F32, 6, (33, 17), (7,)), (70, 13, 5, F64, 33, (33, 17), (7,)), (70, 5, 1, F32, 65, (7,), (33, 17)), (33, 13, 5, F64, 6, (64, 64), (7,)),
         (64, 64, 4, F32, 128, (128, 128), (128,))]


@pytest.mark.parametrize("n, C, K, fdtype, H, actor, critic", CASES, ids=["33-5-6", "70-65-33-f64", "70-5-65", "33-65-6-f64", "64-256-128"])
def test_hard_gates_and_relu_nets_bit_for_bit_under_autoreset(n, C, K, fdtype, H, actor, critic):
    """12 sampling steps; after every one hidden, action, value and logp are the statement's bits.  The statement runs on its own hidden
    state (only the device's z is fed, as in the policy suite): the comparison covers the restart rule, on steps where the task ended
    some plants, the step limit others, and the rest ran on"""
    env = _env(n, C, K, fdtype, H, actor=actor, critic=critic)
    P = _statement(env)
    S = env.policy_spec()
    assert S["core"] == H and S["gates"] == "hard" and env.policy_hidden().shape == (n, H) and env.policy_hidden().data_ptr() == env.policy_hidden().data_ptr()
    theta = _np(env.policy_theta())
    assert theta.size == recurrent.theta_size(K * C, 3, actor, critic, H)
    _same(theta[:recurrent.core_size(K * C, H)], recurrent.pack(*_weights(7 * H + C, H, 3, actor, critic), core=_core(H + K * C, K * C, H))[:recurrent.core_size(K * C, H)], "the core in theta")
    kinds, mixed = set(), False
    for t in range(12):
        _poke(env, t)
        info, out, _ = _one(env, P, t)
        _hold(env, P, info, out, t)
        assert np.isfinite(P.h).all() and np.abs(P.h).max() <= 1.0
        restarted = ~P.last_start.any(axis=1)
        mixed |= bool(t > 0 and restarted.any() and not restarted.all())
        kinds |= ({"terminated"} if (_np(info["done_"]) != 0).any() else set()) | ({"truncated"} if (_np(info["truncated"]) != 0).any() else set())
    assert mixed, "no step on which some plants restarted and others did not"
    assert kinds == {"terminated", "truncated"}, kinds
    assert np.ptp(P.h, axis=0).max() > 1e-4      # the plants differ: the cell does read their features
    assert env.policy_state()["t"] == 12
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def _cell_bound(core, xmax):
    """see test_soft_gates_within_the_bound_of_their_own_weights"""
    W_ih, W_hh, b_ih, b_hh = (np.abs(np.asarray(v, dtype=np.float64)) for v in core)
    H = W_hh.shape[1]
    G = float((b_hh[2 * H:] + W_hh[2 * H:].sum(axis=1)).max())
    Gi = float((b_ih[2 * H:] + W_ih[2 * H:].sum(axis=1) * xmax).max())
    dn = U * G + U + R * (4.0 * G + 2.0 * Gi)
    return 2.0 * dn + 2.0 * U + 12.0 * R


def _net_bound(net, e0):
    """the head's error of a tanh net whose input errs by e0 and lies in [-1, 1]: per layer e <- L e + 2 R (k + 1) (L + B) [+ U], L the
    largest row L1 norm, B the largest |bias|, k the padded fan-in"""
    e = e0
    for i, (W, b) in enumerate(net):
        Li, Bi = float(np.abs(W.astype(np.float64)).sum(axis=1).max()), float(np.abs(b).max())
        e = Li * e + 2.0 * R * (W.shape[1] + 4) * (Li + Bi) + (U if i < len(net) - 1 else 0.0)
    return e


@pytest.mark.parametrize("n, C, K, fdtype, H", [(33, 5, 1, F32, 6), (70, 13, 5, F64, 33), (70, 5, 1, F32, 65)], ids=["33-5-6", "70-65-33-f64", "70-5-65"])
def test_soft_gates_within_the_bound_of_their_own_weights(n, C, K, fdtype, H):
    """The one licensed difference is the float tanh, U = 5 * 2^-24 a call.  Every step is compared with the device's h fed back
    (``step(h=)``), so x and h are the same on both sides and gi and gh -- exact fmaf chains -- are the same bits.  With R = 2^-24, the
    relative error of one float rounding, and both sides rounding:
      S = 0.5f * tanh(0.5f * a) + 0.5f errs by U / 2 + 2 R <= U.
      The candidate's pre-activation a = gi_n + r * gh_n: |gh_n[j]| <= G = max_j |b_hh_n[j]| + ||W_hn[j]||_1 (|h| <= 1, asserted), so the
        product errs by U G + 2 R G, and the sum, at most Gi + G large (Gi = max_j |b_ih_n[j]| + ||W_in[j]||_1 max|x|), by 2 R (Gi + G) more.
      n = T(a), T 1-Lipschitz and itself a tanhf: dn <= U G + U + R (4 G + 2 Gi).
      h' = n + z * (h - n), |h - n| <= 2: the difference errs by dn + 4 R, the product by 2 U + dn + 8 R, the sum by 4 R more:
        dh' <= 2 dn + 2 U + 12 R.
    The outputs are then bounded through the nets' row norms (``_net_bound``).  A wrong gate, index or bias errs by about 0.1."""
    env = _env(n, C, K, fdtype, H, gates="soft", activation="tanh", deterministic=True)
    P = _statement(env)
    a, c = P.nets[0], P.nets[1]
    worst = {"h": 0.0, "act": 0.0, "value": 0.0}
    for t in range(9):
        _poke(env, t)
        before = _np(env.features())
        info, (act, value, logp), h_before = _one(env, P, t, feed_h=True)
        bound_h = _cell_bound(P.gru, float(np.abs(before.astype(np.float32)).max()))
        bound_a, bound_c = _net_bound(a, bound_h), _net_bound(c, bound_h)
        assert bound_h < 3e-5 and bound_a < 5e-3 and bound_c < 5e-3, (bound_h, bound_a, bound_c)
        got_h = _np(env.policy_hidden())
        assert np.abs(got_h).max() <= 1.0 and np.abs(h_before).max() <= 1.0
        err_h = np.abs(got_h.astype(np.float64) - P.h).max()
        err_a = np.abs(_np(env.controls_input()).astype(np.float64) - act).max()
        err_c = np.abs(_np(info["value"]).astype(np.float64) - value).max()
        print("soft t=%d: h err %.3e (bound %.3e), actor err %.3e (bound %.3e), critic err %.3e (bound %.3e)" % (t, err_h, bound_h, err_a, bound_a, err_c, bound_c))
        assert err_h <= bound_h and err_a <= bound_a and err_c <= bound_c, (t, err_h, bound_h, err_a, bound_a, err_c, bound_c)
        _same(info["logp"], logp, (t, "logp"))      # deterministic: z = 0, logp is the constant of log_std
        restarted = ~P.last_start.any(axis=1)
        if t == 3:
            assert restarted.any()      # the step limit: the fed-back h was restarted by the statement's own rule
        assert np.ptp(got_h, axis=0).max() > 1e-4      # the plants differ (with 65 cells mostly by one column of order 1, the oil level)
        for k, e in (("h", err_h), ("act", err_a), ("value", err_c)):
            worst[k] = max(worst[k], e)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("autoreset", [False, True], ids=["no-autoreset", "autoreset"])
def test_the_callers_restarts_zero_exactly_the_masked_plants(autoreset):
    """reset(mask), restore(mask) and, with a bank, restore_from_bank(mask) between two steps: the call itself moves no bit of the hidden
    tensor; the next step starts the masked plants from +0.0 (its h' is the statement's, whose masked plants were unprimed) and every
    other plant from its own state"""
    n, H = 70, 33
    env = _env(n, 5, 1, F32, H, autoreset=autoreset, steps=100)
    if not autoreset:
        env.snapshot()
    P = _statement(env)
    t = 0
    for _ in range(2):
        info, out, _ = _one(env, P, t); _hold(env, P, info, out, t); t += 1
    calls = [("reset", np.arange(n) % 7 == 3), ("restore", np.arange(n) % 5 == 1)] + ([("restore_from_bank", (np.arange(n) >= 31) & (np.arange(n) < 34))] if autoreset else [])
    for name, mask in calls:
        held = _np(env.policy_hidden())
        assert held[mask].any()
        getattr(env, name)(torch.as_tensor(mask))
        _same(env.policy_hidden(), held, (name, "the call itself"))
        P.unprime(mask)
        info, out, h_before = _one(env, P, t)
        assert np.array_equal(~P.last_start.any(axis=1), mask), name      # exactly the masked plants started from zeros
        _hold(env, P, info, out, name)
        t += 1
        info, out, _ = _one(env, P, t); _hold(env, P, info, out, (name, "the step after")); t += 1
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_the_recorded_state_suffices_for_replay_bootstraps_and_last_value():
    """One step, a reset of some plants (so that the episodes' phases differ), then rollout_begin and collect(8) under max_episode_steps
    = 3: truncations fall inside the rollout and on its last slot, and `first` is not zeros.  From the rollout's own tensors
    recurrent.replay reproduces every slot's recorded action, value and logp by bits; policy_values(final_obs, hidden=final) are the
    statement's terminal values; policy_values() is the statement's last_value, zeros for the plants that restarted on the last step"""
    from nuclear_sim_amd.env import BatchedPlantEnv
    n, T, A, H = 70, 8, 3, 33
    env = BatchedPlantEnv(n, dt=DT, autoreset=True, max_episode_steps=L)
    env.set_features(_columns(5), stack=3, dtype=F32)
    env.set_controls(AXES[:A])
    env.set_rollout(T, extras=2)
    a, c, log_std = _weights(8, H, A, (33, 17), (7,))
    env.set_policy(a, c, log_std, activation="relu", seed=21, extras=("value", "logp"), core=_core(3, 15, H), gates="hard")
    P = _statement(env)
    env.step()
    early = np.arange(n) % 3 == 1
    env.reset(torch.as_tensor(early))
    env.rollout_begin()
    r = env.collect(T)
    rh = env.policy_rollout_hidden()
    assert r["t"] == T and rh["first"].shape == (n, H) and rh["final"].shape == (r["final_obs"].shape[0], H) and r["final_obs"].shape[0] == n * L
    first, obs, episode, ended, final_row = _np(rh["first"]), _np(r["obs"]), _np(r["episode"]), _np(r["ended"]), _np(r["final_row"])
    assert not first[early].any() and first[~early].any(axis=1).all()      # the reset plants start from zeros, the others from their own state
    assert (ended[T - 1] & 2).any() and not (ended[T - 1] & 2).all() and (ended[1:T - 1] & 2).any()
    states = recurrent.replay(first, obs, episode, ended, P.gru, "hard")
    after = np.zeros_like(states)
    for t in range(T):
        after[t], bad = recurrent.advance(P.gru, obs[t], states[t], "hard")
        assert not bad.any()
        z = _np(env.policy_noise(1 + t))      # (one draw went to the step before the rollout)
        act, value, logp = policy.outputs(policy.forward(P.nets[0], after[t], "relu"), policy.forward(P.nets[1], after[t], "relu")[:, 0], P.nets[2], P.nets[3], z, obs[t])
        _same(r["act"][t], act, (t, "act")); _same(r["extra"][t, :, 0], value, (t, "value")); _same(r["extra"][t, :, 1], logp, (t, "logp"))
    # the terminal states: final[row] is the h' of the truncated step, and the critic over GRU(final_obs[row], final[row]) is the statement's
    final, taken = _np(rh["final"]), 0
    for t, p in zip(*np.nonzero(final_row >= 0)):
        assert ended[t, p] & 2
        _same(final[final_row[t, p]], after[t, p], ("final", t, p)); taken += 1
    assert taken == int((ended & 2).astype(bool).sum()) > 0
    _same(env.policy_values(r["final_obs"], hidden=rh["final"]), P.values(_np(r["final_obs"]), hidden=final), "final_values")
    # last_value: the live state under the restart rule
    over = (ended[T - 1] & 3) != 0
    P.h, P.seen, P.primed = after[T - 1].copy(), episode[T - 1].copy(), np.ones(n, np.int32)
    want = P.values(_np(env.features()), episode=episode[T - 1] + over)
    held = _np(env.policy_hidden())
    _same(env.policy_values(), want, "last_value")
    _same(env.policy_hidden(), held, "policy_values() writes nothing back")
    _same(held, after[T - 1], "the live state is the last slot's h'")
    h0, _ = recurrent.advance(P.gru, _np(env.features())[over], np.zeros((int(over.sum()), H), np.float32), "hard")
    _same(want[over], policy.forward(P.nets[1], h0, "relu")[:, 0], "a plant that restarted on the last step bootstraps from +0.0")
    # and the advantages take them
    adv, ret = env.rollout_advantages(0.99, 0.95, values=("extra", 0), last_value=env.policy_values(), final_values=env.policy_values(r["final_obs"], hidden=rh["final"]))
    assert np.isfinite(_np(adv)).all() and np.isfinite(_np(ret)).all()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_a_batch_equals_its_shards():
    """70 plants, and the same plants as handles of 33 and 37 with first_plant set: the same bits in every output and in hidden"""
    kw = dict(C=13, K=5, fdtype=F32, H=33, bank=False)
    whole, left, right = _env(70, **kw), _env(33, **kw), _env(37, first=33, **kw)
    for t in range(6):
        _step(whole, t); _step(left, t); _step(right, t, 33)
        for name, get in (("hidden", lambda e: e.policy_hidden()), ("act", lambda e: e.controls_input()), ("value", lambda e: e.policy_outputs()["value"]),
                          ("logp", lambda e: e.policy_outputs()["logp"])):
            _same(np.concatenate([_np(get(left)), _np(get(right))]), get(whole), (t, name))
    assert _np(whole.policy_hidden()).any()
    for e in (whole, left, right):
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_a_checkpoint_resumes_bit_for_bit():
    """policy_state() after 5 steps and a reset of some plants (they are unprimed in it), into a fresh env with the same state arrays:
    steps 6 to 10 are identical; without the core's part of the state they are not"""
    n, H = 70, 33
    noise = np.random.default_rng(11).standard_normal((10, n))

    def fresh():
        return _env(n, 5, 3, F32, H, autoreset=False)

    def run(env, first, steps):
        out = []
        for t in range(first, first + steps):      # (the heat-source noise comes from the test: a fresh env's own stream would start over)
            _, _, _, info = env.step(power_setpoint=_setpoint(t, n), noise_z=noise[t])
            out.append((_np(env.policy_hidden()), _np(env.controls_input()), _np(info["value"]), _np(info["logp"])))
        return out
    a = fresh()
    run(a, 0, 5)
    mask = np.arange(n) % 4 == 2
    a.reset(torch.as_tensor(mask))
    state = a.policy_state()
    assert set(state) == {"t", "hidden", "seen", "primed"} and state["t"] == 5 and state["hidden"].shape == (n, H) and state["hidden"].dtype == np.float32
    assert np.array_equal(state["primed"] == 0, mask) and state["hidden"][mask].any()
    f, i = a.state_arrays()
    saved = dict(f=f.clone(), i=i.clone(), features=a.features_state(), stack=_np(a.features()), task=a.task_state(), controls=a.controls_state())
    want = run(a, 5, 5)

    def loaded(policy_state):
        b = fresh()
        b.load_state_arrays(saved["f"], saved["i"])
        b.load_features_state(saved["features"], saved["stack"])
        b.load_task_state(saved["task"])
        b.load_controls_state(saved["controls"])
        b.load_policy_state(policy_state)
        return b
    b = loaded(state)
    _same(b.policy_hidden(), state["hidden"], "the loaded hidden state")
    got = run(b, 5, 5)
    for t, (g, w) in enumerate(zip(got, want)):
        for name, x, y in zip(("hidden", "act", "value", "logp"), g, w):
            _same(x, y, (5 + t, name))
    # teeth: every plant primed -- the reset plants carry their stale state on
    c = loaded(dict(state, primed=np.ones(n, np.int32)))
    other = run(c, 5, 1)
    assert not np.array_equal(other[0][0][mask], want[0][0][mask])
    _same(other[0][0][~mask], want[0][0][~mask], "the other plants")
    for e in (a, b, c):
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_off_is_off_and_training_is_refused_by_name():
    from nuclear_sim_amd._lib import NpbError
    from nuclear_sim_amd.env import BatchedPlantEnv
    n, A, T = 70, 3, 4

    def plain(core):
        env = BatchedPlantEnv(n, dt=DT)
        env.set_features(_columns(5), stack=3, dtype=F32)
        env.set_controls(AXES[:A])
        env.set_rollout(T, extras=2)
        a, c, log_std = _weights(8, 33 if core else 15, A, (33, 17), (7,))
        env.set_policy(a, c, log_std, activation="relu", seed=21, extras=("value", "logp"), **(dict(core=core, gates="hard") if core else {}))
        return env
    arrays = _core(3, 15, 33)
    gru = torch.nn.GRUCell(15, 33)      # (the core as a torch module: its parameters are read in GRUCell's own order)
    with torch.no_grad():
        for p, v in zip((gru.weight_ih, gru.weight_hh, gru.bias_ih, gru.bias_hh), arrays):
            p.copy_(torch.as_tensor(v))
    off = plain(False)
    assert set(off.policy_state()) == {"t"} and off.policy_spec()["core"] is None
    off.collect(T)
    for call in (lambda: off.policy_values(off.features(), hidden=torch.zeros((n, 33))), off.policy_rollout_hidden, off.policy_hidden):
        with pytest.raises(NpbError, match="no core"):
            call()
    assert off.policy_values().shape == (n,)
    on = plain(gru)
    on.collect(T)
    on.rollout_advantages(0.99, 0.95, values=("extra", 0), last_value=on.policy_values())
    batch = next(on.rollout_minibatches(T * n, 1, seed=3))
    with pytest.raises(NpbError, match="training through time is not built"):
        on.policy_grad(batch, rows_per_chain=64)
    with pytest.raises(NpbError, match="training through time is not built"):
        on.policy_train(T * n // 2, 1, seed=3, rows_per_chain=64)
    with pytest.raises(ValueError, match="hidden"):
        on.policy_values(on.features())
    # whole sequences for a learner outside: unit="plant" keeps them whole, and the longer theta goes back in
    seq = next(on.rollout_minibatches(n, 1, seed=3, unit="plant"))
    assert seq["obs"].shape[:2] == (T, n)
    theta = _np(on.policy_theta())
    a, c, log_std = _weights(8, 33, A, (33, 17), (7,))
    _same(theta[:-A], recurrent.pack(a, c, log_std, core=arrays)[:-A], "theta from a GRUCell is recurrent.pack's")
    on.policy_load(theta)
    _same(on.policy_theta(), theta, "theta through policy_load")
    on.policy_load((arrays, a, c, log_std))
    _same(on.policy_theta(), theta, "(core, actor, critic, log_std) through policy_load")
    with pytest.raises(ValueError):
        on.policy_load(theta[:-1])
    off.close(); on.close()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_a_second_policy_load_lays_out_every_layer_behind_a_core():
    """33 plants (two tiles, the second ragged), 5 cells (a live k extension), H = 6, hard gates, relu nets, deterministic.  theta_a, one
    step; policy_load of a theta_b whose six gate layers, every net layer and log_std all differ; one more step.  After each step hidden,
    action, value and logp are the statement's bits under the parameters then loaded: one layer left at theta_a in the kernel's own copy
    of the weights would show.  Teeth: the second step under theta_a, from the same state, gives another hidden state and another action"""
    n, C, K, H, A, actor, critic = 33, 5, 1, 6, 3, (33, 17), (7,)
    env = _env(n, C, K, F32, H, actor=actor, critic=critic, deterministic=True)
    theta_a = _np(env.policy_theta())
    theta_b = recurrent.pack(*_weights(501, H, A, actor, critic), core=_core(502, K * C, H))
    core_a, actor_a, critic_a, log_std_a, _ = recurrent.unpack(theta_a, K * C, A, actor, critic, H)
    core_b, actor_b, critic_b, log_std_b, _ = recurrent.unpack(theta_b, K * C, A, actor, critic, H)
    for gate in range(3):      # W_ih's and W_hh's row blocks r, z, n with their biases: the six gate layers
        rows = slice(gate * H, (gate + 1) * H)
        assert all((x[rows] != y[rows]).all() for x, y in zip(core_a, core_b))
    assert all((Wa != Wb).all() and (ba != bb).all() for (Wa, ba), (Wb, bb) in zip(actor_a + critic_a, actor_b + critic_b)) and (log_std_a != log_std_b).all()
    env.policy_load(theta_a)
    P = _statement(env)
    info, out, _ = _one(env, P, 0)
    _hold(env, P, info, out, "theta_a")
    env.policy_load(theta_b)
    stale = copy.deepcopy(P)      # the statement that goes on under theta_a
    P.load(_np(env.policy_theta()))
    _same(P.theta[:-A], theta_b[:-A], "theta_b on the device")
    before = _np(env.features())
    info, out, _ = _one(env, P, 1)
    _hold(env, P, info, out, "theta_b")
    old_act, _, _ = stale.step(before, episode=_np(info["episode_index"]))
    assert not np.array_equal(_bits(stale.h), _bits(env.policy_hidden())) and not np.array_equal(_bits(old_act), _bits(env.controls_input()))
    env.close()
