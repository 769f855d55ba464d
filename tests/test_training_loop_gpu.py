"""GPU: a whole PPO iteration with every per-step attachment on at once -- a task, features with a frame stack, the running normaliser,
controls, the rollout, the policy and its training step on ONE handle, with autoreset from a start bank -- where each single suite runs
its own link alone.  npb_step's launch order (policy, rollout pre, controls, step, task, normaliser partials, finish and reward kernels,
features pass A, rollout post, episode kernel, stream restart, features pass B) has many places where a combination can read the wrong
generation of a buffer while every single-feature suite stays green.

The configuration is set in the only order the handle accepts (``_configure``, ``_with_policy``): action_test("oil_top_off", autoreset,
max_episode_steps 3, a start bank), the features suite's oil-level / scram task, eight columns of which the normaliser takes six and must
leave two alone (a BITS column, a column whose ref is a second column), ``set_normalizer("all", reward=...)``, controls, a rollout of 8
slots with two extras, the policy writing value and logp into them.  Steps take the policy suite's per-plant setpoints; an oil level and
a fuel temperature are poked so that the task ends some episodes while max_episode_steps truncates others.

The references are the numpy statements (normalizer.py, features.py, policy.py, ppo.py) and float64 torch autograd; comparisons are by
bits wherever the statements promise bits.  The bounds that are not bits are computed from the test's own data; test_training_loop_cpu.py
checks them on the statements alone.  The runs of tests 2 to 4 are made once per case and shared (``runs``)."""
import numpy as np
import pytest
import torch

from nuclear_sim_amd import features, policy, ppo
from test_policy_gpu import AXES, F32, F64, _bits, _np, _same, _setpoint, _statement, _step, _weights
from test_ppo_cpu import CLIP, ENT, VF, autograd, pooled, split
from test_training_loop_cpu import LOG_RATIO_SLACK, logp_bound

pytestmark = pytest.mark.gpu

DT, K, L, T = 5.0, 3, 3, 8
BANK = tuple(range(100, 110))
TASK = dict(reward=[("reward", 1.0), (("pump.oil_level", 0), -0.25, "beyond", "<", 10.0)],
            terminate=[("done", -100.0), (("pump.oil_level", 0), "<", 10.0, -7.0)])
COLUMNS = [(("pump.oil_level", 0), {"ref": 50.0, "scale": 0.1, "clip": (-5.0, 5.0)}),          # 0 a carried member
           ("obs", 3),                                                                          # 1 the observation
           (("info", "electrical_power"), {"ref": 900.0, "scale": 0.01, "fresh": 900.0}),      # 2 a side column with a fresh value
           (("sg.tube_wall_temp", 1), {"clip": (-10.0, 10.0)}),                                 # 3 an output member
           ("task_reward", {"scale": 0.5, "fresh": -1.0, "clip": (-5.0, 5.0)}),                 # 4 the task's reward
           ("flags", {"bits": 0xF00}),                                                          # 5 BITS: left alone
           (("obs", 5), {"ref": ("obs", 6)}),                                                   # 6 a second column as ref: left alone
           ("maintenance", {"scale": 0.25})]                                                    # 7 an int32 member
C = len(COLUMNS)
ELIGIBLE, LIVE = [0, 1, 2, 3, 4, 7], [0, 1, 3]      # what "all" takes; of those, the ones a fresh frame reads live
# before step t: an oil level of 4 (the task's limit rule fires, alone on that step), a fuel temperature of 1500 (a scram, on a step where
# max_episode_steps truncates the others); plants past the batch are left out
POKES = {1: {"oil": [9, 64, 257]}, 2: {"fuel": [5, 299]}}
HYPER = dict(clip=CLIP, vf_coef=VF, ent_coef=ENT, max_grad_norm=0.5)
GAMMA, LAM, CHAIN, LR = 0.99, 0.95, 64, 1e-3


def _configure(n, storage="f64", fdtype=F32, A=3, cdtype=F32, autoreset=True, normalizer=True, rollout=True, bank=True):
    from nuclear_sim_amd.env import BatchedPlantEnv
    kw = dict(autoreset=True, max_episode_steps=L) if autoreset else {}
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, storage=storage, bank_seeds=BANK if bank else None, **kw)
    env.set_task(**TASK)
    env.set_features(COLUMNS, stack=K, dtype=fdtype, final=autoreset)
    if normalizer:
        env.set_normalizer("all", reward={"gamma": 0.99, "clip": 5.0})
    env.set_controls(AXES[:A], dtype=cdtype)
    if rollout:
        env.set_rollout(T, extras=2)
    return env


def _with_policy(env, A, activation="relu", deterministic=False):
    a, c, log_std = _weights(env.n + A, K * C, A, (64, 64), (33, 17))
    env.set_policy(a, c, log_std, activation=activation, seed=21, deterministic=deterministic, extras=("value", "logp"))
    return env


def _poke(env, t):
    for what, plants in POKES.get(t, {}).items():
        plants = [p for p in plants if p < env.n]
        name, value = ("prim.fuel_temperature", 1500.0) if what == "fuel" else ("pump.oil_level", 4.0)
        v = _np(env.get_field(name))
        v[plants] = value
        env.set_field(name, v)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("n, storage, fdtype", [(70, "f64", F64), (300, "f32", F32)], ids=["70-f64", "300-f32"])
def test_normalised_columns_under_autoreset_bit_for_bit(n, storage, fdtype):
    """No policy: the caller writes the controls.  The twin has neither autoreset nor a normaliser, takes the same inputs and is restored
    from the bank by hand; per step the statement folds the twin's samples (with the TASK's reward and done), puts the table into the
    stack's spec, runs pass A and, behind the restore, pass B.  The state, the stacks, the final stacks and the normalised reward are its
    bits: pass B ran under the table the finish kernel rewrote two launches earlier.  300 plants: two groups of the tree, one ragged"""
    A = 3
    env = _configure(n, storage, fdtype)
    twin = _configure(n, storage, fdtype, autoreset=False, normalizer=False, rollout=False)
    spec0, Z = env.features_spec()["spec"], env.normalizer_spec()
    assert Z.columns == ELIGIBLE and Z.S == len(ELIGIBLE) + 1
    ref = features.Stack(spec0, n, final=True)
    sentinel = -(1000.0 + np.arange(n * K * C)).reshape(n, K, C)
    env.final_features().copy_(torch.as_tensor(sentinel).to(env.final_features()))
    ref.final[:] = sentinel
    twin.features()      # (the observation current: a fresh frame reads it live)
    assert ref.prime(_np(twin.features_samples())).all()
    _same(env.features(), ref.out, "primed with the set-time table")
    index, length = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
    both_kinds = some_not_others = False
    for t in range(T):
        _poke(env, t); _poke(twin, t)
        ctl = torch.as_tensor(0.5 * np.random.default_rng(50 + t).standard_normal((n, A)), dtype=F32)
        obs, rew, done, info = env.step(power_setpoint=_setpoint(t, n), controls=ctl)
        t_obs, t_rew, t_done, _ = twin.step(power_setpoint=_setpoint(t, n), controls=ctl)
        t_obs = t_obs.clone()
        _same(rew, t_rew, ("the twin strayed: reward", t))
        assert torch.equal(done, t_done), ("the twin strayed: done", t)
        assert "reference_reward" in info      # (the reward and done the normaliser reads are the task's)
        samples = _np(twin.features_samples())
        nr = Z.step(samples, _np(t_rew), _np(t_done), index)      # 1. the fold, with the index the transition belonged to
        ref.spec = Z.apply()                                      # 2. the table
        assert not ref.step(samples, index).any()                 # 3. pass A: every plant is primed and of the episode seen
        length += 1
        ended = (_np(t_done) != 0) | (length >= L)
        truncated = _np(info["truncated"]) != 0
        assert np.array_equal(ended, (_np(done) != 0) | truncated), t
        assert np.array_equal(_np(info["episode_index"]), index), t
        both_kinds |= bool((_np(done) != 0).any() and truncated.any())
        some_not_others |= bool(ended.any() and not ended.all())
        if ended.any():
            twin.restore_from_bank(torch.as_tensor(ended))
        index[ended] += 1; length[ended] = 0
        now = torch.as_tensor(ended, device=obs.device)
        _same(obs[now], twin.get_observation()[now], ("the twin strayed: restored rows", t))
        _same(obs[~now], t_obs[~now], ("the twin strayed: stepped rows", t))
        after = _np(twin.features_samples())
        assert np.array_equal(ref.restart(after, index), ended), t      # 4. pass B, with the table as it stands
        state = env.normalizer_state()
        for name, want in Z.state().items():
            _same(state[name], want, (t, name))
        _same(info["features"], ref.out, (t, "features"))
        _same(info["final_features"], ref.final, (t, "final_features"))
        _same(info["norm_reward"], nr, (t, "norm_reward"))
        # a restarted plant's fresh frame is not what the set-time ref / scale would give: the table was the rewritten one
        stale = features.frame(after, spec0, fresh=True)
        for p in np.flatnonzero(ended):
            assert all(np.array_equal(_bits(ref.out[p, k]), _bits(ref.out[p, 0])) for k in range(K)), (t, p)
            assert not np.array_equal(_bits(ref.out[p, -1, LIVE]), _bits(stale[p, LIVE])), (t, p)
    assert both_kinds, "no step with a task termination and a truncation"
    assert some_not_others, "no step on which some plants restarted and others did not"
    assert env.normalizer_state()["count"].tolist() == [float(T * n)] * Z.S      # fresh frames are not folded
    assert not np.any(_np(env.final_features()) == sentinel.astype(ref.final.dtype))      # every plant restarted at least once
    env.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- the shared runs
CASES = {"relu-70": (70, 3, F32, "f64", F32, "relu", False), "relu-257": (257, 8, F64, "f32", F64, "relu", False),
         "tanh-70": (70, 3, F32, "f64", F32, "tanh", False), "deterministic-70": (70, 3, F32, "f64", F32, "relu", True)}


def _collect(n, A, cdtype, storage, fdtype, activation, deterministic):
    """T steps of the full configuration; kept: the env (its rollout full), every step's norm_reward and the table behind it"""
    env = _with_policy(_configure(n, storage, fdtype, A, cdtype), A, activation, deterministic)
    rewards, tables = [], []
    for t in range(T):
        _poke(env, t)
        _, _, _, info = _step(env, t)
        rewards.append(_np(info["norm_reward"]))
        tables.append(env.normalizer_stats())
    return {"env": env, "norm_reward": np.stack(rewards), "tables": tables, "n": n, "A": A}


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = _collect(*CASES[case])
        return cache[case]
    yield get
    for R in cache.values():
        R["env"].close()


def _recorded(R):
    """what every test on a shared run first asserts of it: the rollout is full, finite, and episodes ended inside it both ways"""
    r = R["env"].rollout()
    assert r["t"] == T and np.isfinite(_np(r["obs"])).all()
    ended = _np(r["ended"])
    assert (ended & 2).any() and (ended & 1).any()
    first, last = R["tables"][0], R["tables"][-1]
    assert not np.array_equal(first["mean"], last["mean"]) and not np.array_equal(first["scale"], last["scale"])      # the table moved
    return r


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("case", ["relu-70", "relu-257"])
def test_the_policy_read_what_the_rollout_recorded(runs, case):
    """Re-running the statement on the recorded rows with the device's own z and theta gives back the recorded action, value and
    log-probability by bits; the recorded reward is every step's norm_reward; policy_values on the final rows and on the current
    features are the statement's"""
    R = runs(case)
    env, r = R["env"], _recorded(R)
    P = _statement(env)
    assert P.t == T
    for t in range(T):
        act, value, logp = P.step(_np(r["obs"][t]), z=_np(env.policy_noise(t)))
        _same(r["act"][t], act, (t, "act")); _same(r["extra"][t, :, 0], value, (t, "value")); _same(r["extra"][t, :, 1], logp, (t, "logp"))
    assert _np(r["act"]).std() > 0 and np.ptp(_np(r["extra"][:, :, 0])) > 0
    _same(r["reward"], R["norm_reward"], "the recorded reward is the normalised one")
    _same(env.policy_values(r["final_obs"]), P.values(_np(r["final_obs"])), "final_values")
    _same(env.policy_values(), P.values(_np(env.features())), "last_value")


def test_the_recorded_tanh_value_is_the_critic_of_the_recorded_rows(runs):
    """By bits, not within test_tanh_within_the_bound_of_its_own_weights' bound: the step's launch and npb_policy_values are ONE
    instantiation of npb_policy_kernel (npb_launch_policy picks it by the input type and the size alone; whether the actor runs is a
    runtime flag), so the same float tanh runs on the same rows.  logp does not pass the nets: the statement's bits"""
    R = runs("tanh-70")
    env, r = R["env"], _recorded(R)
    P = _statement(env)
    for t in range(T):
        _same(env.policy_values(r["obs"][t]), r["extra"][t, :, 0], (t, "value"))
        _same(r["extra"][t, :, 1], P.step(_np(r["obs"][t]), z=_np(env.policy_noise(t)))[2], (t, "logp"))
    _same(r["reward"], R["norm_reward"], "the recorded reward is the normalised one")


# ---------------------------------------------------------------------------------------------------------------- 3
def _advantages(env):
    r = env.rollout()
    final = None if r["final_obs"] is None else env.policy_values(r["final_obs"])
    return env.rollout_advantages(GAMMA, LAM, values=("extra", 0), last_value=env.policy_values(), final_values=final)


def _stat(stats, name):
    return float(_np(stats)[ppo.STATS.index(name)])


@pytest.mark.parametrize("case", ["relu-70", "relu-257", "tanh-70", "deterministic-70"])
def test_an_unchanged_policy_gives_its_own_logp_back(runs, case):
    """policy_grad before any update, on the two minibatches of one epoch: value_new is the recorded value by bits (tanh too: the
    gradient's forward pass is the step's own layer routine), no row is skipped or clipped, and |logp_new - logp_old| stays under the
    bound test_training_loop_cpu.py derives, computed per row from the minibatch's own action, the z that made it (policy_noise through
    the row indices), std and logp_old.  A row beyond it means the rollout's act / obs are not what the policy wrote or read; the
    ratio's 4 ulp licence cannot be the cause, it moves no logp.  Deterministic: d is exactly 0, logp_new is logp_old by bits.
    Measured on an MI355X, the largest diff / bound over both minibatches: relu-70 0.874 (170 of 560 rows differ in some bit), tanh-70
    0.833 (177 of 560); relu-257, float64 controls, and deterministic-70: 0.000, logp_new is logp_old by bits on every row.  The largest
    |log ratio| over its bound: 0.593, 0.548, 0.333 and 0.098"""
    R = runs(case)
    env, n, A = R["env"], R["n"], R["A"]
    _recorded(R)
    deterministic = env.policy_spec()["deterministic"]
    _advantages(env)
    theta = _np(env.policy_theta())
    std = theta[-A:].astype(np.float64)
    z_all = np.zeros((T * n, A)) if deterministic else np.concatenate([_np(env.policy_noise(t)) for t in range(T)])      # [s * n + p, a]
    B, seen, worst = T * n // 2, 0, 0.0
    for batch in env.rollout_minibatches(B, 1, seed=3):
        got = env.policy_grad(batch, rows_per_chain=CHAIN, diagnostics=True, **HYPER)
        index, act, extra = _np(batch["index"]), _np(batch["act"]), _np(batch["extra"])
        assert len(index) == B
        _same(got["value_new"], extra[:, 0], "value_new is the recorded value")
        assert _stat(got["stats"], "skipped") == 0 and _stat(got["stats"], "clip_fraction") == 0.0 and _stat(got["stats"], "count") == B
        assert _stat(got["stats"], "approx_kl") >= 0.0
        old, new = extra[:, 1], _np(got["logp_new"])
        bound, ulp = logp_bound(act, z_all[index], std, old)
        diff = np.abs(new.astype(np.float64) - old.astype(np.float64))
        log_ratio = np.abs(np.log(_np(got["ratio"])))
        worst = max(worst, float((diff / bound).max()))
        print("%s, minibatch %d: the largest diff / bound %.3f, %d of %d rows differ in some bit; the largest |log ratio| / its bound %.3f"
              % (case, seen, (diff / bound).max(), int((diff != 0).sum()), B, (log_ratio / (bound + 0.5 * ulp)).max()))
        assert (diff <= bound).all(), (case, np.flatnonzero(diff > bound)[:4].tolist())
        if deterministic:
            _same(new, old, "deterministic: logp_new is logp_old")
            assert (log_ratio <= 0.5 * ulp + LOG_RATIO_SLACK).all()
        else:
            assert (log_ratio <= bound + 0.5 * ulp + LOG_RATIO_SLACK).all()
        seen += 1
    assert seen == 2
    print("%s: the largest diff / bound over both minibatches %.3f" % (case, worst))


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("case, licence", [("relu-70", 4.0), ("tanh-70", 8.0)])
def test_the_gradient_of_a_real_minibatch_against_float64_autograd(runs, case, licence):
    """The first minibatch of the run as host copies: normalised advantages, ratios next to 1, features through the normaliser's scale.
    The yardstick is a reference's own pooled distance from float64 autograd on the same rows, never the device's.  relu: float32
    autograd's, 4 times as far allowed (the CPU suite's contract for the statement, whose bits the device gives).  tanh: the statement's,
    8 times as far allowed (the GPU suite's licence for the device's float tanh).
    Measured on an MI355X (280 rows of 24 cells, actor (64, 64), critic (33, 17), 3 axes, chains of 64): relu-70, the device 6.340e-7
    (the statement's own figure: it gives the statement's bits), float32 autograd 8.004e-7, factor 0.79; tanh-70, the device 4.697e-7, the
    statement 4.080e-7, factor 1.15 (float32 autograd 5.257e-7).  The nearest ratio to a clip boundary is 0.200 away: every ratio lies next to 1"""
    R = runs(case)
    env = R["env"]
    _recorded(R)
    _advantages(env)
    S, theta = env.policy_spec(), _np(env.policy_theta())
    A, B = S["n_axes"], T * R["n"] // 2
    gen = env.rollout_minibatches(B, 1, seed=3)
    batch = next(gen)
    host = {"obs": _np(batch["obs"]).reshape(B, -1), "act": _np(batch["act"]), "logp_old": _np(batch["extra"])[:, 1], "adv": _np(batch["adv"]),
            "ret": _np(batch["ret"])}
    hyper = dict(HYPER, max_grad_norm=0.0)
    got = env.policy_grad(batch, rows_per_chain=CHAIN, diagnostics=True, **hyper)
    grad, norm = _np(got["grad"]), _stat(got["stats"], "grad_norm")
    gen.close()
    assert host["adv"].std() > 0.5 and np.ptp(host["adv"]) > 1.0      # the advantages have spread (normalised: a std next to 1)
    g64, r = autograd(theta, S["cells"], A, S["actor"], S["critic"], S["activation"], host, torch.float64)
    near = min(np.abs(r - (1 + CLIP)).min(), np.abs(r - (1 - CLIP)).min())
    print("nearest ratio to a clip boundary: %.2e" % near)
    assert near > 1e-4
    cut = lambda g: split(g, S["cells"], A, S["actor"], S["critic"])
    mine = pooled(cut(grad), g64)
    g32, _ = autograd(theta, S["cells"], A, S["actor"], S["critic"], S["activation"], host, torch.float32)
    own = ppo.gradient(theta, S["cells"], A, S["actor"], S["critic"], S["activation"], rows_per_chain=CHAIN, **host, **hyper)
    by_autograd, by_statement = pooled(g32, g64), pooled(cut(own["grad"]), g64)
    yard = by_autograd if S["activation"] == "relu" else by_statement
    print("%s: pooled distance from float64: the device %.3e, float32 autograd %.3e, the statement %.3e; the device stands %.2f times as far as its "
          "yardstick (%.0f allowed)" % (case, mine, by_autograd, by_statement, mine / yard, licence))
    assert mine <= licence * yard
    assert abs(norm - np.sqrt(sum((g ** 2).sum() for g in g64))) < 1e-5 * norm
    assert not grad[-A:].any()      # std is derived: no gradient


# ---------------------------------------------------------------------------------------------------------------- 5
def test_a_training_run_resumes_from_a_checkpoint_to_the_same_bits():
    """Autoreset off, as in the single suites' checkpoint tests; 70 plants, a tanh net, sampling.  Iteration 1 (8 steps, advantages,
    policy_train over one epoch of two minibatches), then every getter's piece is saved and loaded into a fresh env set up the same way:
    iteration 2 is the original's by bits -- the rollout, the stats, theta, Adam's state and the normaliser's.  The heat-source noise is
    given per step (noise_z), as the features and normaliser checkpoint tests give it: the host generator is the caller's input, not
    state of the handle.  No piece of carried state lacked a getter.  A third env loaded without the normaliser's state strays from the
    second recorded row on: the comparison would notice a piece that was not restored"""
    n, A = 70, 3
    z = np.random.default_rng(7).standard_normal((2 * T, n))

    def fresh():
        return _with_policy(_configure(n, "f64", F32, A, F32, autoreset=False, bank=False), A, "tanh")

    def iteration(env, first):
        for t in range(first, first + T):
            env.step(power_setpoint=_setpoint(t, n), noise_z=z[t])
        _advantages(env)
        stats = env.policy_train(T * n // 2, 1, seed=3 + first, rows_per_chain=CHAIN, lr=LR, **HYPER)
        r = env.rollout()
        assert r["t"] == T and stats.shape == (2, len(ppo.STATS))
        out = {name: _np(r[name]) for name in ("obs", "act", "extra", "reward")}
        out.update(stats=_np(stats), theta=_np(env.policy_theta()), normalizer=env.normalizer_state(), **env.policy_optimizer_state())
        return out
    a = fresh()
    theta0 = _np(a.policy_theta())
    one = iteration(a, 0)
    assert one["step"] == 2 and not np.array_equal(one["theta"][:-2 * A], theta0[:-2 * A])
    f, i = a.state_arrays()
    saved = dict(f=f.clone(), i=i.clone(), features=a.features_state(), stack=_np(a.features()), task=a.task_state(), controls=a.controls_state(),
                 normalizer=a.normalizer_state(), theta=_np(a.policy_theta()), policy=a.policy_state(), optimizer=a.policy_optimizer_state())
    assert saved["policy"]["t"] == T and saved["features"]["primed"].all()
    b = fresh()
    b.load_state_arrays(saved["f"], saved["i"])
    b.load_features_state(saved["features"], saved["stack"])
    b.load_task_state(saved["task"])
    b.load_controls_state(saved["controls"])
    b.load_normalizer_state(saved["normalizer"])
    b.policy_load(saved["theta"])
    b.load_policy_state(saved["policy"])
    b.load_policy_optimizer_state(saved["optimizer"])
    a.rollout_begin(); b.rollout_begin()
    two, again = iteration(a, T), iteration(b, T)
    assert two["step"] == 4 and not np.array_equal(two["theta"], one["theta"]) and not np.array_equal(two["obs"], one["obs"])
    for name in ("obs", "act", "extra", "reward", "stats", "theta", "m", "v"):
        _same(again[name], two[name], name)
    assert again["step"] == two["step"]
    for name, want in two["normalizer"].items():
        _same(again["normalizer"][name], want, ("normalizer", name))
    assert two["normalizer"]["count"].tolist() == [float(2 * T * n)] * (len(ELIGIBLE) + 1)
    # ... and the comparison has teeth: the same pieces without the normaliser's state give other features from the first step on
    c = fresh()
    c.load_state_arrays(saved["f"], saved["i"])
    c.load_features_state(saved["features"], saved["stack"])
    c.load_task_state(saved["task"])
    c.load_controls_state(saved["controls"])
    c.policy_load(saved["theta"])
    c.load_policy_state(saved["policy"])
    c.load_policy_optimizer_state(saved["optimizer"])
    other = iteration(c, T)
    _same(other["obs"][0], two["obs"][0], "the first recorded rows are the loaded stack")
    assert not np.array_equal(other["obs"][1], two["obs"][1]) and not np.array_equal(other["theta"], two["theta"])
    a.close(); b.close(); c.close()
