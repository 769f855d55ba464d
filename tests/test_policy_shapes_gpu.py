"""GPU: the policy's forward launch (npb_policy.hip, npd_policy_layer) and the training kernels (npb_ppo.hip: gradient, reduce, finish,
Adam) at the shapes and settings where they have logic of their own and the two older suites (test_policy_gpu.py, test_ppo_gpu.py) never
went -- against the same numpy statements (nuclear_sim_amd.policy, nuclear_sim_amd.ppo), by the same contracts and through the same helpers:
a relu net by bits, the ratio within 4 ulp, a tanh gradient within 8 times the statement's distance from float64 autograd, Adam's m, v and
theta by bits and std within 1 float ulp.

THE SHAPE TABLE (``TABLE``), one for the forward and the gradient tests.  Both launchers pick the small-LDS build <64, 64> by ``cells <= 64
&& width_max <= 64`` with width_max over both nets; the gradient walks 32 x 32 blocks of every layer with masked edges.

    a  13 x 5 = 65 cells, (64,) / (64,), 2 axes        cells one past the small build, widths at its limit; in_pad 68
    b  16 x 4 = 64 cells, (65,) / (7,), 4 axes         the actor alone one past; out_pad 96; the back pass writes k up to 68
    c  16 x 4 = 64 cells, (7,) / (65,), 3 axes         the critic alone one past: width_max is over both nets
    d  25 x 4 = 100 cells, (100, 96) / (127,), 5 axes  a ragged last k-block of four (4 live columns); three full j-blocks; 127 -> 128; odd A
    e  51 x 5 = 255 cells, (128,) / (1,), 7 axes       255 -> 256 cells; a hidden width of 1; A4 = 8 with A = 7
    f  33 x 2 = 66 cells, (31, 32, 33) / (3, 2, 1), 6 axes   three hidden layers on both sides of 32; narrow chains

A rule that read ``||``, looked at the actor alone, or was off by one would run rows a, b or c in the 64-row build and put xs[k][row] or
h[j][row] past its LDS arrays.  set_features takes every C and K above as it stands.  Features, controls and advantages mix float32 and
float64 (each at least twice per column); row c runs under storage="f32".

The host half of every input -- weights, batches, rows, optimiser states -- is built by the functions below from seeds alone, so
tests/test_policy_cpu.py and tests/test_ppo_cpu.py hold the statements to their own references at these shapes and assert the CONDITIONS
the tests here rest on (both branches of the clip taken, the norm between the two bounds, the dead units exact zeros, every setting moving
the gradient) without a GPU; the tests here assert them again on what they ran."""
import numpy as np
import pytest
import torch

from nuclear_sim_amd import policy, ppo
from test_policy_gpu import F32, F64, _env, _hold_sampling, _np, _same, _step, _weights
from test_policy_gpu import _statement as _policy_statement
from test_ppo_gpu import HYPER, _batch, _hold_relu, _hold_tanh, _statement, _stats, _to

pytestmark = pytest.mark.gpu

TABLE = {  # C, K, actor, critic, axes, features, controls, advantages, storage
    "a": (13, 5, (64,), (64,), 2, F32, F32, F64, "f64"),
    "b": (16, 4, (65,), (7,), 4, F64, F64, F32, "f64"),
    "c": (16, 4, (7,), (65,), 3, F32, F64, F32, "f32"),
    "d": (25, 4, (100, 96), (127,), 5, F64, F32, F64, "f64"),
    "e": (51, 5, (128,), (1,), 7, F32, F32, F32, "f64"),
    "f": (33, 2, (31, 32, 33), (3, 2, 1), 6, F64, F64, F64, "f64"),
}
ROWS = sorted(TABLE)
WEIGHT_SEED = {"a": 101, "b": 102, "c": 103, "d": 104, "e": 105, "f": 109}
BATCH_SEED = {"relu": 1000, "tanh": 3000}
GRADIENT_RUNS = [(70, 32), (97, 64)]      # count, rows_per_chain: three chains, the last of 6 rows; a full second tile and a short second chain
SETTINGS_ROW, SETTINGS_COUNT, SETTINGS_CHAIN = "b", 97, 64
SETTINGS = [{"clip": 0.05}, {"clip": 0.5}, {"vf_coef": 0.0}, {"vf_coef": 2.0}, {"ent_coef": 0.0}, {"ent_coef": 0.3}]
NORM_LOW, NORM_HIGH = 1e-3, 1e6
DEAD = {"actor": 64, "critic": 3}      # row b's hidden units with a bias of -50: the actor's is the one unit of its second 32-block
ADAM_STEPS = [0, 9, 10_000, 10_000_000]
ADAM_SETTINGS = [dict(betas=(0.5, 0.9)), dict(betas=(0.0, 0.999)), dict(eps=1e-8), dict(eps=1e-3), dict(lr=1e-2)]


# ---------------------------------------------------------------------------------------------------------------- the inputs, host only
def table_spec(row):
    C, K, actor, critic, A = TABLE[row][:5]
    return {"cells": C * K, "n_axes": A, "actor": actor, "critic": critic}


def table_weights(row, dead=False):
    """the row's nets; ``dead``: one first-layer unit of each net gets a bias of -50, which no row of a batch overcomes (a row's L1 norm
    is under 4 and the rows are standard normal)"""
    S = table_spec(row)
    a, c, log_std = _weights(WEIGHT_SEED[row], S["cells"], S["n_axes"], S["actor"], S["critic"])
    if dead:
        a[0][1][DEAD["actor"]], c[0][1][DEAD["critic"]] = -50.0, -50.0
    return a, c, log_std


def table_theta(row, dead=False):
    return policy.pack(*table_weights(row, dead))


def table_batch(row, count, theta, activation="relu"):
    fd, cd, ad = TABLE[row][5:8]
    return _batch(BATCH_SEED[activation] + count, theta, count, table_spec(row), activation, fd, cd, ad)


def table_rows(row, dtype, count=70):
    """explicit rows for policy_values"""
    return np.random.default_rng(7 + WEIGHT_SEED[row]).standard_normal((count, table_spec(row)["cells"])).astype(dtype)


def table_gradient(row, theta, batch, chain, activation="relu", ratio=None, **hyper):
    S = table_spec(row)
    return ppo.gradient(theta, S["cells"], S["n_axes"], S["actor"], S["critic"], activation, rows_per_chain=chain, ratio=ratio, **batch, **dict(HYPER, **hyper))


def critic_slice(row):
    S = table_spec(row)
    a, c = policy.sizes(S["cells"], S["n_axes"], S["actor"], S["critic"])
    first = sum(i * o + o for i, o in a)
    return slice(first, first + sum(i * o + o for i, o in c))


def dead_mask(row):
    """theta's entries whose gradient is exactly +0.0 with the DEAD units: the unit's row of dW and its db, and its column of the next dW"""
    S = table_spec(row)
    nets = []
    for which, dims in zip(("actor", "critic"), policy.sizes(S["cells"], S["n_axes"], S["actor"], S["critic"])):
        net = [(np.zeros((o, i), np.float32), np.zeros(o, np.float32)) for i, o in dims]
        u = DEAD[which]
        net[0][0][u, :], net[0][1][u], net[1][0][:, u] = 1.0, 1.0, 1.0
        nets.append(net)
    return policy.pack(nets[0], nets[1], np.zeros(S["n_axes"], np.float32), std=np.zeros(S["n_axes"], np.float32)) != 0


def adam_state(size, A, seed=5):
    """m and v over many magnitudes, v >= 0, with entries of exactly 0 (in both, and in one alone), float denormals and entries near 1e30;
    log_std's lanes stay moderate (std = exp(log_std') has to stay a finite float for its 1 ulp) and std's are 0: nothing moves them"""
    rng = np.random.default_rng(seed)
    m = (rng.standard_normal(size) * 10.0 ** rng.uniform(-12, 3, size)).astype(np.float32)
    v = ((rng.standard_normal(size) * 10.0 ** rng.uniform(-8, 2, size)) ** 2).astype(np.float32)
    at = rng.permutation(size - 2 * A)
    m[at[:8]], v[at[4:12]] = 0.0, 0.0
    m[at[12:16]], v[at[14:18]] = np.float32([1e-40, -3e-42, 1.4e-45, -1e-39]), np.float32([1e-40, 1.4e-45, 7e-43, 1e-39])
    m[at[18:22]], v[at[20:24]] = np.float32([1e30, -2e30, 5e29, -1e30]), np.float32([1e30, 3e30, 8e29, 1e30])
    m[-2 * A:-A], v[-2 * A:-A] = (1e-3 * rng.standard_normal(A)).astype(np.float32), (1e-6 * rng.uniform(1, 2, A)).astype(np.float32)
    m[-A:], v[-A:] = 0.0, 0.0
    assert (v >= 0).all() and np.isfinite(m).all() and np.isfinite(v).all()
    tiny = np.finfo(np.float32).tiny
    assert ((m != 0) & (np.abs(m) < tiny)).sum() >= 4 and ((v != 0) & (v < tiny)).sum() >= 4 and (np.abs(m) > 1e29).sum() >= 4 and (v > 1e29).sum() >= 4
    return m, v


# ---------------------------------------------------------------------------------------------------------------- the device's side
def _table_env(row, activation="relu", n=4, dead=False, **kw):
    C, K, actor, critic, A, fd, cd, ad, storage = TABLE[row]
    env = _env(n, C, K, fd, A, cd, storage)
    a, c, log_std = table_weights(row, dead)
    if "seed" not in kw:
        kw["deterministic"] = True
    env.set_policy(a, c, log_std, activation=activation, **kw)
    return env


def _device_batch(env, row, count, activation="relu"):
    """the row's batch around the DEVICE's theta (its std is the one torch formed)"""
    return table_batch(row, count, _np(env.policy_theta()), activation)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("n", [33, 70])
@pytest.mark.parametrize("row", ROWS)
def test_the_steps_launch_at_the_table_bit_for_bit(row, n):
    """controls_input(), value and logp of two deterministic steps are the statement's bits on one full tile and one row, and on two
    tiles and six rows"""
    env = _table_env(row, n=n)
    P = _policy_statement(env)
    for t in range(2):
        before = _np(env.features())
        obs, rew, done, info = _step(env, t)
        act, value, logp = P.step(before)
        assert np.isfinite(act).all() and np.isfinite(value).all() and np.isfinite(logp).all()
        _same(env.controls_input(), act, (t, "act")); _same(info["value"], value, (t, "value")); _same(info["logp"], logp, (t, "logp"))
    print("row %s: the actions' spread over the plants %.3e, the values' %.3e" % (row, np.ptp(act, axis=0).min(), np.ptp(value)))
    assert np.ptp(act, axis=0).min() > 0      # the plants differ: the actor does read its features
    env.close()


@pytest.mark.parametrize("row", ROWS)
def test_policy_values_of_explicit_rows_at_the_table(row):
    """70 rows (two tiles and six rows) once float32 and once float64, narrowed on the device: the critic's bits"""
    env = _table_env(row)
    P = _policy_statement(env)
    for dtype in (np.float32, np.float64):
        x = table_rows(row, dtype)
        want = P.values(x)
        assert np.isfinite(want).all() and np.ptp(want) > 0      # the rows differ: the critic does read them
        _same(env.policy_values(torch.as_tensor(x).to(env.device)), want, (row, dtype.__name__))
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("row, n, seed", [("a", 70, 7), ("d", 33, 2 ** 64 - 3), ("e", 70, 2 ** 32 + 1)])
def test_relu_sampling_at_2_5_and_7_axes(row, n, seed):
    """test_policy_gpu's sampling test (the same body, the same bounds) at the axes counts it leaves out: with 5 and 7 axes the
    Box-Muller pair of the last group is half used"""
    env = _table_env(row, n=n, seed=seed)
    assert env.policy_spec()["n_axes"] == {"a": 2, "d": 5, "e": 7}[row]
    _hold_sampling(env, seed)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("count, chain", GRADIENT_RUNS)
@pytest.mark.parametrize("row", ROWS)
def test_relu_gradient_at_the_table_bit_for_bit(row, count, chain):
    """test_ppo_gpu's relu contract, through its own body (_hold_relu): logp_new and value_new by bits, the ratio within 4 ulp, gradient
    and statistics by bits fed the device's ratio; finite, not zero, nothing skipped, the clip fraction strictly inside (0.02, 0.98)"""
    env = _table_env(row)
    _, want, ulps = _hold_relu(env, _device_batch(env, row, count), chain)
    print("row %s, %d rows in chains of %d: ratio %.1f ulp, clip fraction %.3f, norm %.3e" % (row, count, chain, ulps, want["stats"]["clip_fraction"],
                                                                                               want["stats"]["grad_norm"]))
    env.close()


def test_row_d_gives_the_same_bits_for_every_launch_geometry():
    env = _table_env("d")
    batch = _to(env, _device_batch(env, "d", 70))
    outs = [env.policy_grad(batch, rows_per_chain=32, max_blocks=b, diagnostics=True, **HYPER) for b in (1, 2, 0)]
    for o in outs[1:]:
        for k in ("grad", "stats", "ratio", "logp_new", "value_new"):
            _same(o[k], outs[0][k], k)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_tanh_gradient_of_row_d_within_8_times_the_statements_distance_from_float64():
    """test_ppo_gpu's tanh contract through its own body (_hold_tanh), max_grad_norm 0.  Measured on an MI355X: in DESIGN.md"""
    env = _table_env("d", activation="tanh")
    mine, yard = _hold_tanh(env, _device_batch(env, "d", 97, "tanh"), 64)
    print("row d, tanh, 97 rows: the device %.3e, the statement %.3e, factor %.3f" % (mine, yard, mine / yard))
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.fixture(scope="module")
def settings():
    """row b's env, its batch of 97 rows and the default run, shared by the tests of the settings and left unchanged by them"""
    env = _table_env(SETTINGS_ROW)
    batch = _device_batch(env, SETTINGS_ROW, SETTINGS_COUNT)
    default = _np(env.policy_grad(_to(env, batch), rows_per_chain=SETTINGS_CHAIN, **HYPER)["grad"])
    yield env, batch, default
    env.close()


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "%s=%s" % next(iter(s.items())))
def test_a_loss_coefficient_other_than_the_default(settings, setting):
    """by bits against the statement run with the same setting, and the setting does enter: the gradient is not the default's"""
    env, batch, default = settings
    got, want, _ = _hold_relu(env, batch, SETTINGS_CHAIN, **setting)
    assert not np.array_equal(_np(got["grad"]), default)
    A = env.policy_spec()["n_axes"]
    if "vf_coef" in setting and setting["vf_coef"] == 0.0:
        critic = _np(got["grad"])[critic_slice(SETTINGS_ROW)]
        assert critic.size == 64 * 7 + 7 + 7 + 1 and not critic.view(np.int32).any()      # every entry of the critic is +0.0
    if "ent_coef" in setting:      # it enters through log_std's lanes alone: with the norm clip off every other entry keeps its bits
        off = dict(HYPER, max_grad_norm=0.0)
        one = _np(env.policy_grad(_to(env, batch), rows_per_chain=SETTINGS_CHAIN, **off)["grad"])
        two = _np(env.policy_grad(_to(env, batch), rows_per_chain=SETTINGS_CHAIN, **dict(off, **setting))["grad"])
        others = np.ones(one.size, bool)
        others[-2 * A:-A] = False
        _same(two[others], one[others], "every entry but log_std's")
        assert (two[-2 * A:-A] != one[-2 * A:-A]).all()


def test_both_branches_of_the_norm_clip(settings):
    env, batch, _ = settings
    A = env.policy_spec()["n_axes"]
    low, want_low, _ = _hold_relu(env, batch, SETTINGS_CHAIN, max_grad_norm=NORM_LOW)
    high, want_high, _ = _hold_relu(env, batch, SETTINGS_CHAIN, max_grad_norm=NORM_HIGH)
    off, want_off, _ = _hold_relu(env, batch, SETTINGS_CHAIN, max_grad_norm=0.0)
    norm = want_off["stats"]["grad_norm"]
    assert want_low["stats"]["grad_norm"] == norm == want_high["stats"]["grad_norm"]      # (the reported norm is the unclipped one)
    assert NORM_LOW < norm < NORM_HIGH      # the first bound scales, the second does not
    # a scale of 1.0 in double and the narrowing are the identity
    _same(high["grad"], off["grad"], "max_grad_norm above the norm")
    # the scaled gradient's own norm: every entry is the exact product rounded once, so the vector stands within the norm of the
    # entries' half spacings from the exact one, whose norm is NORM_LOW * norm / (norm + 1e-6) (to the double evaluation's 1e-12)
    g = _np(low["grad"])[:-A].astype(np.float64)
    target = NORM_LOW * norm / (norm + 1e-6)
    bound = np.sqrt(((0.5 * np.spacing(np.abs(want_low["grad"][:-A])).astype(np.float64)) ** 2).sum()) + 1e-12 * target
    own = np.sqrt((g * g).sum())
    print("the clipped gradient's norm %.9e, the target %.9e, apart %.3e, bound %.3e" % (own, target, abs(own - target), bound))
    assert abs(own - target) <= bound and bound < 1e-7 * target
    assert not np.array_equal(_np(low["grad"]), _np(off["grad"]))


def test_poisoned_rows_at_the_tile_seams(settings):
    """test_poisoned_rows_are_skipped_and_counted's assertions with the rows at the ends of the first chain's tiles and the batch's last"""
    env, batch, default = settings
    chain = SETTINGS_CHAIN
    clean = env.policy_grad(_to(env, batch), rows_per_chain=chain, diagnostics=True, **HYPER)
    value = _np(clean["value_new"])
    dirty = {k: v.copy() for k, v in batch.items()}
    dirty["obs"][31, 63], dirty["act"][32, 3], dirty["logp_old"][63], dirty["adv"][96], dirty["ret"][96] = np.nan, np.inf, np.nan, -np.inf, np.nan
    bad = [31, 32, 63, 96]
    got = env.policy_grad(_to(env, dirty), rows_per_chain=chain, diagnostics=True, **HYPER)
    stats = _np(got["stats"])
    assert stats[ppo.STATS.index("skipped")] == 4 and stats[ppo.STATS.index("count")] == 97
    assert np.isfinite(_np(got["grad"])).all() and np.isfinite(stats).all()
    for k in ("ratio", "logp_new", "value_new"):
        x = _np(got[k])
        assert np.isnan(x[bad]).all() and np.isfinite(np.delete(x, bad)).all(), k
    want = _statement(env, dirty, chain, ratio=_np(got["ratio"]))
    _same(got["grad"], want["grad"], "grad"); _same(got["stats"], _stats(want), "stats")
    zeroed = {k: v.copy() for k, v in batch.items()}
    zeroed["adv"][bad], zeroed["ret"][bad] = 0.0, value[bad].astype(zeroed["ret"].dtype)
    same = env.policy_grad(_to(env, zeroed), rows_per_chain=chain, **HYPER)
    _same(got["grad"], same["grad"], "the gradient with the seeds zeroed")
    assert not np.array_equal(_np(got["grad"]), _np(clean["grad"]))
    _same(clean["grad"], default, "the batch itself was left as it was")


# ---------------------------------------------------------------------------------------------------------------- 6
def _adam(env, theta, m, v, step, grad, **kw):
    """one policy_adam against ppo.adam fed the device's gradient and the device's std: m, v and theta by bits, std within 1 float ulp,
    and the step count one further"""
    A = env.policy_spec()["n_axes"]
    env.policy_adam(**kw)
    now = _np(env.policy_theta())
    std_want = np.exp(now[-2 * A:-A].astype(np.float64)).astype(np.float32)
    assert np.isfinite(std_want).all() and (np.abs(now[-A:] - std_want) <= np.spacing(std_want)).all()
    theta, m, v, step = ppo.adam(theta, m, v, step, grad, A, std=now[-A:], **kw)
    state = env.policy_optimizer_state()
    assert state["step"] == step
    _same(now, theta, "theta behind Adam"); _same(state["m"], m, "m"); _same(state["v"], v, "v")
    return theta, m, v, step


@pytest.fixture(scope="module")
def trained():
    """row b's env with a gradient formed: (env, theta0, the gradient, the batch)"""
    env = _table_env(SETTINGS_ROW)
    batch = _device_batch(env, SETTINGS_ROW, SETTINGS_COUNT)
    theta0 = _np(env.policy_theta())
    grad = _np(env.policy_grad(_to(env, batch), rows_per_chain=SETTINGS_CHAIN, **HYPER)["grad"])
    yield env, theta0, grad, batch
    env.close()


@pytest.mark.parametrize("step", ADAM_STEPS)
def test_adam_from_a_loaded_state(trained, step):
    """load_policy_optimizer_state followed by an update: step_size and root are formed on the host from the LOADED count.  At 10 000 000
    b2^step has underflowed and root is exactly 1"""
    env, theta0, grad, _ = trained
    A = env.policy_spec()["n_axes"]
    m, v = adam_state(theta0.size, A)
    if step == 10_000_000:
        assert 0.999 ** (step + 1) == 0.0 and np.sqrt(1.0 - 0.999 ** (step + 1)) == 1.0
    env.policy_load(theta0)
    env.load_policy_optimizer_state({"m": m, "v": v, "step": step})
    theta, m1, v1, now = _adam(env, theta0, m, v, step, grad)
    assert now == step + 1 and not np.array_equal(theta[:-2 * A], theta0[:-2 * A]) and not np.array_equal(m1, m) and not np.array_equal(v1, v)


@pytest.mark.parametrize("kw", ADAM_SETTINGS, ids=lambda kw: "%s=%s" % next(iter(kw.items())))
def test_adam_with_other_settings(trained, kw):
    """from the loaded state at step 9 (m and v not zero: b1 = 0 has something to drop)"""
    env, theta0, grad, _ = trained
    m, v = adam_state(theta0.size, env.policy_spec()["n_axes"])
    env.policy_load(theta0)
    env.load_policy_optimizer_state({"m": m, "v": v, "step": 9})
    default = ppo.adam(theta0, m, v, 9, grad, env.policy_spec()["n_axes"])[0]
    theta, _, _, _ = _adam(env, theta0, m, v, 9, grad, **kw)
    assert not np.array_equal(theta, default)      # the setting does enter


def test_three_updates_in_a_row_on_one_batch(trained):
    env, theta0, _, batch = trained
    A = env.policy_spec()["n_axes"]
    env.policy_load(theta0)
    env.load_policy_optimizer_state({"m": np.zeros_like(theta0), "v": np.zeros_like(theta0), "step": 0})
    theta, m, v, step = theta0, np.zeros_like(theta0), np.zeros_like(theta0), 0
    for k in range(3):
        got = env.policy_grad(_to(env, batch), rows_per_chain=SETTINGS_CHAIN, diagnostics=True, **HYPER)
        want = table_gradient(SETTINGS_ROW, theta, batch, SETTINGS_CHAIN, ratio=_np(got["ratio"]))
        _same(got["grad"], want["grad"], (k, "the gradient at the statement's theta"))
        theta, m, v, step = _adam(env, theta, m, v, step, _np(got["grad"]), lr=1e-3)
    assert step == 3 and env.policy_optimizer_state()["step"] == 3 and not np.array_equal(theta[:-2 * A], theta0[:-2 * A])


def test_a_gradient_with_exact_zeros_leaves_m_v_and_theta_as_they_were():
    """one hidden unit of each net is dead on every row (a bias of -50): its row of dW, its db and its column of the next dW are +0.0 in
    the statement, and from a zero state Adam keeps m and v +0.0 there and theta's bits"""
    env = _table_env(SETTINGS_ROW, dead=True)
    A = env.policy_spec()["n_axes"]
    theta0 = _np(env.policy_theta())
    batch = _device_batch(env, SETTINGS_ROW, SETTINGS_COUNT)
    mask = dead_mask(SETTINGS_ROW)
    own = table_gradient(SETTINGS_ROW, theta0, batch, SETTINGS_CHAIN)
    assert mask.sum() == (64 + 1 + 4) + (64 + 1 + 1) and not own["grad"].view(np.int32)[mask].any()      # on the statement alone, first
    got, want, _ = _hold_relu(env, batch, SETTINGS_CHAIN)
    grad = _np(got["grad"])
    assert not grad.view(np.int32)[mask].any() and (grad[:-A][~mask[:-A]] != 0).mean() > 0.9
    zero = np.zeros_like(theta0)
    theta, m, v, _ = _adam(env, theta0, zero, zero, 0, grad)
    assert not m.view(np.int32)[mask].any() and not v.view(np.int32)[mask].any()
    _same(theta[mask], theta0[mask], "theta where the gradient is +0.0")
    assert (theta[:-2 * A][~mask[:-2 * A]] != theta0[:-2 * A][~mask[:-2 * A]]).mean() > 0.9
    env.close()
