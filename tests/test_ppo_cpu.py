"""CPU: the statement of the policy's training step (nuclear_sim_amd/ppo.py) -- the PPO loss, its gradient with the sums over rows pinned,
the clipping and Adam -- against float64 torch autograd of the same loss, against float64 torch.optim.Adam, and on hand-built rows.

The gradient's yardstick is float32 torch autograd's own distance from the float64 evaluation, pooled: the maximum over all parameter
tensors of max|g - g64| / max|g64|.  The statement, a float32 evaluation in another order, may be at most 4 times as far; a wrong index
errs by order 1.  Measured here (statement / float32 autograd): relu 70 rows 3.6e-7 / 3.4e-7 = 1.05; tanh 300 rows 4.7e-7 / 5.4e-7 =
0.87; relu 257 rows of 64 cells 1.05e-6 / 1.43e-6 = 0.74.

Adam: the statement narrows theta, m and v once per step, so k steps in it may stand k * (2^-24 |theta| + 2^-22 lr) from the float64
optimiser fed the same gradients: half an ulp of theta for its own narrowing, and the rest for m and v, whose relative 2^-24 moves a step of
about lr by far less than 2^-22 lr."""
import numpy as np
import pytest
import torch

from nuclear_sim_amd import policy, ppo

CASES = [  # rows, cells, actor = critic hidden, axes, activation, rows_per_chain, seed
    (70, 15, (33, 17), 3, "relu", 32, 1),
    (300, 15, (33, 17), 3, "tanh", 64, 0),
    (257, 64, (64, 64), 8, "relu", 256, 0),
]
CLIP, VF, ENT = 0.2, 0.5, 0.01


def make_theta(rng, cells, axes, actor, critic):
    nets = []
    for dims in policy.sizes(cells, axes, actor, critic):
        nets.append([((rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32), (0.1 * rng.standard_normal(o)).astype(np.float32)) for i, o in dims])
    return policy.pack(nets[0], nets[1], (-0.5 + 0.2 * rng.standard_normal(axes)).astype(np.float32))


def make_batch(rng, theta, n, cells, axes, actor, critic, activation, wobble=0.15):
    """rows whose actions and logp_old come from a perturbed policy, so the ratios scatter around 1 and some are clipped"""
    old = theta.copy()
    old[:-2 * axes] += (wobble * rng.standard_normal(old.size - 2 * axes) * np.abs(old[:-2 * axes])).astype(np.float32)
    a_net, c_net, log_std, std = policy.unpack(old, cells, axes, actor, critic)
    obs = rng.standard_normal((n, cells)).astype(np.float32)
    z = rng.standard_normal((n, axes))
    act, _, logp = policy.outputs(policy.forward(a_net, obs, activation), np.zeros(n, np.float32), log_std, std, z, obs)
    adv = rng.standard_normal(n).astype(np.float32)
    ret = rng.standard_normal(n).astype(np.float32)
    return {"obs": obs, "act": act, "logp_old": logp, "adv": adv, "ret": ret}


def autograd(theta, cells, axes, actor, critic, activation, batch, dtype):
    """the gradient of the same loss by torch autograd in ``dtype``, per tensor in theta's order (std's apart), and the ratios"""
    a_net, c_net, log_std, _ = policy.unpack(theta, cells, axes, actor, critic)
    leaves = []

    def leaf(x):
        t = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
        leaves.append(t)
        return t
    nets = [[(leaf(W), leaf(b)) for W, b in net] for net in (a_net, c_net)]
    ls = leaf(log_std)
    f = torch.relu if activation == "relu" else torch.tanh
    t = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in batch.items()}

    def run(net):
        h = t["obs"]
        for W, b in net[:-1]:
            h = f(h @ W.T + b)
        return h @ net[-1][0].T + net[-1][1]
    mean, v = run(nets[0]), run(nets[1])[:, 0]
    d = (t["act"] - mean) / torch.exp(ls)
    lp = (-0.5 * d * d - ls - policy.HALF_LOG_2PI).sum(dim=1)
    r = torch.exp(lp - t["logp_old"])
    ploss = -torch.minimum(r * t["adv"], torch.clamp(r, 1 - CLIP, 1 + CLIP) * t["adv"])
    loss = ploss.mean() + VF * (0.5 * (v - t["ret"]) ** 2).mean() - ENT * (ls + 0.5 + policy.HALF_LOG_2PI).sum()
    loss.backward()
    return [x.grad.numpy().astype(np.float64) for x in leaves], r.detach().numpy().astype(np.float64)


def split(grad, cells, axes, actor, critic):
    a, c, ls, _ = policy.unpack(grad, cells, axes, actor, critic)
    return [x.astype(np.float64) for net in (a, c) for W, b in net for x in (W, b)] + [ls.astype(np.float64)]


def pooled(gs, ref):
    return max(np.abs(g - r).max() / np.abs(r).max() for g, r in zip(gs, ref))


@pytest.mark.parametrize("n, cells, hidden, axes, activation, chain, seed", CASES, ids=["relu-70", "tanh-300", "relu-257"])
def test_the_gradient_stands_as_close_to_float64_autograd_as_float32_autograd_does(n, cells, hidden, axes, activation, chain, seed):
    rng = np.random.default_rng(seed)
    theta = make_theta(rng, cells, axes, hidden, hidden)
    batch = make_batch(rng, theta, n, cells, axes, hidden, hidden, activation)
    g64, r = autograd(theta, cells, axes, hidden, hidden, activation, batch, torch.float64)
    near = min(np.abs(r - (1 + CLIP)).min(), np.abs(r - (1 - CLIP)).min())
    print("nearest ratio to a clip boundary: %.2e" % near)
    assert near > 1e-4      # (no row may flip between the evaluations)
    g32, _ = autograd(theta, cells, axes, hidden, hidden, activation, batch, torch.float32)
    out = ppo.gradient(theta, cells, axes, hidden, hidden, activation, clip=CLIP, vf_coef=VF, ent_coef=ENT, max_grad_norm=0.0, rows_per_chain=chain, **batch)
    assert 0.05 <= out["stats"]["clip_fraction"] <= 0.95
    assert out["stats"]["skipped"] == 0 and out["stats"]["count"] == n
    mine, yard = pooled(split(out["grad"], cells, axes, hidden, hidden), g64), pooled(g32, g64)
    print("pooled distance from float64: the statement %.3e, float32 autograd %.3e, ratio %.2f" % (mine, yard, mine / yard))
    assert mine <= 4 * yard
    assert not out["grad"][-axes:].any()      # std is derived: no gradient
    # the statistics are those of the float64 evaluation
    assert abs(out["stats"]["approx_kl"] - ((r - 1) - np.log(r)).mean()) < 1e-6
    assert abs(out["stats"]["grad_norm"] - np.sqrt(sum((g ** 2).sum() for g in g64))) < 1e-5 * out["stats"]["grad_norm"]


def _rows(r, adv, **change):
    """the epilogue of rows fed the ratio r: one axis, mean 0, std 1, the action 0.5"""
    n = len(adv)
    kw = {"mean": np.zeros((n, 1), np.float32), "v": np.full(n, 0.25, np.float32), "log_std": [0.0], "std": [1.0], "act": np.full((n, 1), 0.5, np.float32),
          "logp_old": np.zeros(n, np.float32), "adv": np.asarray(adv, np.float64), "ret": np.zeros(n), "bad": np.zeros(n, bool)}
    kw.update(change)
    return ppo.rows(clip=CLIP, vf_coef=VF, ratio=np.asarray(r, np.float64), **kw)


def test_a_ratio_exactly_on_the_boundary_is_not_clipped_and_one_past_it_is():
    hi, lo = 1.0 + CLIP, 1.0 - CLIP
    R = _rows([hi, hi, hi, np.nextafter(hi, 2), lo, np.nextafter(lo, 0), lo], [2.0, -2.0, 0.0, 2.0, -2.0, -2.0, 2.0])
    assert R["clipped"].tolist() == [0, 0, 0, 1, 0, 1, 0]
    # c = -(adv * r), the seed ((c * d) / std) / count with d = 0.5
    assert R["dmean"][0, 0] == np.float32(((-(2.0 * hi) * 0.5) / 1.0) / 7.0) and R["dmean"][1, 0] == np.float32((((2.0 * hi) * 0.5) / 1.0) / 7.0)
    assert R["dmean"][2, 0] == 0 and R["dls"][2, 0] == 0 and R["dmean"][3, 0] == 0 and R["dls"][3, 0] == 0 and R["dmean"][5, 0] == 0
    assert R["dls"][0, 0] == (-(2.0 * hi) * (0.25 - 1.0)) / 7.0
    # the loss of a clipped row is the clamped branch's
    assert R["policy_loss"][3] == -(hi * 2.0) and R["policy_loss"][5] == -(lo * -2.0) and R["policy_loss"][0] == -(hi * 2.0)
    assert R["dv"][0] == np.float32((VF * 0.25) / 7.0) and R["value_loss"][0] == 0.5 * 0.0625


@pytest.mark.parametrize("what", ["obs", "act", "logp_old", "adv", "ret"])
@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_a_row_with_an_input_that_is_not_finite_is_skipped_and_counted(what, poison):
    rng = np.random.default_rng(5)
    cells, axes, hidden = 6, 2, (5,)
    theta = make_theta(rng, cells, axes, hidden, hidden)
    batch = make_batch(rng, theta, 40, cells, axes, hidden, hidden, "relu")
    clean = ppo.gradient(theta, cells, axes, hidden, hidden, "relu", rows_per_chain=32, **batch)
    dirty = {k: v.copy() for k, v in batch.items()}
    dirty[what][(7, 1) if dirty[what].ndim == 2 else 7] = poison
    out = ppo.gradient(theta, cells, axes, hidden, hidden, "relu", rows_per_chain=32, **dirty)
    assert out["stats"]["skipped"] == 1 and out["stats"]["count"] == 40 and np.isfinite(out["grad"]).all()
    assert all(np.isfinite(v) for v in out["stats"].values())
    assert np.isnan(out["ratio"][7]) and np.isnan(out["logp_new"][7]) and np.isnan(out["value_new"][7]) and np.isfinite(np.delete(out["ratio"], 7)).all()
    assert not np.array_equal(out["grad"], clean["grad"])
    # it is the gradient of the batch with that row's seeds zeroed: a row whose advantage is 0 and whose return is its value, the divisor kept
    zeroed = {k: v.copy() for k, v in batch.items()}
    zeroed["adv"][7], zeroed["ret"][7] = 0.0, clean["value_new"][7]
    same = ppo.gradient(theta, cells, axes, hidden, hidden, "relu", rows_per_chain=32, **zeroed)
    assert np.array_equal(same["grad"], out["grad"])


def test_adam_follows_float64_torch_adam():
    rng = np.random.default_rng(11)
    axes, size = 3, 500
    theta = rng.standard_normal(size).astype(np.float32)
    theta[-axes:] = np.exp(theta[-2 * axes:-axes])
    lr, betas, eps = 3e-4, (0.9, 0.999), 1e-5
    ref = torch.tensor(theta[:-axes].astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([ref], lr=lr, betas=betas, eps=eps)
    m, v, step = np.zeros(size, np.float32), np.zeros(size, np.float32), 0
    for k in range(1, 4):
        g = (rng.standard_normal(size) * 10.0 ** rng.uniform(-4, 1, size)).astype(np.float32)
        ref.grad = torch.tensor(g[:-axes].astype(np.float64))
        opt.step()
        theta, m, v, step = ppo.adam(theta, m, v, step, g, axes, lr, betas, eps)
        assert step == k
        want = ref.detach().numpy()
        err = np.abs(theta[:-axes].astype(np.float64) - want)
        bound = k * (2.0 ** -24 * np.abs(want) + 2.0 ** -22 * lr)
        print("step %d: the largest error over its bound %.3f" % (k, (err / bound).max()))
        assert (err <= bound).all()
        assert np.array_equal(theta[-axes:], np.exp(theta[-2 * axes:-axes].astype(np.float64)).astype(np.float32))
        assert not m[-axes:].any() and not v[-axes:].any()


def test_up_to_32_rows_every_chain_length_gives_the_same_bits():
    rng = np.random.default_rng(7)
    cells, axes, hidden = 9, 2, (6, 5)
    theta = make_theta(rng, cells, axes, hidden, hidden)
    for n in (1, 31, 32):
        batch = make_batch(rng, theta, n, cells, axes, hidden, hidden, "tanh")
        outs = [ppo.gradient(theta, cells, axes, hidden, hidden, "tanh", rows_per_chain=c, **batch) for c in (32, 64, 256)]
        for o in outs[1:]:
            assert np.array_equal(o["grad"], outs[0]["grad"]) and o["stats"] == outs[0]["stats"]
    # and beyond 32 rows the chains are the statement's: 70 rows in chains of 32 and of 64 differ in some bit
    batch = make_batch(rng, theta, 70, cells, axes, hidden, hidden, "tanh")
    a, b = (ppo.gradient(theta, cells, axes, hidden, hidden, "tanh", rows_per_chain=c, **batch)["grad"] for c in (32, 64))
    assert not np.array_equal(a, b) and np.allclose(a, b, rtol=1e-4, atol=1e-7)


def test_the_clipping_scales_by_the_pinned_norm_and_refusals_are_named():
    g = np.arange(1, 601, dtype=np.float32)
    out, norm = ppo.clip_grad(g, 2, 0.5)
    wide = g[:-2].astype(np.float64)
    assert abs(norm - np.sqrt((wide * wide).sum())) < 1e-9 * norm
    assert np.array_equal(out[:-2], (wide * (0.5 / (norm + 1e-6))).astype(np.float32)) and np.array_equal(out[-2:], g[-2:])
    assert np.array_equal(ppo.clip_grad(g, 2, 0.0)[0], g) and np.array_equal(ppo.clip_grad(g, 2, 1e9)[0], g)
    for kw, words in (({"count": 0}, "count"), ({"rows_per_chain": 48}, "multiple of 32"), ({"rows_per_chain": 0}, "multiple of 32"),
                      ({"clip": 0.0}, "(0, 1)"), ({"clip": 1.0}, "(0, 1)"), ({"clip": float("nan")}, "(0, 1)")):
        args = {"count": 5, "rows_per_chain": 256, "clip": 0.2}
        args.update(kw)
        with pytest.raises(ValueError, match=words.replace("(", r"\(").replace(")", r"\)")):
            ppo.check(**args)


# ---------------------------------------------------------------------------------------------------------------- the shape table
# tests/test_policy_shapes_gpu.py holds the device to this statement at ragged shapes and other settings.  The statement has to be right
# there first, and the inputs of those tests have to be what the tests take them for: both are checked here, without a GPU.
def _table():
    import test_policy_shapes_gpu as T      # (not at the top: that module imports this one)
    return T


@pytest.mark.parametrize("activation", ["relu", "tanh"])
@pytest.mark.parametrize("row", ["a", "d", "e", "f"])
def test_the_gradient_at_the_shape_tables_rows_against_float64_autograd(row, activation):
    """70 rows in chains of 32, the actor and the critic of different shapes, 2 / 5 / 7 / 6 axes: the same yardstick and the same factor
    of 4 as the first test of this file"""
    T = _table()
    S = T.table_spec(row)
    shape = (S["cells"], S["n_axes"], S["actor"], S["critic"])
    rng = np.random.default_rng({"a": 2, "d": 1, "e": 1, "f": 1}[row])
    theta = make_theta(rng, *shape)
    batch = make_batch(rng, theta, 70, *shape, activation)
    g64, r = autograd(theta, *shape, activation, batch, torch.float64)
    near = min(np.abs(r - (1 + CLIP)).min(), np.abs(r - (1 - CLIP)).min())
    assert near > 1e-4, near
    assert all(np.abs(g).max() > 0 for g in g64)      # (every tensor has a scale to be measured against)
    g32, _ = autograd(theta, *shape, activation, batch, torch.float32)
    out = ppo.gradient(theta, *shape, activation, clip=CLIP, vf_coef=VF, ent_coef=ENT, max_grad_norm=0.0, rows_per_chain=32, **batch)
    assert 0.05 <= out["stats"]["clip_fraction"] <= 0.95 and out["stats"]["skipped"] == 0 and out["stats"]["count"] == 70
    mine, yard = pooled(split(out["grad"], *shape), g64), pooled(g32, g64)
    print("row %s %s: the statement %.3e, float32 autograd %.3e, ratio %.2f" % (row, activation, mine, yard, mine / yard))
    assert mine <= 4 * yard
    assert abs(out["stats"]["grad_norm"] - np.sqrt(sum((g ** 2).sum() for g in g64))) < 1e-5 * out["stats"]["grad_norm"]


@pytest.mark.parametrize("row", ["a", "b", "c", "d", "e", "f"])
def test_the_shape_tables_batches_take_both_branches_of_the_loss_clip(row):
    """a condition on the inputs of the GPU tests, not a measurement: every batch they run has a clip fraction strictly inside (0.02,
    0.98), skips nothing and has a gradient that is finite and not zero"""
    T = _table()
    theta = T.table_theta(row)
    A = T.table_spec(row)["n_axes"]
    for count, chain in T.GRADIENT_RUNS:
        out = T.table_gradient(row, theta, T.table_batch(row, count, theta), chain)
        assert 0.02 < out["stats"]["clip_fraction"] < 0.98, (count, out["stats"]["clip_fraction"])
        assert out["stats"]["skipped"] == 0 and np.isfinite(out["grad"]).all() and out["grad"][:-A].any()


def test_the_tanh_batch_of_row_d_has_no_ratio_on_a_clip_boundary():
    T = _table()
    S = T.table_spec("d")
    theta = T.table_theta("d")
    batch = T.table_batch("d", 97, theta, "tanh")
    _, r = autograd(theta, S["cells"], S["n_axes"], S["actor"], S["critic"], "tanh", batch, torch.float64)
    assert min(np.abs(r - (1 + CLIP)).min(), np.abs(r - (1 - CLIP)).min()) > 1e-3      # (ten times what the GPU test needs: its std is the device's)
    out = T.table_gradient("d", theta, batch, 64, "tanh", max_grad_norm=0.0)
    assert 0.02 < out["stats"]["clip_fraction"] < 0.98


def test_every_setting_of_the_settings_tests_moves_the_statements_gradient():
    """the batch of 97 rows on row b: each loss coefficient changes the gradient (and keeps both clip branches taken), ent_coef changes
    log_std's entries alone, vf_coef = 0 makes the critic's entries +0.0, and the unclipped norm lies strictly between the two bounds of
    the norm-clip test, of which the first then scales and the second does not"""
    T = _table()
    row, count, chain = T.SETTINGS_ROW, T.SETTINGS_COUNT, T.SETTINGS_CHAIN
    A = T.table_spec(row)["n_axes"]
    theta = T.table_theta(row)
    batch = T.table_batch(row, count, theta)
    default = T.table_gradient(row, theta, batch, chain)
    for setting in T.SETTINGS:
        out = T.table_gradient(row, theta, batch, chain, **setting)
        assert not np.array_equal(out["grad"], default["grad"]), setting
        assert 0.02 < out["stats"]["clip_fraction"] < 0.98, (setting, out["stats"]["clip_fraction"])
        if setting.get("vf_coef") == 0.0:
            assert not out["grad"][T.critic_slice(row)].view(np.int32).any()
        if "ent_coef" in setting:
            one, two = (T.table_gradient(row, theta, batch, chain, max_grad_norm=0.0, **kw)["grad"] for kw in ({}, setting))
            assert np.array_equal(np.delete(one, np.s_[-2 * A:-A]).view(np.int32), np.delete(two, np.s_[-2 * A:-A]).view(np.int32))
            assert (one[-2 * A:-A] != two[-2 * A:-A]).all()
    norm = default["stats"]["grad_norm"]
    assert T.NORM_LOW < norm < T.NORM_HIGH
    low, high, off = (T.table_gradient(row, theta, batch, chain, max_grad_norm=x) for x in (T.NORM_LOW, T.NORM_HIGH, 0.0))
    assert np.array_equal(high["grad"].view(np.int32), off["grad"].view(np.int32)) and not np.array_equal(low["grad"], off["grad"])
    # a bad row at each tile seam is skipped in the statement too, and the rest of the batch goes on
    dirty = {k: v.copy() for k, v in batch.items()}
    dirty["obs"][31, 63], dirty["act"][32, 3], dirty["logp_old"][63], dirty["adv"][96], dirty["ret"][96] = np.nan, np.inf, np.nan, -np.inf, np.nan
    out = T.table_gradient(row, theta, dirty, chain)
    assert out["stats"]["skipped"] == 4 and np.flatnonzero(np.isnan(out["ratio"])).tolist() == [31, 32, 63, 96] and np.isfinite(out["grad"]).all()


def test_the_dead_units_give_exact_zeros_and_adam_leaves_them():
    T = _table()
    row = T.SETTINGS_ROW
    A = T.table_spec(row)["n_axes"]
    theta = T.table_theta(row, dead=True)
    mask = T.dead_mask(row)
    out = T.table_gradient(row, theta, T.table_batch(row, T.SETTINGS_COUNT, theta), T.SETTINGS_CHAIN)
    assert mask.sum() == (64 + 1 + 4) + (64 + 1 + 1) and not out["grad"].view(np.int32)[mask].any()
    assert (out["grad"][:-A][~mask[:-A]] != 0).mean() > 0.9      # (and the rest of the gradient is there)
    new, m, v, step = ppo.adam(theta, np.zeros_like(theta), np.zeros_like(theta), 0, out["grad"], A)
    assert step == 1 and not m.view(np.int32)[mask].any() and not v.view(np.int32)[mask].any()
    assert np.array_equal(new.view(np.int32)[mask], theta.view(np.int32)[mask])
    assert (new[:-2 * A][~mask[:-2 * A]] != theta[:-2 * A][~mask[:-2 * A]]).mean() > 0.9


def test_adam_at_large_loaded_steps_and_other_settings():
    """the host's step_size and root at the loaded steps of the GPU test: finite, root exactly 1 once b2^step has underflowed; and the
    loaded state (zeros, float denormals, entries near 1e30) goes through one update finite, under every setting the GPU test runs"""
    T = _table()
    rng = np.random.default_rng(2)
    A, size = 4, 400
    theta = rng.standard_normal(size).astype(np.float32)
    g = (rng.standard_normal(size) * 10.0 ** rng.uniform(-4, 0, size)).astype(np.float32)
    m, v = T.adam_state(size, A)
    assert 0.999 ** 10_000_001 == 0.0 and np.sqrt(1.0 - 0.999 ** 10_000_001) == 1.0 and 0.0 < 0.999 ** 10_001 < 1e-4
    default = ppo.adam(theta, m, v, 9, g, A)[0]
    for step in T.ADAM_STEPS:
        new, m1, v1, now = ppo.adam(theta, m, v, step, g, A)
        assert now == step + 1 and np.isfinite(new).all() and np.isfinite(m1).all() and np.isfinite(v1).all() and (v1 >= 0).all()
        assert not m1[-A:].any() and not v1[-A:].any()
    for kw in T.ADAM_SETTINGS:
        new = ppo.adam(theta, m, v, 9, g, A, **kw)[0]
        assert np.isfinite(new).all() and not np.array_equal(new, default), kw
