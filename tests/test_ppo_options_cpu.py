"""CPU: the options of the policy's training step as nuclear_sim_amd/ppo.py states them -- value-loss clipping, explained_variance and the
target_kl gate.  Left at their defaults the statement returns the bits it returns without them; with ``clip_vf`` its gradient is compared
with float64 torch autograd of the max-form loss by the yardstick of tests/test_ppo_cpu.py (float32 autograd's own pooled distance, at
most 4 times as far); explained_variance is compared with numpy's variances; the gate on hand-built numbers.

THE VALUE-CLIP INPUTS (``vf_inputs``) are built from the statement's own forward ``v`` so that every branch of the clipped epilogue is
taken, far from its boundaries.  Row i is of class i % 5, with c = clip_vf and u, w uniform in [0.8, 1.2]:
    0 below, not used:  value_old = v + 2 c u (dvo = -2 c u < -c);  ret = v + w      (sqc = (c - w)^2 < sq = w^2)
    1 inside:           value_old = v +- 0.5 c u;                    ret = v +- w
    2 below, used:      value_old = v + 2 c u;                       ret = v - w      (sqc = (c + w)^2 > sq)
    3 above, used:      value_old = v - 2 c u;                       ret = v + w
    4 above, not used:  value_old = v - 2 c u;                       ret = v - w
so |dvo| is at least 0.4 c from c, and with c = 0.2 sqc / sq is at most (1 - 0.2 / 1.2)^2 = 0.69 or at least (1 + 0.2 / 1.2)^2 = 1.36."""
import numpy as np
import pytest
import torch

from nuclear_sim_amd import policy, ppo
from test_ppo_cpu import CASES, CLIP, ENT, VF, make_batch, make_theta, pooled, split

CLIP_VF = 0.2
CLASSES = ("below", "inside", "below_use", "above_use", "above")


def forward_value(theta, cells, axes, actor, critic, activation, obs):
    """the statement's own v of the rows"""
    nets = policy.unpack(theta, cells, axes, actor, critic)
    x = np.asarray(obs).reshape(len(obs), -1).astype(np.float32)
    return ppo.forward_keep(nets[1], x, activation)[1][:, 0]


def vf_inputs(rng, v, clip_vf=CLIP_VF, dtype=np.float32):
    """``(value_old float32, ret dtype)`` of the classes of this file's docstring around the forward values v"""
    n = len(v)
    k = np.arange(n) % 5
    u, w = rng.uniform(0.8, 1.2, n), rng.uniform(0.8, 1.2, n)
    side = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    shift = np.select([k == 1, (k == 0) | (k == 2)], [side * 0.5 * clip_vf * u, 2.0 * clip_vf * u], -2.0 * clip_vf * u)
    sign = np.select([k == 1, (k == 0) | (k == 3)], [np.where(rng.random(n) < 0.5, -1.0, 1.0), 1.0], -1.0)
    v = np.asarray(v, dtype=np.float64)
    return (v + shift).astype(np.float32), (v + sign * w).astype(dtype)


def classes(R, value_old, ret, clip_vf=CLIP_VF):
    """the rows of every class, from what the statement's epilogue returned (``gradient``'s ``rows``), and the nearest the batch comes
    to a boundary: the smallest | |dvo| / clip_vf - 1 | over the live rows and the smallest | sqc / sq - 1 | outside the inside class"""
    live = R["skipped"] == 0
    v, vo, ret = R["value_new"].astype(np.float64), np.asarray(value_old, np.float32).astype(np.float64), np.asarray(ret).astype(np.float64)
    with np.errstate(all="ignore"):
        dvo = v - vo
        out, use = R["vf_clipped"] == 1, R["vf_use"] == 1
        rows = {"below": live & out & ~use & (dvo < 0), "inside": live & ~out, "below_use": live & out & use & (dvo < 0),
                "above_use": live & out & use & (dvo > 0), "above": live & out & ~use & (dvo > 0)}
        dc = np.clip(dvo, -clip_vf, clip_vf)
        sq, sqc = (v - ret) ** 2, ((vo + dc) - ret) ** 2
        edge = np.abs(np.abs(dvo[live]) / clip_vf - 1.0).min() if live.any() else np.inf
        tie = np.abs(sqc / sq - 1.0)[live & out].min() if (live & out).any() else np.inf
    return rows, edge, tie


def hold_classes(R, value_old, ret, clip_vf=CLIP_VF):
    """every class has min(4, rows // 5) rows at least, and no row stands within 1e-4 relative of a boundary; returns the counts"""
    rows, edge, tie = classes(R, value_old, ret, clip_vf)
    counts = {k: int(x.sum()) for k, x in rows.items()}
    live = int((R["skipped"] == 0).sum())
    assert sum(counts.values()) == live
    assert min(counts.values()) >= min(4, len(R["skipped"]) // 5), counts
    assert edge > 1e-4 and tie > 1e-4, (edge, tie)
    return counts


def autograd_vf(theta, cells, axes, actor, critic, activation, batch, value_old, clip_vf, dtype):
    """the gradient by torch autograd in ``dtype`` of the loss with the value loss 0.5 * max((v - ret)^2, (v_clipped - ret)^2), v_clipped
    = v_old + clamp(v - v_old, -clip_vf, clip_vf): per tensor in theta's order (std's apart), and the ratios"""
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
    vo = torch.tensor(np.asarray(value_old), dtype=dtype)

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
    vc = vo + torch.clamp(v - vo, -clip_vf, clip_vf)
    vloss = 0.5 * torch.maximum((v - t["ret"]) ** 2, (vc - t["ret"]) ** 2)
    loss = ploss.mean() + VF * vloss.mean() - ENT * (ls + 0.5 + policy.HALF_LOG_2PI).sum()
    loss.backward()
    return [x.grad.numpy().astype(np.float64) for x in leaves], r.detach().numpy().astype(np.float64)


def _case(k):
    n, cells, hidden, axes, activation, chain, seed = CASES[k]
    rng = np.random.default_rng(seed)
    theta = make_theta(rng, cells, axes, hidden, hidden)
    batch = make_batch(rng, theta, n, cells, axes, hidden, hidden, activation)
    return (theta, cells, axes, hidden, hidden, activation), batch, chain, rng


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


# ---------------------------------------------------------------------------------------------------------------- the defaults
@pytest.mark.parametrize("k", range(len(CASES)), ids=["relu-70", "tanh-300", "relu-257"])
def test_left_at_their_defaults_the_options_change_no_bit(k):
    """Fails without the feature: ``value_old`` and ``clip_vf`` are no arguments of the statement"""
    shape, batch, chain, _ = _case(k)
    hyper = dict(clip=CLIP, vf_coef=VF, ent_coef=ENT, max_grad_norm=0.5, rows_per_chain=chain)
    plain = ppo.gradient(*shape, **hyper, **batch)
    poison = np.full(len(batch["adv"]), np.nan, np.float32)
    for kw in (dict(value_old=None, clip_vf=0.0), dict(value_old=poison, clip_vf=0.0), dict(value_old=poison, clip_vf=0.0, stopped=True, kl_limit=0.0)):
        out = ppo.gradient(*shape, **hyper, **batch, **kw)
        for name in ("grad", "logp_new", "value_new", "ratio"):
            _same_bits(out[name], plain[name], name)
        assert list(out["stats"]) == list(ppo.STATS) and all(np.float64(out["stats"][s]).tobytes() == np.float64(plain["stats"][s]).tobytes() for s in ppo.STATS)
        assert out["more"]["vf_clip_fraction"] == 0.0 and out["more"]["applied"] == 1.0 and out["more"]["stopped"] == 0.0
        assert np.float64(out["more"]["explained_variance"]).tobytes() == np.float64(plain["more"]["explained_variance"]).tobytes()
    # and the epilogue alone
    nets = policy.unpack(*shape[:5])
    x = batch["obs"].astype(np.float32)
    args = (policy.forward(nets[0], x, shape[5]), policy.forward(nets[1], x, shape[5])[:, 0], nets[2], nets[3], batch["act"], batch["logp_old"], batch["adv"],
            batch["ret"], np.zeros(len(x), bool), CLIP, VF)
    one, two = ppo.rows(*args), ppo.rows(*args, value_old=poison, clip_vf=0.0)
    assert set(one) == set(two)
    for name in one:
        _same_bits(one[name], two[name], name)
    assert len(ppo.STATS) == 8 and ppo.STATS_MORE == ("vf_clip_fraction", "explained_variance", "applied", "stopped")


# ---------------------------------------------------------------------------------------------------------------- value-loss clipping
@pytest.mark.parametrize("k", [0, 1], ids=["relu-70", "tanh-300"])
def test_the_clipped_value_loss_against_float64_autograd(k):
    shape, batch, chain, rng = _case(k)
    cells, axes, hidden = shape[1], shape[2], shape[3]
    value_old, batch["ret"] = vf_inputs(rng, forward_value(*shape, batch["obs"]))
    hyper = dict(clip=CLIP, vf_coef=VF, ent_coef=ENT, max_grad_norm=0.0, rows_per_chain=chain)
    out = ppo.gradient(*shape, **hyper, **batch, value_old=value_old, clip_vf=CLIP_VF)
    counts = hold_classes(out["rows"], value_old, batch["ret"])
    print("rows per class:", counts)
    g64, r = autograd_vf(*shape, batch, value_old, CLIP_VF, torch.float64)
    assert min(np.abs(r - (1 + CLIP)).min(), np.abs(r - (1 - CLIP)).min()) > 1e-4
    g32, _ = autograd_vf(*shape, batch, value_old, CLIP_VF, torch.float32)
    mine, yard = pooled(split(out["grad"], cells, axes, hidden, hidden), g64), pooled(g32, g64)
    print("pooled distance from float64: the statement %.3e, float32 autograd %.3e, ratio %.2f" % (mine, yard, mine / yard))
    assert mine <= 4 * yard
    # the clipping is there: the critic's gradient is not the plain loss's, the actor's is, and the statistics say what was clipped
    plain = ppo.gradient(*shape, **hyper, **batch)
    a, b = split(out["grad"], cells, axes, hidden, hidden), split(plain["grad"], cells, axes, hidden, hidden)
    half = len(a) // 2
    assert all(np.array_equal(x, y) for x, y in zip(a[:half], b[:half])) and not any(np.array_equal(x, y) for x, y in zip(a[half:-1], b[half:-1]))
    n = len(batch["adv"])
    assert out["more"]["vf_clip_fraction"] == (n - counts["inside"]) / n and plain["more"]["vf_clip_fraction"] == 0.0
    assert out["stats"]["value_loss"] > plain["stats"]["value_loss"]      # (the max form never lowers a row's loss)
    assert out["more"]["explained_variance"] == plain["more"]["explained_variance"]      # (always of the unclipped diff)


def test_the_clipped_epilogue_on_hand_built_rows():
    """one axis, v = 0.25, c = 0.1: inside; out below and above, used and not; |dvo| exactly c is inside (strict), sqc == sq is not used"""
    vo = np.array([0.25, 0.5, 0.5, 0.0, 0.0, 0.15, 0.5], np.float32)
    ret = np.array([1.0, 1.0, -1.0, -1.0, 1.0, 1.0, 0.3])
    n = len(vo)
    kw = {"mean": np.zeros((n, 1), np.float32), "v": np.full(n, 0.25, np.float32), "log_std": [0.0], "std": [1.0], "act": np.full((n, 1), 0.5, np.float32),
          "logp_old": np.zeros(n, np.float32), "adv": np.ones(n), "ret": ret, "bad": np.zeros(n, bool)}
    c = np.float64(np.float32(0.1))
    R = ppo.rows(clip=CLIP, vf_coef=VF, ratio=np.ones(n), value_old=vo, clip_vf=c, **kw)
    # row 5: dvo = 0.25 - (double)0.15f, a hair below (double)0.1f: inside; row 6: vc = 0.5 - c = 0.4, diffc = 0.1, diff = -0.05 ... used
    assert R["vf_clipped"].tolist() == [0, 1, 1, 1, 1, 0, 1] and R["vf_use"].tolist() == [0, 0, 1, 0, 1, 0, 1]
    diff = 0.25 - ret
    assert R["dv"][1] == np.float32((VF * diff[1]) / n) and R["value_loss"][1] == 0.5 * (diff[1] * diff[1])
    low, high = (0.5 - c) - ret[2], (0.0 + c) - ret[4]
    assert R["dv"][2] == 0 and R["value_loss"][2] == 0.5 * (low * low)       # out and used: the clipped value is a constant
    assert R["dv"][4] == 0 and R["value_loss"][4] == 0.5 * (high * high)
    assert R["dv"][3] == np.float32((VF * diff[3]) / n)
    tie = ppo.rows(clip=CLIP, vf_coef=VF, ratio=np.ones(n), value_old=np.full(n, 0.25, np.float32), clip_vf=c, **kw)
    assert not tie["vf_use"].any() and not tie["vf_clipped"].any()      # dvo = 0: vc = v, sqc == sq, strict
    for bad in (np.nan, np.inf, -np.inf):
        poisoned = vo.copy()
        poisoned[3] = bad
        R = ppo.rows(clip=CLIP, vf_coef=VF, ratio=np.ones(n), value_old=poisoned, clip_vf=c, **kw)
        assert R["skipped"].tolist() == [0, 0, 0, 1, 0, 0, 0] and R["dv"][3] == 0 and R["ret"][3] == 0 and R["diff2"][3] == 0 and np.isnan(R["value_new"][3])
        assert ppo.rows(clip=CLIP, vf_coef=VF, ratio=np.ones(n), value_old=poisoned, clip_vf=0.0, **kw)["skipped"].sum() == 0
    for kw2, words in ((dict(clip_vf=-0.1, value_old=vo), "clip_vf"), (dict(clip_vf=np.inf, value_old=vo), "clip_vf"), (dict(clip_vf=np.nan, value_old=vo), "clip_vf"),
                       (dict(clip_vf=0.1), "value_old")):
        with pytest.raises(ValueError, match=words):
            ppo.rows(clip=CLIP, vf_coef=VF, ratio=np.ones(n), **kw, **kw2)


# ---------------------------------------------------------------------------------------------------------------- explained_variance
def _small(rng, n, ret):
    cells, axes, hidden = 6, 2, (5,)
    theta = make_theta(rng, cells, axes, hidden, hidden)
    batch = make_batch(rng, theta, n, cells, axes, hidden, hidden, "relu")
    batch["ret"] = np.asarray(ret, dtype=np.float64)
    batch["adv"] = batch["adv"].astype(np.float64)
    return (theta, cells, axes, hidden, hidden, "relu"), batch


@pytest.mark.parametrize("mean", [0.0, 50.0])
def test_explained_variance_is_numpys(mean):
    rng = np.random.default_rng(3)
    n = 200
    shape, batch = _small(rng, n, mean + rng.standard_normal(n))
    out = ppo.gradient(*shape, rows_per_chain=64, **batch)
    v = out["value_new"].astype(np.float64)
    want = 1.0 - np.var(batch["ret"] - v) / np.var(batch["ret"])
    print("explained_variance %.12f, numpy's %.12f" % (out["more"]["explained_variance"], want))
    assert abs(out["more"]["explained_variance"] - want) < 1e-9
    # a skipped row is left out of m
    batch["adv"][17] = np.nan
    out = ppo.gradient(*shape, rows_per_chain=64, **batch)
    keep = np.arange(n) != 17
    want = 1.0 - np.var(batch["ret"][keep] - v[keep]) / np.var(batch["ret"][keep])
    assert out["stats"]["skipped"] == 1 and abs(out["more"]["explained_variance"] - want) < 1e-9
    assert abs(want - (1.0 - np.var(batch["ret"] - v) / np.var(batch["ret"]))) > 1e-7      # (the row mattered)


def test_explained_variance_is_nan_for_constant_returns_and_for_an_all_skipped_batch():
    rng = np.random.default_rng(4)
    for const in (0.0, 2.0):      # (sums of these are exact: vr is exactly 0)
        shape, batch = _small(rng, 96, np.full(96, const))
        assert np.isnan(ppo.gradient(*shape, rows_per_chain=32, **batch)["more"]["explained_variance"])
    shape, batch = _small(rng, 40, rng.standard_normal(40))
    batch["logp_old"][:] = np.inf
    out = ppo.gradient(*shape, rows_per_chain=32, **batch)
    assert out["stats"]["skipped"] == 40 and np.isnan(out["more"]["explained_variance"])
    assert np.isnan(ppo.explained_variance(1.0, 1.0, 0.0, 0.0, 0)) and np.isnan(ppo.explained_variance(3.0, 3.0, 1.0, 1.0, 3))
    assert ppo.explained_variance(0.0, 2.0, 0.0, 0.5, 2) == 0.75


# ---------------------------------------------------------------------------------------------------------------- the gate
def test_the_gate_is_strict_sticky_and_a_nan_does_not_stop():
    limit = 1.5 * 0.02
    assert ppo.gate(False, limit, limit) == (False, True)
    assert ppo.gate(False, np.nextafter(limit, 1.0), limit) == (True, False)
    assert ppo.gate(False, np.nan, limit) == (False, True) and ppo.gate(False, -1.0, limit) == (False, True)
    assert ppo.gate(True, 0.0, limit) == (True, False) and ppo.gate(True, np.nan, limit) == (True, False)
    stopped, applied = False, []
    for kl in (0.01, 0.029, 0.031, 0.001, np.nan):
        stopped, a = ppo.gate(stopped, kl, limit)
        applied.append(a)
    assert applied == [True, True, False, False, False]
    # and through the gradient: the gate reads the update's own approx_kl, and the gradient and statistics are formed either way
    shape, batch, chain, _ = _case(0)
    free = ppo.gradient(*shape, rows_per_chain=chain, **batch)
    kl = free["stats"]["approx_kl"]
    assert kl > 0 and (free["more"]["applied"], free["more"]["stopped"]) == (1.0, 0.0)
    for kw, want in ((dict(kl_limit=kl), (1.0, 0.0)), (dict(kl_limit=np.nextafter(kl, 0.0)), (0.0, 1.0)), (dict(kl_limit=2 * kl, stopped=True), (0.0, 1.0))):
        out = ppo.gradient(*shape, rows_per_chain=chain, **batch, **kw)
        assert (out["more"]["applied"], out["more"]["stopped"]) == want, kw
        _same_bits(out["grad"], free["grad"], "grad")
        assert out["stats"] == free["stats"]
