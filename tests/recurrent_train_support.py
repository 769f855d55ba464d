"""What the suites of training through time share (tests/test_recurrent_train_cpu.py, tests/test_recurrent_train_gpu.py): a hand-made
sequence minibatch with every kind of cell in it, the statement's call over it, and the same loss in torch float64 with autograd."""
import numpy as np
import torch

from nuclear_sim_amd import policy, recurrent

CUT = recurrent.ROLLOUT_CUT


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def weights(seed, cells, H, A, actor, critic):
    """``(core, actor, critic, log_std)``: float32, rows of a size that makes the gates work without saturating all of them"""
    rng = np.random.default_rng(seed)

    def net(dims):
        return [((rng.standard_normal((o, i)) * (1.2 / np.sqrt(i))).astype(np.float32), (0.1 * rng.standard_normal(o)).astype(np.float32)) for i, o in dims]
    a, c = policy.sizes(H, A, actor, critic)
    core = tuple((rng.standard_normal(shape) * scale).astype(np.float32)
                 for shape, scale in (((3 * H, cells), 1.5 / np.sqrt(cells)), ((3 * H, H), 1.5 / np.sqrt(H)), ((3 * H,), 0.2), ((3 * H,), 0.2)))
    return core, net(a), net(c), (0.2 * rng.standard_normal(A) - 0.5).astype(np.float32)


def problem(seed, t, count, cells, H, A, actor, critic, gates, activation, special=True):
    """One sequence minibatch as a dict: theta and the shapes, the time-major tensors, the restart words and ``first``.  ``logp_old`` is the
    density under slightly different parameters, so that the ratios lie around 1 and some are clipped.  ``special``: plant 1 restarts in
    front of slot 3 by an episode change, plant 2 in front of slot 2 by a cut, plant 3 restarted in front of slot 0 (its ``first`` is
    +0.0), plant 4's slot 2 is poisoned (a NaN feature) and plant 5's slot 1 skipped (a NaN adv); plant count - 1 has both restarts"""
    rng = np.random.default_rng(seed)
    core, a, c, log_std = weights(seed, cells, H, A, actor, critic)
    theta = recurrent.pack(a, c, log_std, core=core)
    P = dict(cells=cells, n_axes=A, actor=tuple(actor), critic=tuple(critic), activation=activation, core=H, gates=gates, theta=theta, t=t, count=count)
    P["obs"] = rng.standard_normal((t, count, cells)).astype(np.float32)
    P["episode"] = np.tile(rng.integers(0, 5, count).astype(np.int32), (t, 1))
    P["ended"] = np.zeros((t, count), dtype=np.uint8)
    P["ended"][rng.random((t, count)) < 0.2] = 1      # (terminations and truncations alone restart nothing: the episode index does)
    P["first"] = rng.uniform(-1, 1, (count, H)).astype(np.float32)
    if special:
        P["episode"][3:, 1] += 1
        P["ended"][1, 2] |= CUT
        P["first"][3] = 0.0
        P["episode"][2:, count - 1] += 1
        P["ended"][3, count - 1] |= CUT
    # the actions and their old densities: a draw around the means of nearby parameters
    near = theta + (0.02 * rng.standard_normal(theta.size)).astype(np.float32)
    near[-A:] = np.exp(near[-2 * A:-A].astype(np.float64)).astype(np.float32)
    out = recurrent.gradient(near, cells, A, actor, critic, activation, H, gates, P["obs"], np.zeros((t, count, A), np.float32), np.zeros((t, count), np.float32),
                             np.ones((t, count), np.float32), np.zeros((t, count), np.float32), P["episode"], P["ended"], P["first"])
    nets = recurrent.unpack(near, cells, A, actor, critic, H)
    mean = policy.forward(nets[1], out["hidden"].reshape(t * count, H), activation).reshape(t, count, A)
    std = nets[4].astype(np.float64)
    z = rng.standard_normal((t, count, A))
    P["act"] = (mean + std * z).astype(np.float32)
    d = (P["act"].astype(np.float64) - mean) / std
    P["logp_old"] = (-(A * policy.HALF_LOG_2PI) - 0.5 * (d * d).sum(axis=2) - nets[3].astype(np.float64).sum()).astype(np.float32)
    P["adv"] = rng.standard_normal((t, count)).astype(np.float32)
    P["ret"] = (out["value_new"] + 0.5 * rng.standard_normal((t, count))).astype(np.float32)
    P["value_old"] = (out["value_new"] + 0.1 * rng.standard_normal((t, count))).astype(np.float32)
    if special:
        P["obs"][2, 4, cells // 2] = np.nan
        P["adv"][1, 5] = np.nan
    return P


EDGE_PLANTS = {"episode": 6, "cut": 7, "restarted": 8, "skipped": 9, "wide": 10}


def edges(P):
    """Plants the cells at time's edges and on the tile seam into a problem made with ``special=False`` (t >= 3, count >= 33), in place,
    and returns the ``skipped`` count they make.  EDGE_PLANTS names the plants:
      "episode" restarts by an episode change in front of the LAST slot, "cut" by a cut in front of slot 1;
      plant 31, the last of tile 0, is poisoned at slot 0 (a NaN); plant 32, the first of tile 1, at the last slot (an infinity);
      the last plant is poisoned at slots 1 and 2, two in a row (a NaN, then -infinity);
      "restarted" restarts in front of slot 2 and is poisoned there; "skipped" is poisoned at slot 1 and has a NaN adv there;
      float64 ``obs`` only: "wide" holds 1e300 at slot 1, finite as a double and an infinity once narrowed, so that cell is poisoned too."""
    t, count, cells = P["t"], P["count"], P["cells"]
    assert t >= 3 and count >= 33 and P["obs"].shape == (t, count, cells)
    E = EDGE_PLANTS
    P["episode"][t - 1:, E["episode"]] += 1
    P["ended"][0, E["cut"]] |= CUT
    P["episode"][2:, E["restarted"]] += 1
    poisoned = {(0, 31): (0, np.nan), (t - 1, 32): (cells - 1, np.inf), (1, count - 1): (cells // 2, np.nan), (2, count - 1): (0, -np.inf),
                (2, E["restarted"]): (1 % cells, np.nan), (1, E["skipped"]): (cells - 1, np.nan)}
    if P["obs"].dtype == np.float64:
        poisoned[(1, E["wide"])] = (0, 1e300)
    for (s, p), (k, value) in poisoned.items():
        P["obs"][s, p, k] = value
    P["adv"][1, E["skipped"]] = np.nan
    return len(poisoned)      # (distinct cells: with count = 33 and t = 3 the last plant's slot 2 IS plant 32's last slot)


def poisoned_cells(P):
    """bool [t, count]: the cells with a feature that is not finite once narrowed to float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        return ~np.isfinite(P["obs"].astype(np.float32)).all(axis=2)


def statement(P, fn=recurrent.gradient, **kw):
    args = dict(clip=0.2, vf_coef=0.5)
    args.update(kw)
    return fn(P["theta"], P["cells"], P["n_axes"], P["actor"], P["critic"], P["activation"], P["core"], P["gates"], P["obs"], P["act"], P["logp_old"],
              P["adv"], P["ret"], P["episode"], P["ended"], P["first"], **args)


def autograd(P, clip=0.2, vf_coef=0.5, ent_coef=0.0):
    """the gradient of the same loss by torch float64 autograd, in theta's layout (std's slots 0): the cell written out from clamps for hard
    gates.  A poisoned cell gives h' = 0 and no loss term; a skipped cell gives no loss term and carries.  The features are the float32
    roundings the policy reads, widened again: the loss is a function of those"""
    f64 = torch.float64
    theta = torch.tensor(P["theta"].astype(np.float64), requires_grad=True)
    cells, A, H, t, count = P["cells"], P["n_axes"], P["core"], P["t"], P["count"]
    at = [0]

    def take(*shape):
        n = int(np.prod(shape))
        v = theta[at[0]:at[0] + n].reshape(shape)
        at[0] += n
        return v
    W_ih, b_ih, W_hh, b_hh = take(3 * H, cells), take(3 * H), take(3 * H, H), take(3 * H)
    a_dims, c_dims = policy.sizes(H, A, P["actor"], P["critic"])
    a_net = [(take(o, i), take(o)) for i, o in a_dims]
    c_net = [(take(o, i), take(o)) for i, o in c_dims]
    log_std = take(A)
    hard = P["gates"] == "hard"
    S = (lambda a: torch.clamp(0.25 * a + 0.5, 0.0, 1.0)) if hard else torch.sigmoid
    T = (lambda a: torch.clamp(a, -1.0, 1.0)) if hard else torch.tanh
    act_fn = torch.relu if P["activation"] == "relu" else torch.tanh

    def mlp(net, x):
        for W, b in net[:-1]:
            x = act_fn(x @ W.T + b)
        return x @ net[-1][0].T + net[-1][1]
    fresh = recurrent.restarts(P["episode"], P["ended"])
    # the features as the policy reads them: narrowed to float32 (a double beyond float's range is an infinity); a poisoned cell's are +0.0
    bad = poisoned_cells(P)
    with np.errstate(over="ignore", invalid="ignore"):
        obs = np.where(bad[..., None], 0.0, P["obs"].astype(np.float32).astype(np.float64))
    skipped = bad | ~np.isfinite(P["adv"])
    h = torch.tensor(P["first"].astype(np.float64))
    loss = torch.zeros((), dtype=f64)
    for s in range(t):
        h = torch.where(torch.tensor(fresh[s])[:, None], torch.zeros_like(h), h)
        gi, gh = torch.tensor(obs[s]) @ W_ih.T + b_ih, h @ W_hh.T + b_hh
        r, z = S(gi[:, :H] + gh[:, :H]), S(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = T(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = n + z * (h - n)
        h = torch.where(torch.tensor(bad[s])[:, None], torch.zeros_like(h), h)
        mean, v = mlp(a_net, h), mlp(c_net, h)[:, 0]
        d = (torch.tensor(P["act"][s].astype(np.float64)) - mean) / torch.exp(log_std)
        lp = -(A * policy.HALF_LOG_2PI) - 0.5 * (d * d).sum(dim=1) - log_std.sum()
        ratio = torch.exp(lp - torch.tensor(P["logp_old"][s].astype(np.float64)))
        adv = torch.tensor(np.nan_to_num(P["adv"][s].astype(np.float64), nan=0.0))
        surrogate = -torch.minimum(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv)
        value = 0.5 * (v - torch.tensor(P["ret"][s].astype(np.float64))) ** 2
        keep = torch.tensor(~skipped[s])
        loss = loss + torch.where(keep, surrogate + vf_coef * value, torch.zeros_like(value)).sum()
    loss = loss / (t * count) - ent_coef * (log_std + 0.5 + policy.HALF_LOG_2PI).sum()
    loss.backward()
    g = theta.grad.numpy().copy()
    g[-A:] = 0.0
    return g


def distance(g, want):
    """the pooled relative distance |g - want| / |want| over every entry"""
    g, want = np.asarray(g, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.sqrt(((g - want) ** 2).sum() / (want ** 2).sum()))
