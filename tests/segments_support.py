"""What the suites of truncated segments share (tests/test_segments_cpu.py, tests/test_segments_gpu.py): a hand-made ROLLOUT with every kind
of cell placed against the segment boundaries, its stored states, the segment minibatch cut from it, the statement's call over that, and
the same loss in torch float64 with autograd, the state detached at every segment boundary and the stored states fed as constants."""
import numpy as np
import torch

from nuclear_sim_amd import policy, recurrent
from recurrent_train_support import CUT, problem

NAMES = ("obs", "act", "logp_old", "adv", "ret", "value_old")


def rollout_problem(seed, t, n, cells, H, A, actor, critic, gates, activation, every):
    """``recurrent_train_support.problem`` read as a rollout of t slots by n plants, its special cells laid out against segments of
    ``every`` slots (L):
      plant 1 restarts by an episode change ON a segment boundary (in front of slot L; with one chunk: in front of slot 0, first = +0.0);
      plant 2 restarts by a cut INSIDE a segment (in front of slot 1; with L = 1 every slot is a boundary);
      plant 4's cell at slot L - 1, the last of segment 0, is poisoned: the next segment's stored state is +0.0;
      plant 5's cell at slot t - 2 is skipped (a NaN adv).
    Adds ``every``, ``chunks``, ``n`` and ``starts`` [chunks, n, H], the stored states under the problem's own theta"""
    L = int(every)
    R = problem(seed, t, n, cells, H, A, actor, critic, gates, activation, special=False)
    if L < t:
        R["episode"][L:, 1] += 1
    else:
        R["first"][1] = 0.0
    R["ended"][0, 2] |= CUT
    R["obs"][L - 1, 4, cells // 2] = np.nan
    R["adv"][t - 2, 5] = np.nan
    core = recurrent.unpack(R["theta"], cells, A, actor, critic, H)[0]
    R.update(every=L, chunks=t // L, n=n, starts=recurrent.starts(R["first"], R["obs"], R["episode"], R["ended"], core, gates, L))
    return R


def segment_batch(R, index=None):
    """the segments ``index`` (None: all of them, in id order) of the rollout problem as one sequence minibatch: a dict shaped like
    ``problem``'s with t = every and count = the segments, its restart words and ``first`` the section-5 equivalents, plus ``index``"""
    L, n = R["every"], R["n"]
    g = np.arange(R["chunks"] * n, dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
    ok = (g >= 0) & (g < R["chunks"] * n)
    safe = np.where(ok, g, 0)
    slots, cols = (safe // n)[None, :] * L + np.arange(L)[:, None], (safe % n)[None, :]
    Q = {k: R[k] for k in ("cells", "n_axes", "actor", "critic", "activation", "core", "gates", "theta")}
    Q.update(t=L, count=len(g), index=g.astype(np.int32), valid=ok)
    for name in NAMES:
        Q[name] = np.ascontiguousarray(R[name][slots, cols])
    Q["episode"], Q["ended"], _ = recurrent.segment_words(R["episode"], R["ended"], g, n, L)
    Q["first"] = R["starts"].reshape(-1, R["core"])[safe]
    return Q


def statement_segments(R, Q, fn=recurrent.gradient_segments, **kw):
    """``recurrent.gradient_segments`` (or ``shard_sums_segments``) over the batch Q of the rollout problem R"""
    args = dict(clip=0.2, vf_coef=0.5)
    args.update(kw)
    return fn(R["theta"], R["cells"], R["n_axes"], R["actor"], R["critic"], R["activation"], R["core"], R["gates"], Q["obs"], Q["act"], Q["logp_old"],
              Q["adv"], Q["ret"], R["episode"], R["ended"], R["starts"], Q["index"], R["n"], R["every"], **args)


def autograd_truncated(R, clip=0.2, vf_coef=0.5, ent_coef=0.0):
    """The gradient of the PPO loss over ALL cells of the rollout problem by torch float64 autograd, in theta's layout (std's slots 0), with
    the hidden state REPLACED in front of every slot c * every by the constant ``starts[c]`` -- no gradient flows across a boundary, and the
    forward pass starts every segment from the stored state.  The walk is over the rollout's own [t, n] tensors, slot by slot: nothing of
    the segment gather or of ``segment_words`` is used"""
    f64 = torch.float64
    theta = torch.tensor(R["theta"].astype(np.float64), requires_grad=True)
    cells, A, H, t, n, L = R["cells"], R["n_axes"], R["core"], R["t"], R["n"], R["every"]
    at = [0]

    def take(*shape):
        k = int(np.prod(shape))
        v = theta[at[0]:at[0] + k].reshape(shape)
        at[0] += k
        return v
    W_ih, b_ih, W_hh, b_hh = take(3 * H, cells), take(3 * H), take(3 * H, H), take(3 * H)
    a_dims, c_dims = policy.sizes(H, A, R["actor"], R["critic"])
    a_net = [(take(o, i), take(o)) for i, o in a_dims]
    c_net = [(take(o, i), take(o)) for i, o in c_dims]
    log_std = take(A)
    hard = R["gates"] == "hard"
    S = (lambda a: torch.clamp(0.25 * a + 0.5, 0.0, 1.0)) if hard else torch.sigmoid
    T = (lambda a: torch.clamp(a, -1.0, 1.0)) if hard else torch.tanh
    act_fn = torch.relu if R["activation"] == "relu" else torch.tanh

    def mlp(net, x):
        for W, b in net[:-1]:
            x = act_fn(x @ W.T + b)
        return x @ net[-1][0].T + net[-1][1]
    fresh = recurrent.restarts(R["episode"], R["ended"])
    obs = np.nan_to_num(R["obs"].astype(np.float64), nan=0.0)
    bad = ~np.isfinite(R["obs"]).all(axis=2)
    skipped = bad | ~np.isfinite(R["adv"])
    h = None
    loss = torch.zeros((), dtype=f64)
    for s in range(t):
        if s % L == 0:      # a boundary: the stored state, a constant; the restart in front of it is in it already
            h = torch.tensor(R["starts"][s // L].astype(np.float64))
        else:
            h = torch.where(torch.tensor(fresh[s])[:, None], torch.zeros_like(h), h)
        gi, gh = torch.tensor(obs[s]) @ W_ih.T + b_ih, h @ W_hh.T + b_hh
        r, z = S(gi[:, :H] + gh[:, :H]), S(gi[:, H:2 * H] + gh[:, H:2 * H])
        c = T(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = c + z * (h - c)
        h = torch.where(torch.tensor(bad[s])[:, None], torch.zeros_like(h), h)
        mean, v = mlp(a_net, h), mlp(c_net, h)[:, 0]
        d = (torch.tensor(R["act"][s].astype(np.float64)) - mean) / torch.exp(log_std)
        lp = -(A * policy.HALF_LOG_2PI) - 0.5 * (d * d).sum(dim=1) - log_std.sum()
        ratio = torch.exp(lp - torch.tensor(R["logp_old"][s].astype(np.float64)))
        adv = torch.tensor(np.nan_to_num(R["adv"][s].astype(np.float64), nan=0.0))
        surrogate = -torch.minimum(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv)
        value = 0.5 * (v - torch.tensor(R["ret"][s].astype(np.float64))) ** 2
        keep = torch.tensor(~skipped[s])
        loss = loss + torch.where(keep, surrogate + vf_coef * value, torch.zeros_like(value)).sum()
    loss = loss / (t * n) - ent_coef * (log_std + 0.5 + policy.HALF_LOG_2PI).sum()
    loss.backward()
    g = theta.grad.numpy().copy()
    g[-A:] = 0.0
    return g
