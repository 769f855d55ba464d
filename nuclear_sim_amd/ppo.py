"""Training the policy on the device, stated once in numpy: what ``env.policy_grad`` and ``env.policy_adam`` compute (npb_policy_grad,
npb_policy_adam, nuclear_sim_amd/csrc/npb_ppo.hip).  Host only.  This statement is the contract, as ``policy.py`` is the forward pass's;
the device gives its bits for every count, storage type and launch geometry, with the forward pass's licensed float ``tanh`` and TWO more
licensed differences: the device's double ``exp`` for the ratio ``r`` and for ``std`` (``ratio=`` and ``std=`` take the device's own
values back, as ``Policy.step`` takes ``z=``).

THE INPUTS.  One minibatch of ``count`` rows as ``rollout_minibatches`` yields them: ``obs`` [count, K * C] float32 (a float64 one narrowed,
round to nearest even), ``act`` [count, A] of the controls' input type, ``logp_old`` float32, ``adv`` and ``ret`` float32 or float64.  The
hyper-parameters ``clip``, ``vf_coef``, ``ent_coef``, ``max_grad_norm`` (0 = off) are doubles.  ``rows_per_chain`` (a positive multiple of
32, default 256) is an argument of THIS statement: it pins the order of the sums over rows, and is not a property of any launch.

A SKIPPED ROW is one with a feature (after the narrowing), an action, ``logp_old``, ``adv`` or ``ret`` that is not finite.  Its features
are read as +0.0, every seed and every term of it is +0.0, it is counted in ``skipped``, and its ``logp_new``, ``value_new`` and ``ratio``
are THE quiet NaN.  The divisor stays ``count``.

THE FORWARD PASS is ``policy.forward`` for both nets, every hidden activation kept: ``mean`` float32 [count, A], ``v`` float32 [count].

PER ROW (``rows``), in double, every operation rounded on its own:

    d[a]  = ((double)act[a] - (double)mean[a]) / (double)std[a]
    lp    = -(A * HALF_LOG_2PI);  for a ascending  lp = (lp - 0.5 * (d[a] * d[a])) - (double)log_std[a]
    lr    = lp - (double)logp_old;  r = exp(lr)
    clipped = (adv > 0 and r > 1 + clip) or (adv < 0 and r < 1 - clip)          every comparison strict
    c     = clipped ? 0.0 : -(adv * r)
    dmean[a] = (float)(((c * d[a]) / std[a]) / count)        dv = (float)((vf_coef * ((double)v - ret)) / count)        the seeds
    dls[a]   = (c * (d[a] * d[a] - 1.0)) / count
    policy loss = -min(r * adv, clamp(r, 1 - clip, 1 + clip) * adv);  value loss = 0.5 * (((double)v - ret) * ((double)v - ret))
    kl = (r - 1.0) - lr

An infinite ``r`` is outside the contract.

THE BACKWARD PASS (``backward``), float32, per net, from the head down.  ``back[i][k] = acc`` with ``acc = +0.0`` and then for j ascending
``acc = fmaf(delta[i][j], W[j][k], acc)``, j extended with +0.0 to a multiple of 4.  relu: ``delta' = h > 0 ? back : +0.0``.  tanh:
``delta' = back * (1.0f - h * h)``: three rounded operations, no contraction.

THE SUMS OVER ROWS ARE THE CONTRACT (``chain_sums``).  The rows are cut into chains of ``rows_per_chain`` rows.  Within a chain
``dW[j][k]`` starts at +0.0 and is ``fmaf(delta[i][j], h[i][k], acc)`` for i ascending, ``db[j]`` the same with h = 1.0f; the last chain
is extended with +0.0 rows to a multiple of 32 (which changes no bit: an accumulator here is never -0.0).  Across chains each parameter's
partials are widened to double, added in ascending chain order onto 0.0 and narrowed once.  The per-row doubles (``dls``, the four
statistics, the skipped count) are added the same way: rows ascending within a chain onto 0.0, then the chains ascending onto 0.0.
``grad(log_std[a]) = (float)(sum dls[a] - ent_coef)``; ``grad(std[a]) = 0``: std is derived, not a parameter.  The entropy is ``sum_a
((log_std[a] + 0.5) + HALF_LOG_2PI)``, a ascending onto 0.0; it is reported, and its gradient is the ``- ent_coef`` above.

CLIPPING (``clip_grad``).  ``norm = sqrt(_tree((double)g * (double)g))`` over every entry but std's, in theta's order.  With
``max_grad_norm > 0``: ``s = min(1.0, max_grad_norm / (norm + 1e-6))`` and ``g = (float)((double)g * s)``.

ADAM (``adam``).  The state is ``m``, ``v`` (float32, theta's layout) and ``step``.  ``step`` advances first; the host forms ``step_size
= lr / (1 - b1^step)`` and ``root = sqrt(1 - b2^step)`` in Python doubles, and ``1 - b1``, ``1 - b2``.  Per element, in double, every
operation rounded on its own, each result narrowed once:

    m' = (float)(b1 * m + (1 - b1) * g)        v' = (float)(b2 * v + (1 - b2) * (g * g))
    theta' = (float)(theta - step_size * (m' / (sqrt(v') / root + eps)))          (m', v': the narrowed values)

std's slots are skipped in all three; then ``std[a] = (float)exp((double)log_std'[a])``.

``stats`` is float64: ``{policy_loss, value_loss, entropy, approx_kl, clip_fraction, skipped, grad_norm, count}`` (``STATS`` has the
order); the first five are means over ``count`` (the entropy is the same for every row).

THE OPTIONS.  Left at their defaults, every function here returns the bits it returned before they existed.

VALUE-LOSS CLIPPING (``value_old`` [count] float32, ``clip_vf`` a double, 0.0 = off), the max form of baselines' PPO2.  Per row, in
double, every operation rounded on its own, behind ``diff = (double)v - ret``:

    dvo  = (double)v - (double)value_old
    dc   = dvo < -clip_vf ? -clip_vf : (dvo > clip_vf ? clip_vf : dvo)
    vc   = (double)value_old + dc;   diffc = vc - ret
    sq   = diff * diff;   sqc = diffc * diffc
    use  = sqc > sq                                 (strict)
    out  = dvo < -clip_vf or dvo > clip_vf          (strict)
    value loss = 0.5 * (use ? sqc : sq)
    dv   = (float)((vf_coef * (use ? (out ? 0.0 : diffc) : diff)) / count)
    vf_clipped = out ? 1.0 : 0.0

With ``clip_vf > 0`` a ``value_old`` that is not finite makes the row a skipped row; with ``clip_vf == 0`` it is not read and may be absent.

MORE STATISTICS, always formed.  Four more per-row doubles, +0.0 on a skipped row: ``ret``, ``ret * ret``, ``diff`` and ``diff * diff``
(always the unclipped ``diff``), summed as the other per-row doubles are.  From the sums ``S_r, S_rr, S_d, S_dd`` and ``m = count -
skipped`` (``explained_variance``):

    vr = S_rr / m - (S_r / m) * (S_r / m);   vd = S_dd / m - (S_d / m) * (S_d / m);   explained_variance = 1.0 - vd / vr

THE quiet NaN when ``m < 1`` or not ``vr > 0``.  ``more`` is float64: ``{vf_clip_fraction, explained_variance, applied, stopped}``
(``STATS_MORE`` has the order); ``vf_clip_fraction`` is the pinned sum of ``vf_clipped`` over ``count``.

THE GATE (``gate``), target_kl early stopping as SB3 takes it: the check comes before the optimiser step of the offending minibatch.
``kl_limit = 1.5 * target_kl``, formed by the caller in double.

    stopped' = stopped or (approx_kl > kl_limit)      (strict; a NaN approx_kl does not stop)
    applied  = not stopped'

An update that is not applied leaves theta, ``std``, ``m`` and ``v`` exactly as they were; its gradient and all its statistics are still
formed.  Once stopped, every later update of the same training call is not applied.  Adam's ``step`` counts applied updates only: within
one call they are a prefix, so update ``i`` (0-based), if applied, is step ``step0 + i + 1``.

ONE POLICY ACROSS SHARDS (``shard_sums``, ``combine``; npb_policy_shard_sums, npb_policy_apply_shards).  An update over ``count_total``
rows held by W shards (the devices of a node, two handles on one device, or successive minibatches of one handle) is cut where the pinned
double sums end.  A shard's VECTOR is float64 [L], ``L = shard_size(theta_size, A) = theta_size - 2 * A + 18``: every weight and bias
slot in theta's layout, up to where ``log_std`` starts, each ``across(chain partials)`` as the double it is; then the 18 per-row sums
``row_sums(...)`` in ``SHARD_ROWS``'s order: ``dls[a]`` at a < 8 (+0.0 beyond A), ``policy_loss`` 8, ``kl`` 9, ``clipped`` 10,
``skipped`` 11, ``value_loss`` 12, ``vf_clipped`` 13, ``ret`` 14, ``ret2`` 15, ``diff`` 16, ``diff2`` 17.  ``ent_coef`` is not yet
subtracted.  ONE change in the per-row arithmetic: wherever ``gradient`` divides a seed by ``count`` (``dmean``, ``dv``, ``dls``), a shard
divides by ``(double)count_total``; skipped rows behave as they do there.  THE COMBINE:

    total = 0.0;  for w ascending  total = total + shards[w]                    (in double, entry by entry)
    grad[e] = (float)total[e];  grad(log_std[a]) = (float)(total_dls[a] - ent_coef);  grad(std[a]) = 0

then ``clip_grad``, the ``STATS`` and ``STATS_MORE`` of ``gradient`` with ``count = count_total`` and the totals for the sums, and
``gate`` on the GLOBAL ``approx_kl``.  Every replica that combines the same W vectors computes the same bits, so replicas that apply
``adam`` to them stay identical with no broadcast of parameters.  THE INVARIANT: ``combine(shard_sums(..., count_total=count)[None],
...)`` has the bits of ``gradient(...)``: no sum over the chains is ever -0.0, so ``0.0 + x`` is ``x``."""
import numpy as np

from .policy import HALF_LOG_2PI, activate, fmaf, layer, unpack
from .rollout import _tree

STATS = ("policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "skipped", "grad_norm", "count")
STATS_MORE = ("vf_clip_fraction", "explained_variance", "applied", "stopped")
SHARD_ROWS = ("dls0", "dls1", "dls2", "dls3", "dls4", "dls5", "dls6", "dls7", "policy_loss", "kl", "clipped", "skipped", "value_loss",
              "vf_clipped", "ret", "ret2", "diff", "diff2")      # NPD_PPO_* of csrc/npb_ppo.h: the per-row sums in the device's order
SHARDS_MAX = 64      # NPB_PPO_SHARDS_MAX
ROWS_PER_CHAIN = 256
TILE = 32


def check(count, rows_per_chain, clip):
    """refuse what npb_ppo_check refuses of the numbers, by name"""
    if int(count) < 1:
        raise ValueError("count must be >= 1")
    if int(rows_per_chain) < TILE or int(rows_per_chain) % TILE:
        raise ValueError("rows_per_chain must be a positive multiple of 32, not %r" % (rows_per_chain,))
    if not 0.0 < float(clip) < 1.0:
        raise ValueError("clip must lie inside (0, 1), not %r" % (clip,))


def check_clip_vf(clip_vf, value_old):
    """``clip_vf`` as a float: refused, by name, when negative or not finite, or positive with no ``value_old``"""
    clip_vf = float(clip_vf)
    if not 0.0 <= clip_vf < float("inf"):
        raise ValueError("clip_vf must be finite and >= 0 (0 = off), not %r" % (clip_vf,))
    if clip_vf > 0.0 and value_old is None:
        raise ValueError("clip_vf > 0 needs value_old")
    return clip_vf


def forward_keep(net, x, activation):
    """``(inputs, head)``: the float32 input of every layer of the net (the rows first, then each hidden activation) and the head's
    outputs, exactly ``policy.forward``"""
    hs = [np.asarray(x, dtype=np.float32)]
    for W, b in net[:-1]:
        hs.append(activate(layer(hs[-1], W, b), activation))
    return hs, layer(hs[-1], *net[-1])


def rows(mean, v, log_std, std, act, logp_old, adv, ret, bad, clip, vf_coef, ratio=None, value_old=None, clip_vf=0.0, count_total=None):
    """the per-row epilogue: a dict of ``dmean`` float32 [n, A], ``dv`` float32 [n], ``dls`` float64 [n, A], ``policy_loss``,
    ``value_loss``, ``kl``, ``clipped``, ``skipped`` float64 [n], and ``logp_new``, ``value_new`` float32 [n], ``ratio`` float64 [n];
    and ``vf_clipped``, ``ret``, ``ret2``, ``diff``, ``diff2`` float64 [n], the options' per-row doubles, with ``vf_use`` (not summed).
    ``bad``: the rows with a feature that is not finite.  ``ratio``: the device's own r in place of numpy's exp.  ``value_old`` float32
    [n] and ``clip_vf`` > 0: the value loss clipped.  ``count_total``: the seeds' divisor (``dmean``, ``dv``, ``dls``) in place of n, for
    a shard's rows of a larger update (``shard_sums``)"""
    mean = np.asarray(mean, dtype=np.float32).astype(np.float64)
    n, A = mean.shape
    count = np.float64(n if count_total is None else int(count_total))
    clip, vf_coef = np.float64(clip), np.float64(vf_coef)
    log_std, std = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (log_std, std))
    act = np.asarray(act).astype(np.float64).reshape(n, A)
    old = np.asarray(logp_old, dtype=np.float32).astype(np.float64).reshape(n)
    adv, ret = (np.asarray(x).astype(np.float64).reshape(n) for x in (adv, ret))
    vd = np.asarray(v, dtype=np.float32).astype(np.float64).reshape(n)
    skipped = np.asarray(bad, dtype=bool) | ~np.isfinite(act).all(axis=1) | ~np.isfinite(old) | ~np.isfinite(adv) | ~np.isfinite(ret)
    clip_vf = np.float64(check_clip_vf(clip_vf, value_old))
    if clip_vf > 0.0:
        vo = np.asarray(value_old, dtype=np.float32).astype(np.float64).reshape(n)
        skipped = skipped | ~np.isfinite(vo)
    with np.errstate(all="ignore"):
        d = (act - mean) / std[None, :]
        lp = np.full(n, -(A * HALF_LOG_2PI))
        for a in range(A):
            lp = (lp - 0.5 * (d[:, a] * d[:, a])) - log_std[a]
        lr = lp - old
        r = np.exp(lr) if ratio is None else np.asarray(ratio, dtype=np.float64).reshape(n)
        lo, hi = 1.0 - clip, 1.0 + clip
        clipped = ((adv > 0.0) & (r > hi)) | ((adv < 0.0) & (r < lo))
        c = np.where(clipped, 0.0, -(adv * r))
        dmean = (((c[:, None] * d) / std[None, :]) / count).astype(np.float32)
        diff = vd - ret
        sq = diff * diff
        seed, lsq, out_vf, use = diff, sq, np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        if clip_vf > 0.0:
            dvo = vd - vo
            dc = np.where(dvo < -clip_vf, -clip_vf, np.where(dvo > clip_vf, clip_vf, dvo))
            diffc = (vo + dc) - ret
            sqc = diffc * diffc
            use, out_vf = sqc > sq, (dvo < -clip_vf) | (dvo > clip_vf)
            seed, lsq = np.where(use, np.where(out_vf, 0.0, diffc), diff), np.where(use, sqc, sq)
        dv = ((vf_coef * seed) / count).astype(np.float32)
        dls = (c[:, None] * (d * d - 1.0)) / count
        rc = np.where(r < lo, lo, np.where(r > hi, hi, r))
        first, second = r * adv, rc * adv
        ploss = -np.where(second < first, second, first)
        vloss = 0.5 * lsq
        kl = (r - 1.0) - lr
    out = {"dmean": dmean, "dv": dv, "dls": dls, "policy_loss": ploss, "value_loss": vloss, "kl": kl, "clipped": clipped.astype(np.float64),
           "logp_new": lp.astype(np.float32), "value_new": np.asarray(v, dtype=np.float32).reshape(n).copy(), "ratio": np.array(r, dtype=np.float64),
           "vf_clipped": out_vf.astype(np.float64), "ret": ret.copy(), "ret2": ret * ret, "diff": diff.copy(), "diff2": sq.copy(), "vf_use": use.astype(np.float64)}
    for name in ("dmean", "dv", "dls", "policy_loss", "value_loss", "kl", "clipped", "vf_clipped", "ret", "ret2", "diff", "diff2", "vf_use"):
        out[name][skipped] = 0.0
    for name in ("logp_new", "value_new", "ratio"):
        out[name][skipped] = np.nan
    out["skipped"] = skipped.astype(np.float64)
    return out


def back(delta, W):
    """``back[i][k]``: the fmaf chain over j ascending from +0.0, j extended with +0.0 to a multiple of 4"""
    delta, W = np.asarray(delta, dtype=np.float32), np.asarray(W, dtype=np.float32)
    n, J = delta.shape
    pad = -J % 4
    if pad:
        delta = np.concatenate([delta, np.zeros((n, pad), np.float32)], axis=1)
        W = np.concatenate([W, np.zeros((pad, W.shape[1]), np.float32)], axis=0)
    acc = np.zeros((n, W.shape[1]), dtype=np.float32)
    for j in range(J + pad):
        acc = fmaf(delta[:, j:j + 1], W[j][None, :], acc)
    return acc


def through(backed, h, activation):
    """``delta'`` of ``back`` and the hidden activation h it passes"""
    if activation == "relu":
        return np.where(h > 0, backed, np.float32(0.0)).astype(np.float32)
    one = np.float32(1.0)
    return (backed * (one - h * h)).astype(np.float32)


def chain_sums(delta, h, rows_per_chain):
    """``dW`` float32 [chains, J, K] and ``db`` float32 [chains, J]: every chain's own sums over its rows, i ascending from +0.0"""
    delta, h = np.asarray(delta, dtype=np.float32), np.asarray(h, dtype=np.float32)
    n, R = len(delta), int(rows_per_chain)
    chains = -(-n // R)
    pad = chains * R - n      # (whole chains of +0.0 rows: what the extension to a multiple of 32 adds, and further rows that change no bit)
    if pad:
        delta = np.concatenate([delta, np.zeros((pad, delta.shape[1]), np.float32)])
        h = np.concatenate([h, np.zeros((pad, h.shape[1]), np.float32)])
    delta, h = delta.reshape(chains, R, -1), h.reshape(chains, R, -1)
    dW = np.zeros((chains, delta.shape[2], h.shape[2]), dtype=np.float32)
    db = np.zeros((chains, delta.shape[2]), dtype=np.float32)
    one = np.float32(1.0)
    for i in range(R):
        dW = fmaf(delta[:, i, :, None], h[:, i, None, :], dW)
        db = fmaf(delta[:, i], one, db)
    return dW, db


def across(partials):
    """[chains, ...] -> [...]: widened, added in ascending chain order onto 0.0; the caller narrows"""
    partials = np.asarray(partials)
    total = np.zeros(partials.shape[1:], dtype=np.float64)
    for c in range(len(partials)):
        total = total + partials[c].astype(np.float64)
    return total


def row_sums(x, rows_per_chain):
    """the pinned sum of per-row doubles x [n] or [n, q]: rows ascending onto 0.0 within a chain, the chains ascending onto 0.0"""
    x = np.asarray(x, dtype=np.float64)
    n, R = len(x), int(rows_per_chain)
    total = np.zeros(x.shape[1:], dtype=np.float64)
    for first in range(0, n, R):
        acc = np.zeros(x.shape[1:], dtype=np.float64)
        for i in range(first, min(first + R, n)):
            acc = acc + x[i]
        total = total + acc
    return total


def backward(net, inputs, seed, activation, rows_per_chain, wide=False):
    """the gradient of one net, ``[(dW float32 [out, in], db float32 [out])]`` in the net's order, of the head's seed [n, out]; ``wide``:
    the float64 sums over the chains as they are, not narrowed"""
    delta = np.asarray(seed, dtype=np.float32)
    grads = [None] * len(net)
    for l in range(len(net) - 1, -1, -1):
        dW, db = chain_sums(delta, inputs[l], rows_per_chain)
        grads[l] = (across(dW), across(db)) if wide else (across(dW).astype(np.float32), across(db).astype(np.float32))
        if l:
            delta = through(back(delta, net[l][0]), inputs[l], activation)
    return grads


def entropy(log_std):
    total = np.float64(0.0)
    for x in np.asarray(log_std, dtype=np.float32).astype(np.float64):
        total = total + ((x + 0.5) + HALF_LOG_2PI)
    return total


def clip_grad(grad, n_axes, max_grad_norm):
    """``(grad', norm)``: the norm over every entry but std's through ``_tree``, and the scaled gradient"""
    g = np.asarray(grad, dtype=np.float32).copy()
    A = int(n_axes)
    wide = g[:g.size - A].astype(np.float64)
    norm = np.sqrt(_tree(wide * wide))
    if float(max_grad_norm) > 0.0:
        with np.errstate(all="ignore"):
            s = np.float64(max_grad_norm) / (norm + 1e-6)
            s = np.float64(1.0) if not s < 1.0 else s
            g[:g.size - A] = (wide * s).astype(np.float32)
    return g, np.float64(norm)


def explained_variance(s_r, s_rr, s_d, s_dd, m):
    """``1 - var(ret - v) / var(ret)`` from the four pinned sums over the ``m`` rows that were not skipped; THE quiet NaN when ``m < 1``
    or not ``vr > 0``"""
    m = np.float64(m)
    if not m >= 1.0:
        return np.float64(np.nan)
    with np.errstate(all="ignore"):
        mr, md = np.float64(s_r) / m, np.float64(s_d) / m
        vr = np.float64(s_rr) / m - mr * mr
        vd = np.float64(s_dd) / m - md * md
        if not vr > 0.0:
            return np.float64(np.nan)
        return np.float64(1.0) - vd / vr


def gate(stopped, approx_kl, kl_limit):
    """``(stopped', applied)`` of one update: strict, sticky, and a NaN ``approx_kl`` does not stop"""
    stopped = bool(stopped) or bool(np.float64(approx_kl) > np.float64(kl_limit))
    return stopped, not stopped


def gradient(theta, cells, n_axes, actor, critic, activation, obs, act, logp_old, adv, ret, clip=0.2, vf_coef=0.5, ent_coef=0.0,
             max_grad_norm=0.5, rows_per_chain=ROWS_PER_CHAIN, ratio=None, value_old=None, clip_vf=0.0, stopped=False, kl_limit=0.0):
    """``{"grad", "stats", "more", "rows", "logp_new", "value_new", "ratio"}`` of one minibatch: grad float32 in theta's layout
    (clipped), stats a dict of float64 (``STATS``), more a dict of float64 (``STATS_MORE``), rows what ``rows`` returned.  ``stopped`` and ``kl_limit`` (0 = no gate) are the
    gate's: ``more``'s ``applied`` and ``stopped`` are what it says of this update"""
    obs = np.asarray(obs)
    n = len(obs)
    check(n, rows_per_chain, clip)
    A = int(n_axes)
    nets = unpack(theta, cells, A, actor, critic)
    with np.errstate(over="ignore", invalid="ignore"):
        x = obs.reshape(n, -1).astype(np.float32)
    bad = ~np.isfinite(x).all(axis=1)
    per_row_bad = bad | ~np.isfinite(np.asarray(act).astype(np.float64).reshape(n, A)).all(axis=1) | \
        ~np.isfinite(np.asarray(logp_old, dtype=np.float64).reshape(n)) | ~np.isfinite(np.asarray(adv, dtype=np.float64).reshape(n)) | \
        ~np.isfinite(np.asarray(ret, dtype=np.float64).reshape(n))
    if check_clip_vf(clip_vf, value_old) > 0.0:
        per_row_bad = per_row_bad | ~np.isfinite(np.asarray(value_old, dtype=np.float32).reshape(n))
    x = x.copy()
    x[per_row_bad] = 0.0
    a_in, mean = forward_keep(nets[0], x, activation)
    c_in, value = forward_keep(nets[1], x, activation)
    R = rows(mean, value[:, 0], nets[2], nets[3], act, logp_old, adv, ret, bad, clip, vf_coef, ratio, value_old, clip_vf)
    parts = []
    for net, inputs, seed in ((nets[0], a_in, R["dmean"]), (nets[1], c_in, R["dv"][:, None])):
        for dW, db in backward(net, inputs, seed, activation, rows_per_chain):
            parts += [dW.reshape(-1), db]
    dls = (row_sums(R["dls"], rows_per_chain) - np.float64(ent_coef)).astype(np.float32)
    g, norm = clip_grad(np.concatenate(parts + [dls, np.zeros(A, np.float32)]), A, max_grad_norm)
    count = np.float64(n)
    sums = {name: row_sums(R[name], rows_per_chain) for name in ("policy_loss", "value_loss", "kl", "clipped", "skipped")}
    stats = {"policy_loss": sums["policy_loss"] / count, "value_loss": sums["value_loss"] / count, "entropy": entropy(nets[2]),
             "approx_kl": sums["kl"] / count, "clip_fraction": sums["clipped"] / count, "skipped": sums["skipped"], "grad_norm": norm, "count": count}
    extra = {name: row_sums(R[name], rows_per_chain) for name in ("vf_clipped", "ret", "ret2", "diff", "diff2")}
    now, applied = gate(stopped, stats["approx_kl"], kl_limit) if float(kl_limit) > 0.0 else (False, True)
    more = {"vf_clip_fraction": extra["vf_clipped"] / count,
            "explained_variance": explained_variance(extra["ret"], extra["ret2"], extra["diff"], extra["diff2"], count - sums["skipped"]),
            "applied": np.float64(applied), "stopped": np.float64(now)}
    return {"grad": g, "stats": stats, "more": more, "rows": R, "logp_new": R["logp_new"], "value_new": R["value_new"], "ratio": R["ratio"]}


def shard_size(theta_size, n_axes):
    """L, the length of a shard's vector: theta's slots up to ``log_std``, then the ``SHARD_ROWS`` sums"""
    return int(theta_size) - 2 * int(n_axes) + len(SHARD_ROWS)


def shard_sums(theta, cells, n_axes, actor, critic, activation, obs, act, logp_old, adv, ret, count_total, clip=0.2, vf_coef=0.5,
               rows_per_chain=ROWS_PER_CHAIN, ratio=None, value_old=None, clip_vf=0.0):
    """a shard's vector, float64 [L]: what ``gradient`` computes of these rows up to, but not including, the narrowing, with every seed
    divided by ``(double)count_total``, the rows of the whole update.  ``combine(shard_sums(..., count_total=count)[None], ...)`` has the
    bits of ``gradient(...)``"""
    obs = np.asarray(obs)
    n = len(obs)
    check(n, rows_per_chain, clip)
    if int(count_total) < n:
        raise ValueError("count_total must be >= the shard's %d rows, not %r" % (n, count_total))
    A = int(n_axes)
    nets = unpack(theta, cells, A, actor, critic)
    with np.errstate(over="ignore", invalid="ignore"):
        x = obs.reshape(n, -1).astype(np.float32)
    bad = ~np.isfinite(x).all(axis=1)
    per_row_bad = bad | ~np.isfinite(np.asarray(act).astype(np.float64).reshape(n, A)).all(axis=1) | \
        ~np.isfinite(np.asarray(logp_old, dtype=np.float64).reshape(n)) | ~np.isfinite(np.asarray(adv, dtype=np.float64).reshape(n)) | \
        ~np.isfinite(np.asarray(ret, dtype=np.float64).reshape(n))
    if check_clip_vf(clip_vf, value_old) > 0.0:
        per_row_bad = per_row_bad | ~np.isfinite(np.asarray(value_old, dtype=np.float32).reshape(n))
    x = x.copy()
    x[per_row_bad] = 0.0
    a_in, mean = forward_keep(nets[0], x, activation)
    c_in, value = forward_keep(nets[1], x, activation)
    R = rows(mean, value[:, 0], nets[2], nets[3], act, logp_old, adv, ret, bad, clip, vf_coef, ratio, value_old, clip_vf, count_total)
    parts = []
    for net, inputs, seed in ((nets[0], a_in, R["dmean"]), (nets[1], c_in, R["dv"][:, None])):
        for dW, db in backward(net, inputs, seed, activation, rows_per_chain, wide=True):
            parts += [dW.reshape(-1), db]
    dls = np.zeros(8, dtype=np.float64)
    dls[:A] = row_sums(R["dls"], rows_per_chain)
    tail = np.array([row_sums(R[name], rows_per_chain) for name in SHARD_ROWS[8:]], dtype=np.float64)
    out = np.concatenate(parts + [dls, tail])
    assert out.size == shard_size(np.asarray(theta).size, A)
    return out


def combine(shards, theta, n_axes, count_total, ent_coef=0.0, max_grad_norm=0.5, stopped=False, kl_limit=0.0):
    """``(grad, stats, more)`` of W shards' vectors [W, L]: added in ascending shard order onto 0.0 in double, narrowed once, then the
    clipping, the statistics (``count = count_total``) and the gate of ``gradient``.  ``theta``: the parameters, for the entropy.
    ``combine(shard_sums(..., count_total=count)[None], ...)`` has the bits of ``gradient(...)``"""
    shards = np.asarray(shards, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float32).reshape(-1)
    A = int(n_axes)
    L = shard_size(theta.size, A)
    if shards.ndim != 2 or shards.shape[1] != L or not 1 <= len(shards) <= SHARDS_MAX:
        raise ValueError("shards must be [W, %d] with W in 1 .. %d, not %r" % (L, SHARDS_MAX, shards.shape))
    if int(count_total) < 1:
        raise ValueError("count_total must be >= 1")
    P = L - len(SHARD_ROWS)
    total = np.zeros(L, dtype=np.float64)
    with np.errstate(all="ignore"):
        for w in range(len(shards)):
            total = total + shards[w]
        dls = (total[P:P + A] - np.float64(ent_coef)).astype(np.float32)
        g, norm = clip_grad(np.concatenate([total[:P].astype(np.float32), dls, np.zeros(A, np.float32)]), A, max_grad_norm)
        count = np.float64(int(count_total))
        sums = dict(zip(SHARD_ROWS, total[P:]))
        stats = {"policy_loss": sums["policy_loss"] / count, "value_loss": sums["value_loss"] / count, "entropy": entropy(theta[P:P + A]),
                 "approx_kl": sums["kl"] / count, "clip_fraction": sums["clipped"] / count, "skipped": sums["skipped"], "grad_norm": norm, "count": count}
        now, applied = gate(stopped, stats["approx_kl"], kl_limit) if float(kl_limit) > 0.0 else (False, True)
        more = {"vf_clip_fraction": sums["vf_clipped"] / count,
                "explained_variance": explained_variance(sums["ret"], sums["ret2"], sums["diff"], sums["diff2"], count - sums["skipped"]),
                "applied": np.float64(applied), "stopped": np.float64(now)}
    return g, stats, more


def adam(theta, m, v, step, grad, n_axes, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, std=None):
    """one step: ``(theta', m', v', step + 1)``.  ``std``: the device's own exp(log_std') in place of numpy's"""
    A = int(n_axes)
    theta, m, v, g = (np.asarray(x, dtype=np.float32).reshape(-1).copy() for x in (theta, m, v, grad))
    step = int(step) + 1
    b1, b2 = float(betas[0]), float(betas[1])
    step_size, root = np.float64(float(lr) / (1.0 - b1 ** step)), np.float64(np.sqrt(1.0 - b2 ** step))
    p = theta.size - A      # (every slot but std's)
    gw, mw, vw, tw = (x[:p].astype(np.float64) for x in (g, m, v, theta))
    with np.errstate(all="ignore"):
        m[:p] = (np.float64(b1) * mw + np.float64(1.0 - b1) * gw).astype(np.float32)
        v[:p] = (np.float64(b2) * vw + np.float64(1.0 - b2) * (gw * gw)).astype(np.float32)
        m1, v1 = m[:p].astype(np.float64), v[:p].astype(np.float64)
        theta[:p] = (tw - step_size * (m1 / (np.sqrt(v1) / root + np.float64(eps)))).astype(np.float32)
        theta[p:] = np.exp(theta[p - A:p].astype(np.float64)).astype(np.float32) if std is None else np.asarray(std, dtype=np.float32)
    return theta, m, v, step
