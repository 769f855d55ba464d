"""The recurrent policy on the device, stated once in numpy: what ``env.set_policy(core=...)`` runs in front of every step
(npb_set_policy_core, nuclear_sim_amd/csrc/npb_policy_core.hip).  Host only.  This statement is the contract; everything it does not
restate is ``nuclear_sim_amd.policy``'s, whose functions it calls and whose bits it leaves alone.

THE CORE.  One GRU cell shared by actor and critic, hidden width H (1 .. 128).  Its input is the K * C feature cells, narrowed to float32
as ``policy`` narrows them; its state ``h`` is H float32 cells per plant.  Both MLPs read the NEW state ``h'`` in place of the features:
their first layers have ``in = H``; every other rule of ``policy.check`` stands.

THE PARAMETERS come in ``torch.nn.GRUCell``'s layout and gate order (r, z, n), as two layers of ``policy.layer``: ``W_ih[3H][K * C]``
with ``b_ih[3H]`` and ``W_hh[3H][H]`` with ``b_hh[3H]``.  In ``theta`` they come first:
``W_ih | b_ih | W_hh | b_hh | actor | critic | log_std | std``.  ``pack``, ``unpack`` and ``theta_size`` state it; without a core
``theta`` is ``policy``'s.

ONE STEP OF ONE PLANT (``cell``), all of it float32, every operation rounded on its own (no contraction):

    gi = layer(x, W_ih, b_ih)      gh = layer(h, W_hh, b_hh)      policy.layer's fmaf chains: bias first, k padded with +0.0 to a multiple of 4
    r[j] = S(gi[j] + gh[j])        z[j] = S(gi[H + j] + gh[H + j])
    n[j] = T(gi[2H + j] + r[j] * gh[2H + j])
    h'[j] = n[j] + z[j] * (h[j] - n[j])

THE GATES.  ``"hard"`` is bit-exact everywhere: ``y = 0.25f * a + 0.5f; S = y < 0 ? +0.0 : (y > 1 ? 1 : y)`` and
``T = a < -1 ? -1 : (a > 1 ? 1 : a)`` (a NaN passes through both).  ``"soft"``: ``T = tanh`` and ``S(a) = 0.5f * tanh(0.5f * a) + 0.5f``,
``tanh`` being ``policy``'s: the double tanh narrowed here, the device's float ``tanhf`` there.  The sigmoid goes through tanh so that the
float tanh stays the ONE licensed difference and its 5-ulp bound the only one needed.  An infinite or subnormal intermediate is outside
the contract, as in ``policy``.

RESTART.  In front of a step a plant's ``h`` is +0.0 in every cell where the plant is unprimed (fresh, or reset or restored by the caller)
or where its carried episode index differs from the one the policy saw last -- the rule by which the controls' hold restarts.  A step that
acts then remembers the index and primes the plant.  ``values`` applies the rule and remembers nothing.

POISON.  A plant with a non-finite feature gets THE quiet NaN in every output, as in ``policy``; its ``h'`` is +0.0: it does not poison its
own later steps, and touches no other plant.

The noise, the epilogue, ``logp``, the value and the extras slots are ``policy``'s, unchanged.

REPLAY (``replay``).  A rollout records ``obs``, ``episode`` and ``ended`` per slot and, with a core, ``first``: the ``h`` the policy read
in front of slot 0, the restart rule applied.  The states in front of every later slot follow: the plant restarts in front of slot t where
``episode[t] != episode[t - 1]`` (the autoreset's restarts, and the caller's under autoreset: both bump the index) or
``ended[t - 1] & NPB_ROLLOUT_CUT`` (the caller's reset / restore between two recorded steps, which the env marks in the slot before).
``npb_reset``, ``npb_restore``, ``npb_restore_bank`` and the episode kernel restart nothing these two columns do not show: a restart in
front of slot 0 is in ``first`` already.

TRAINING THROUGH TIME (``gradient``, ``shard_sums``; npb_policy_grad_seq, npb_policy_shard_sums_seq, nuclear_sim_amd/csrc/npb_ppo_seq.hip):
PPO's loss over whole sequences and its gradient through both nets, through the cell and through time.  Everything it does not restate is
``ppo``'s, whose functions it calls and whose bits it leaves alone.

THE INPUTS.  One sequence minibatch of ``t`` slots by ``count`` plants, time-major as ``rollout_minibatches(unit="plant")`` yields it:
``obs`` [t, count, K * C], ``act`` [t, count, A], ``logp_old``, ``adv``, ``ret`` and optionally ``value_old`` [t, count]; the restart words
``episode`` and ``ended`` [t, count] of the same plants; ``first`` [count, H], the state in front of slot 0.  The seeds' divisor is
``t * count``, or ``count_total`` for a shard.  ``first`` is the state the COLLECTING parameters produced: after the first update of an
iteration it is stale.  That is inherent, and what every recurrent PPO does.  Here a sequence is differentiated whole; TRUNCATED SEGMENTS,
below, cut it.

FORWARD.  ``replay``'s recurrence under the CURRENT theta: slot s reads ``h_s``, +0.0 where the plant restarted in front of s (``replay``'s
rule: an episode change, or ``ended[s - 1] & ROLLOUT_CUT``); ``advance`` gives ``h'_s`` and the poison flag; both nets run
``ppo.forward_keep`` over ``h'_s``.  ``cell_keep`` is ``cell`` with everything the backward pass reads.

PER CELL ``ppo.rows``, unchanged, ``bad`` the poison flag.  A cell whose features are finite and whose ``act``, ``logp_old``, ``adv``,
``ret`` or ``value_old`` is not is a skipped row as there: its seeds are +0.0, but the cell still runs and the carry still flows through
it.  A plant marked not ``valid`` (the device: an index outside the rollout's plants) is poisoned and skipped in every slot.

BACKWARD, s descending, all float32, every operation rounded on its own.  The nets as in ``ppo.backward``, and one ``back`` more, through
their first layers and without a derivative (``h'`` is an input, not an activation):

    dh' = (carry + back(delta_actor_layer0, W_actor0)) + back(delta_critic_layer0, W_critic0)            carry = +0.0 behind the last slot

On a poisoned cell ``dh'``, every gate delta and the outgoing carry are +0.0 (its ``h'`` was the constant +0.0).  Otherwise, ``u = h - n``:

    dn = dh' * (1.0f - z)        dz = dh' * u        direct = dh' * z
    dan  = dn * T'               soft: T' = 1.0f - n * n         hard: +0.0 where the forward took a clamped branch (a < -1 or a > 1), else dn
    dghn = dan * r               dr = dan * gh_n
    daz  = dz * S'(z)            soft: S' = s * (1.0f - s)       hard: +0.0 where y < 0 or y > 1 (the forward's own strict tests), else d * 0.25f
    dar  = dr * S'(r)            likewise
    delta_i = [dar | daz | dan]          delta_h = [dar | daz | dghn]          (3H wide, GRUCell's row order)
    carry_out = direct + back(delta_h, W_hh)

``back(delta_h, W_hh)`` is ONE fmaf chain over the 3H rows of ``W_hh`` ascending, from +0.0 (``ppo.back``).  ``carry_out`` is then +0.0
where the plant restarted in front of slot s.

THE SUMS.  A chain is ``plants_per_chain`` plants (a positive multiple of 32, default 32) with all their slots.  The row order within a
chain: tiles of 32 plants ascending, within a tile s DESCENDING, within a slot the plants ascending; ``ppo.chain_sums`` and
``ppo.row_sums`` are fed the rows in that order (``order``), the last chain extended with +0.0 rows, which change no bit.  ``dW_ih, db_ih``
come from ``(delta_i, x)`` and ``dW_hh, db_hh`` from ``(delta_h, h)``; the nets' as in ``ppo.backward``, their first layers reading
``h'``.  ``x`` of a poisoned cell reads +0.0.  Across chains ``ppo.across``.  The gradient comes out in theta's layout; clipping, the
statistics, the options and Adam are ``ppo``'s, unchanged.  THE INVARIANT: ``ppo.combine(shard_sums(..., count_total=t * count)[None],
...)`` has the bits of ``gradient(...)``.

TRUNCATED SEGMENTS (``starts``, ``segment_words``, ``gradient_segments``, ``shard_sums_segments``; npb_policy_core_segments,
npb_policy_grad_segments, npb_policy_segment_starts).  The t recorded slots are cut into ``chunks = t / every`` segments of ``every`` slots;
segment ``g = c * n + p`` is slots ``c * every .. c * every + every - 1`` of plant p.  While collecting, the policy records beside
``first`` the state it read in front of every slot ``c * every`` (``starts`` [chunks, n, H]; ``starts[0]`` is ``first``); that is
``replay(...)[::every]``.  A segment minibatch IS a sequence minibatch of length ``every`` whose plants are segments: its restart words are
the rollout's at the segment's own slots, the word in front of its first slot dropped (that restart is in ``starts`` already), and its
``first`` is ``starts.reshape(-1, H)[index]``.  The gradient stops at the segment's first slot: the carry out of it is dropped.
``gradient_segments`` and ``shard_sums_segments`` call ``gradient`` and ``shard_sums`` on exactly that and add no arithmetic of their
own.  A segment id outside ``0 .. chunks * n - 1`` is not ``valid``: poisoned and skipped in every slot.  After an update the stored
states are stale, as ``first`` is; the refresh recomputes ``starts(first, obs, ...)`` under the current parameters, row 0 left alone.
Ragged last segments (``t % every != 0``) are refused."""
import numpy as np

from . import policy, ppo
from .policy import fmaf, layer, activate, forward, noise, outputs      # noqa: F401  (the statement's pieces, for its readers)

CORE_MAX = 128
GATES = {"soft": 0, "hard": 1}
ROLLOUT_CUT = 4


def check(cells, n_axes, actor, critic, activation, core, gates="soft"):
    """refuse what npb_policy_check and npb_policy_core_check refuse of the shapes, by name"""
    policy.check(cells, n_axes, actor, critic, activation)
    if not 1 <= int(core) <= CORE_MAX:
        raise ValueError("the core is 1 to %d wide, not %r" % (CORE_MAX, core))
    if gates not in GATES:
        raise ValueError("the gates are 'soft' or 'hard', not %r" % (gates,))


def core_size(cells, core):
    H, KC = int(core), int(cells)
    return 3 * H * KC + 3 * H + 3 * H * H + 3 * H


def theta_size(cells, n_axes, actor, critic, core=None):
    if core is None:
        return policy.theta_size(cells, n_axes, actor, critic)
    return core_size(cells, core) + policy.theta_size(core, n_axes, actor, critic)


def pack(actor, critic, log_std, std=None, core=None):
    """``theta``; ``core``: ``(W_ih[3H][K * C], W_hh[3H][H], b_ih[3H], b_hh[3H])``, GRUCell's parameters in its own order"""
    rest = policy.pack(actor, critic, log_std, std)
    if core is None:
        return rest
    W_ih, W_hh, b_ih, b_hh = (np.asarray(v, dtype=np.float32) for v in core)
    H = W_hh.shape[-1]
    if W_ih.ndim != 2 or W_ih.shape[0] != 3 * H or W_hh.shape != (3 * H, H) or b_ih.shape != (3 * H,) or b_hh.shape != (3 * H,):
        raise ValueError("a core is W_ih[3H][cells], W_hh[3H][H], b_ih[3H], b_hh[3H]")
    if np.asarray(actor[0][0]).shape[1] != H:
        raise ValueError("both nets read the core's %d cells" % H)
    return np.concatenate([W_ih.reshape(-1), b_ih, W_hh.reshape(-1), b_hh, rest]).astype(np.float32)


def unpack(theta, cells, n_axes, actor, critic, core=None):
    """the inverse: ``(core, actor, critic, log_std, std)``, ``core`` as ``pack`` takes it (None without one)"""
    if core is None:
        return (None,) + tuple(policy.unpack(theta, cells, n_axes, actor, critic))
    theta = np.asarray(theta, dtype=np.float32).reshape(-1)
    if theta.size != theta_size(cells, n_axes, actor, critic, core):
        raise ValueError("theta has %d elements, these shapes take %d" % (theta.size, theta_size(cells, n_axes, actor, critic, core)))
    H, KC = int(core), int(cells)
    at = 0
    W_ih = theta[at:at + 3 * H * KC].reshape(3 * H, KC); at += 3 * H * KC
    b_ih = theta[at:at + 3 * H]; at += 3 * H
    W_hh = theta[at:at + 3 * H * H].reshape(3 * H, H); at += 3 * H * H
    b_hh = theta[at:at + 3 * H]; at += 3 * H
    return ((W_ih, W_hh, b_ih, b_hh),) + tuple(policy.unpack(theta[at:], H, n_axes, actor, critic))


def sigma(a, gates):
    """S of the statement, float32 elementwise"""
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if gates == "hard":
            y = (np.float32(0.25) * a).astype(np.float32) + np.float32(0.5)
            return np.where(y < 0, np.float32(0.0), np.where(y > 1, np.float32(1.0), y)).astype(np.float32)
        t = activate((np.float32(0.5) * a).astype(np.float32), "tanh")
        return ((np.float32(0.5) * t).astype(np.float32) + np.float32(0.5)).astype(np.float32)


def tau(a, gates):
    """T of the statement, float32 elementwise"""
    a = np.asarray(a, dtype=np.float32)
    if gates == "hard":
        with np.errstate(invalid="ignore"):
            return np.where(a < -1, np.float32(-1.0), np.where(a > 1, np.float32(1.0), a)).astype(np.float32)
    return activate(a, "tanh")


def cell(core, x, h, gates="soft"):
    """one step of the cell: float32 rows x [n, K * C] and h [n, H] -> h' [n, H]; no restart, no poison"""
    W_ih, W_hh, b_ih, b_hh = core
    x, h = np.asarray(x, dtype=np.float32), np.asarray(h, dtype=np.float32)
    H = h.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        gi, gh = layer(x, W_ih, b_ih), layer(h, W_hh, b_hh)
        r = sigma(gi[:, :H] + gh[:, :H], gates)
        z = sigma(gi[:, H:2 * H] + gh[:, H:2 * H], gates)
        n = tau(gi[:, 2 * H:] + (r * gh[:, 2 * H:]).astype(np.float32), gates)
        return (n + (z * (h - n).astype(np.float32)).astype(np.float32)).astype(np.float32)


def _rows(x):
    x = np.asarray(x)
    with np.errstate(over="ignore", invalid="ignore"):
        return x.reshape(len(x), -1).astype(np.float32)


def advance(core, x, h, gates="soft"):
    """``(h', bad)`` of feature rows x (any float type) and the states h in front of them: the cell and the poison rule"""
    x = _rows(x)
    bad = ~np.isfinite(x).all(axis=1)
    h2 = cell(core, x, h, gates)
    h2[bad] = np.float32(0.0)
    return h2, bad


def replay(first, obs, episode, ended, core, gates="soft"):
    """The hidden states in front of every recorded slot: float32 [T, n, H] of ``first`` [n, H] (the state in front of slot 0), the
    recorded ``obs`` [T, n, ...], ``episode`` [T, n] and ``ended`` [T, n], and the core's parameters as ``pack`` takes them.  Slot t's
    outputs are the nets' over ``advance(core, obs[t], replay[t])``."""
    obs, episode, ended = np.asarray(obs), np.asarray(episode), np.asarray(ended)
    T = len(obs)
    h = np.array(first, dtype=np.float32)
    out = np.zeros((T,) + h.shape, dtype=np.float32)
    for t in range(T):
        if t:
            restart = (episode[t] != episode[t - 1]) | ((ended[t - 1] & ROLLOUT_CUT) != 0)
            h[restart] = np.float32(0.0)
        out[t] = h
        h, _ = advance(core, obs[t], h, gates)
    return out


class Policy(policy.Policy):
    """What the device keeps with a core: ``policy.Policy``'s, and per plant ``h`` [n, H], ``primed`` and ``seen``.  ``step(x, episode)``
    is one step's launch; ``values(x, hidden=)`` is npb_policy_values_hidden."""

    def __init__(self, cells, n_axes, actor, critic, activation="tanh", seed=0, deterministic=False, first_plant=0, act_dtype=np.float32,
                 core=None, gates="soft", n=None):
        if core is None or n is None:
            raise ValueError("a recurrent Policy takes core= (its width) and n= (the plants)")
        check(cells, n_axes, actor, critic, activation, core, gates)
        policy.Policy.__init__(self, cells, n_axes, actor, critic, activation, seed, deterministic, first_plant, act_dtype)
        self.core, self.gates, self.n = int(core), gates, int(n)
        self.h = np.zeros((self.n, self.core), dtype=np.float32)
        self.primed, self.seen = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.int32)

    def load(self, theta):
        self.theta = np.array(theta, dtype=np.float32).reshape(-1)
        parts = unpack(self.theta, self.cells, self.n_axes, self.actor, self.critic, self.core)
        self.gru, self.nets = parts[0], parts[1:]

    def unprime(self, mask=None):
        """what a reset or restore of the caller's does to the masked plants (None = all)"""
        self.primed[slice(None) if mask is None else np.asarray(mask, dtype=bool)] = 0

    def started(self, episode=None, h=None):
        """the states in front of a step, the restart rule applied to ``h`` (None: the policy's own)"""
        episode = self.seen if episode is None else np.asarray(episode, dtype=np.int32)
        h = np.array(self.h if h is None else h, dtype=np.float32)
        h[(self.primed == 0) | (episode != self.seen)] = np.float32(0.0)
        return h

    def values(self, x, hidden=None, episode=None):
        """the critic over GRU(x, hidden); ``hidden`` None: the policy's own states under the restart rule (x: every plant's features)"""
        h = self.started(episode) if hidden is None else np.asarray(hidden, dtype=np.float32)
        h2, bad = advance(self.gru, x, h, self.gates)
        v = forward(self.nets[1], h2, self.activation)[:, 0].copy()
        v[bad] = np.nan
        return v

    def step(self, x, episode=None, z=None, h=None):
        """one step; ``episode``: the carried episode indices (None: no autoreset, nothing carried); ``z`` / ``h`` given: the device's own
        draw / hidden state in place of the statement's (what the tests feed back)"""
        start = self.started(episode, h)
        self.last_start = start
        h2, _ = advance(self.gru, x, start, self.gates)
        self.h = h2
        self.primed[:] = 1
        if episode is not None:
            self.seen = np.array(episode, dtype=np.int32)
        actor, critic, log_std, std = self.nets
        if self.deterministic:
            z = np.zeros((len(h2), self.n_axes))
        else:
            if z is None:
                z = noise(self.seed, self.t, len(h2), self.n_axes, self.first_plant)
            self.t += 1
        return outputs(forward(actor, h2, self.activation), forward(critic, h2, self.activation)[:, 0], log_std, std, z, _rows(x), self.act_dtype)


# ---------------------------------------------------------------------------------------------------------------- training through time

PLANTS_PER_CHAIN = 32


def cell_keep(core, x, h, gates="soft"):
    """``cell`` with what it computed on the way: a dict of ``h2`` (``cell``'s own bits), ``gi``, ``gh`` [n, 3H], ``r``, ``z``, ``n`` and
    the three pre-activations ``ar``, ``az``, ``an`` [n, H]"""
    W_ih, W_hh, b_ih, b_hh = core
    x, h = np.asarray(x, dtype=np.float32), np.asarray(h, dtype=np.float32)
    H = h.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        gi, gh = layer(x, W_ih, b_ih), layer(h, W_hh, b_hh)
        ar = (gi[:, :H] + gh[:, :H]).astype(np.float32)
        az = (gi[:, H:2 * H] + gh[:, H:2 * H]).astype(np.float32)
        r, z = sigma(ar, gates), sigma(az, gates)
        an = (gi[:, 2 * H:] + (r * gh[:, 2 * H:]).astype(np.float32)).astype(np.float32)
        n = tau(an, gates)
        h2 = (n + (z * (h - n).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return {"h2": h2, "gi": gi, "gh": gh, "r": r, "z": z, "n": n, "ar": ar, "az": az, "an": an}


def sigma_slope(d, a, s, gates):
    """``d * S'``: float32 elementwise, of the pre-activation a and S(a) = s"""
    one = np.float32(1.0)
    if gates == "hard":
        y = (np.float32(0.25) * a).astype(np.float32) + np.float32(0.5)
        return np.where((y < 0) | (y > 1), np.float32(0.0), (d * np.float32(0.25)).astype(np.float32)).astype(np.float32)
    return (d * (s * (one - s).astype(np.float32)).astype(np.float32)).astype(np.float32)


def tau_slope(d, a, n, gates):
    """``d * T'``"""
    if gates == "hard":
        return np.where((a < -1) | (a > 1), np.float32(0.0), d).astype(np.float32)
    return (d * (np.float32(1.0) - (n * n).astype(np.float32)).astype(np.float32)).astype(np.float32)


def cell_back(core, K, dh2, h, bad, gates="soft"):
    """one cell backwards: ``(delta_i, delta_h, carry_out)`` of ``dh2`` = dh', what ``cell_keep`` kept (K) and the states h it read; the
    restart in front of the slot is the caller's"""
    W_hh = core[1]
    one = np.float32(1.0)
    bad = np.asarray(bad, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        dh2 = np.where(bad[:, None], np.float32(0.0), dh2).astype(np.float32)
        r, z, n, H = K["r"], K["z"], K["n"], h.shape[1]
        ghn = K["gh"][:, 2 * H:]
        u = (h - n).astype(np.float32)
        dn, dz, direct = (dh2 * (one - z).astype(np.float32)).astype(np.float32), (dh2 * u).astype(np.float32), (dh2 * z).astype(np.float32)
        dan = tau_slope(dn, K["an"], n, gates)
        dghn, dr = (dan * r).astype(np.float32), (dan * ghn).astype(np.float32)
        daz, dar = sigma_slope(dz, K["az"], z, gates), sigma_slope(dr, K["ar"], r, gates)
        parts = [np.where(bad[:, None], np.float32(0.0), v).astype(np.float32) for v in (dar, daz, dan, dghn, direct)]
        dar, daz, dan, dghn, direct = parts
        delta_i, delta_h = np.concatenate([dar, daz, dan], axis=1), np.concatenate([dar, daz, dghn], axis=1)
        carry = (direct + ppo.back(delta_h, W_hh)).astype(np.float32)
    return delta_i, delta_h, carry


def restarts(episode, ended):
    """bool [t, count]: the plant restarted in front of slot s (``replay``'s rule; False at s = 0: that restart is in ``first``)"""
    episode, ended = np.asarray(episode), np.asarray(ended)
    out = np.zeros(episode.shape, dtype=bool)
    out[1:] = (episode[1:] != episode[:-1]) | ((ended[:-1] & ROLLOUT_CUT) != 0)
    return out


def order(t, count, plants_per_chain=PLANTS_PER_CHAIN):
    """``(rows, rows_per_chain)``: the flat cells ``s * count + p`` in the sums' order -- per chain of ``plants_per_chain`` plants the tiles
    of 32 plants ascending, within a tile s descending, within a slot the plants ascending -- every chain extended with -1 (a +0.0 row) to
    ``rows_per_chain = t * plants_per_chain`` rows"""
    t, count, ppc = int(t), int(count), int(plants_per_chain)
    if ppc < ppo.TILE or ppc % ppo.TILE:
        raise ValueError("plants_per_chain must be a positive multiple of 32, not %r" % (plants_per_chain,))
    rows = []
    for c0 in range(0, count, ppc):
        chain = [s * count + p for p0 in range(c0, min(c0 + ppc, count), ppo.TILE) for s in range(t - 1, -1, -1) for p in range(p0, min(p0 + ppo.TILE, c0 + ppc, count))]
        rows += chain + [-1] * (t * ppc - len(chain))
    return np.asarray(rows, dtype=np.int64), t * ppc


def _ordered(x, rows):
    """x [cells, ...] in the sums' order, a row of +0.0 where rows is -1"""
    x = np.asarray(x)
    return np.concatenate([x, np.zeros((1,) + x.shape[1:], x.dtype)])[rows]


def _sweep(theta, cells, n_axes, actor, critic, activation, core, gates, obs, act, logp_old, adv, ret, episode, ended, first, clip, vf_coef,
           plants_per_chain, ratio, value_old, clip_vf, count_total, valid, wide):
    """what ``gradient`` and ``shard_sums`` share: ``(parts, R, rows, rpc, nets, hidden, gate deltas)`` -- the weights' and biases' sums in
    theta's order (float32, or the float64 sums as they are with ``wide``), ``ppo.rows``'s dict over the t * count cells (time-major), the
    sums' order, the states h' [t, count, H], and ``(delta_i, delta_h)`` [t, count, 3H]"""
    obs = np.asarray(obs)
    t, count = obs.shape[:2]
    N, A, H = t * count, int(n_axes), int(core)
    ppo.check(N, ppo.TILE, clip)
    rows, rpc = order(t, count, plants_per_chain)
    gru, a_net, c_net, log_std, std = unpack(theta, cells, A, actor, critic, H)
    with np.errstate(over="ignore", invalid="ignore"):
        x = obs.reshape(t, count, -1).astype(np.float32)
    valid = np.ones(count, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    fresh = restarts(np.asarray(episode).reshape(t, count), np.asarray(ended).reshape(t, count))
    # forward, s ascending
    h = np.where(valid[:, None], np.asarray(first, dtype=np.float32).reshape(count, H), np.float32(0.0)).astype(np.float32)
    hs, h2s, bads, keeps = [], [], [], []
    for s in range(t):
        h = h.copy()
        h[fresh[s]] = np.float32(0.0)
        bad = ~np.isfinite(x[s]).all(axis=1) | ~valid
        xs = x[s].copy()
        xs[bad] = np.float32(0.0)
        K = cell_keep(gru, xs, h, gates)
        h2 = K["h2"].copy()
        h2[bad] = np.float32(0.0)
        hs.append(h); h2s.append(h2); bads.append(bad); keeps.append((xs, K))
        h = h2
    hidden, bad_all = np.stack(h2s), np.stack(bads).reshape(N)
    flat = hidden.reshape(N, H)
    a_in, mean = ppo.forward_keep(a_net, flat, activation)
    c_in, value = ppo.forward_keep(c_net, flat, activation)
    R = ppo.rows(mean, value[:, 0], log_std, std, np.asarray(act).reshape(N, A), np.asarray(logp_old).reshape(N), np.asarray(adv).reshape(N),
                 np.asarray(ret).reshape(N), bad_all, clip, vf_coef, None if ratio is None else np.asarray(ratio).reshape(N),
                 None if value_old is None else np.asarray(value_old).reshape(N), clip_vf, N if count_total is None else count_total)
    # the nets backward over every cell at once (a row's deltas depend on that row alone), keeping every layer's delta
    deltas = []
    for net, inputs, seed in ((a_net, a_in, R["dmean"]), (c_net, c_in, R["dv"][:, None])):
        delta, per = np.asarray(seed, dtype=np.float32), [None] * len(net)
        for l in range(len(net) - 1, -1, -1):
            per[l] = delta
            delta = ppo.back(delta, net[l][0])
            if l:
                delta = ppo.through(delta, inputs[l], activation)
        deltas.append((per, delta.reshape(t, count, H)))      # (the last one: back through layer 0, no derivative)
    # the cell backward through time, s descending
    carry = np.zeros((count, H), dtype=np.float32)
    d_i, d_h = np.zeros((t, count, 3 * H), np.float32), np.zeros((t, count, 3 * H), np.float32)
    for s in range(t - 1, -1, -1):
        dh2 = ((carry + deltas[0][1][s]).astype(np.float32) + deltas[1][1][s]).astype(np.float32)
        d_i[s], d_h[s], carry = cell_back(gru, keeps[s][1], dh2, hs[s], bads[s], gates)
        carry[fresh[s]] = np.float32(0.0)
    # the sums, in the chains' order
    def sums(delta, inputs):
        dW, db = ppo.chain_sums(_ordered(delta, rows), _ordered(inputs, rows), rpc)
        dW, db = ppo.across(dW), ppo.across(db)
        return [dW.reshape(-1), db] if wide else [dW.astype(np.float32).reshape(-1), db.astype(np.float32)]
    xs_all, h_all = np.stack([k[0] for k in keeps]).reshape(N, -1), np.stack(hs).reshape(N, H)
    (dW_ih, db_ih), (dW_hh, db_hh) = sums(d_i.reshape(N, -1), xs_all), sums(d_h.reshape(N, -1), h_all)
    parts = [dW_ih, db_ih, dW_hh, db_hh]
    for (per, _), inputs in zip(deltas, (a_in, c_in)):
        for l in range(len(per)):
            parts += sums(per[l], inputs[l])
    return parts, R, rows, rpc, (log_std, std), hidden, (d_i, d_h)


def gradient(theta, cells, n_axes, actor, critic, activation, core, gates, obs, act, logp_old, adv, ret, episode, ended, first, clip=0.2,
             vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5, plants_per_chain=PLANTS_PER_CHAIN, ratio=None, value_old=None, clip_vf=0.0,
             stopped=False, kl_limit=0.0, valid=None, keep=False):
    """``{"grad", "stats", "more", "rows", "logp_new", "value_new", "ratio", "hidden"}`` of one sequence minibatch: what ``ppo.gradient``
    returns, grad in theta's layout with the core in front; ``logp_new``, ``value_new``, ``ratio`` [t, count]; ``hidden`` [t, count, H]
    the states h' under the current theta.  ``ratio``: the device's own values back, as ``ppo.gradient`` takes them.  ``keep``: also ``delta_i`` and ``delta_h``
    [t, count, 3H], every cell's gate deltas"""
    parts, R, rows, rpc, (log_std, _), hidden, gates_d = _sweep(theta, cells, n_axes, actor, critic, activation, core, gates, obs, act, logp_old, adv, ret,
                                                       episode, ended, first, clip, vf_coef, plants_per_chain, ratio, value_old, clip_vf, None, valid, False)
    t, count = hidden.shape[:2]
    A = int(n_axes)

    def total(name):
        return ppo.row_sums(_ordered(R[name], rows), rpc)
    dls = (total("dls") - np.float64(ent_coef)).astype(np.float32)
    g, norm = ppo.clip_grad(np.concatenate(parts + [dls, np.zeros(A, np.float32)]), A, max_grad_norm)
    n = np.float64(t * count)
    sums = {name: total(name) for name in ("policy_loss", "value_loss", "kl", "clipped", "skipped", "vf_clipped", "ret", "ret2", "diff", "diff2")}
    stats = {"policy_loss": sums["policy_loss"] / n, "value_loss": sums["value_loss"] / n, "entropy": ppo.entropy(log_std),
             "approx_kl": sums["kl"] / n, "clip_fraction": sums["clipped"] / n, "skipped": sums["skipped"], "grad_norm": norm, "count": n}
    now, applied = ppo.gate(stopped, stats["approx_kl"], kl_limit) if float(kl_limit) > 0.0 else (False, True)
    more = {"vf_clip_fraction": sums["vf_clipped"] / n,
            "explained_variance": ppo.explained_variance(sums["ret"], sums["ret2"], sums["diff"], sums["diff2"], n - sums["skipped"]),
            "applied": np.float64(applied), "stopped": np.float64(now)}
    out = {"grad": g, "stats": stats, "more": more, "rows": R, "logp_new": R["logp_new"].reshape(t, count), "value_new": R["value_new"].reshape(t, count),
           "ratio": R["ratio"].reshape(t, count), "hidden": hidden}
    if keep:
        out["delta_i"], out["delta_h"] = gates_d
    return out


def shard_sums(theta, cells, n_axes, actor, critic, activation, core, gates, obs, act, logp_old, adv, ret, episode, ended, first, count_total,
               clip=0.2, vf_coef=0.5, plants_per_chain=PLANTS_PER_CHAIN, ratio=None, value_old=None, clip_vf=0.0, valid=None):
    """a shard's vector, float64 [``ppo.shard_size``]: ``gradient``'s sums up to, but not including, the narrowing, every seed divided by
    ``(double)count_total``, the cells of the whole update (``ppo.shard_sums`` says what for)"""
    obs = np.asarray(obs)
    if int(count_total) < obs.shape[0] * obs.shape[1]:
        raise ValueError("count_total must be >= the shard's %d cells, not %r" % (obs.shape[0] * obs.shape[1], count_total))
    parts, R, rows, rpc, _, _, _ = _sweep(theta, cells, n_axes, actor, critic, activation, core, gates, obs, act, logp_old, adv, ret, episode, ended, first,
                                       clip, vf_coef, plants_per_chain, ratio, value_old, clip_vf, count_total, valid, True)
    dls = np.zeros(8, dtype=np.float64)
    dls[:int(n_axes)] = ppo.row_sums(_ordered(R["dls"], rows), rpc)
    tail = np.array([ppo.row_sums(_ordered(R[name], rows), rpc) for name in ppo.SHARD_ROWS[8:]], dtype=np.float64)
    out = np.concatenate(parts + [dls, tail])
    assert out.size == ppo.shard_size(np.asarray(theta).size, n_axes)
    return out


# ---------------------------------------------------------------------------------------------------------------- truncated segments

def chunks_of(t, every):
    """``t / every``, the segments a plant's t recorded slots are cut into; a ragged last segment is refused"""
    t, L = int(t), int(every)
    if L < 1 or L > t:
        raise ValueError("every must be 1 .. the recorded slots %d, not %r" % (t, every))
    if t % L:
        raise ValueError("the recorded slots %d are not a multiple of every = %d: ragged last segments are not supported" % (t, L))
    return t // L


def starts(first, obs, episode, ended, core, gates, every):
    """The stored states, float32 [chunks, n, H]: the state in front of every slot ``c * every``, the restart rule applied --
    ``replay(...)[::every]``.  Row 0 is ``first``.  What the device records while collecting (npb_policy_core_segments) and what the
    refresh recomputes under the current parameters (npb_policy_segment_starts)"""
    chunks_of(len(np.asarray(obs)), every)
    return replay(first, obs, episode, ended, core, gates)[::int(every)]


def segment_words(episode, ended, index, n, every):
    """``(episode [L, count], ended [L, count], valid [count])`` of the segments ``index`` (ids ``c * n + p``; None: every segment in
    order) of a rollout's ``episode`` and ``ended`` [t, n]: segment g's words are rows ``c * L .. c * L + L - 1`` of column p.  An id
    outside ``0 .. (t / L) * n - 1`` is not valid, and nothing is read through it (its words are zeros)"""
    episode, ended = np.asarray(episode), np.asarray(ended)
    n, L = int(n), int(every)
    chunks = chunks_of(len(episode), L)
    g = np.arange(chunks * n, dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64).reshape(-1)
    valid = (g >= 0) & (g < chunks * n)
    safe = np.where(valid, g, 0)
    slots = (safe // n)[None, :] * L + np.arange(L)[:, None]
    cols = (safe % n)[None, :]
    return (np.where(valid[None, :], episode[slots, cols], 0).astype(episode.dtype), np.where(valid[None, :], ended[slots, cols], 0).astype(ended.dtype), valid)


def _segments(episode, ended, starts, index, n, every, valid):
    starts = np.asarray(starts, dtype=np.float32)
    H = starts.shape[-1]
    ep, en, ok = segment_words(episode, ended, index, n, every)
    rows = starts.reshape(-1, H)
    if len(rows) < chunks_of(len(np.asarray(episode)), every) * int(n):
        raise ValueError("starts has %d rows, the rollout's segments are %d" % (len(rows), chunks_of(len(np.asarray(episode)), every) * int(n)))
    g = np.arange(len(ok), dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64).reshape(-1)
    first = rows[np.where(ok, g, 0)]
    return ep, en, first, ok if valid is None else ok & np.asarray(valid, dtype=bool)


def gradient_segments(theta, cells, n_axes, actor, critic, activation, core, gates, obs, act, logp_old, adv, ret, episode, ended, starts, index, n,
                      every, valid=None, **options):
    """``gradient`` over a segment minibatch: ``obs`` [every, count, K * C] and the other tensors as
    ``rollout.minibatch(unit="segment", every=every)`` gathers them, ``index`` [count] its segment ids (None: every segment in order),
    ``episode`` and ``ended`` the ROLLOUT's [t, n], ``starts`` [chunks, n, H].  ``plants_per_chain`` counts segments.  No arithmetic of
    its own: ``gradient(..., *segment_words(...), starts.reshape(-1, H)[index], valid=...)``"""
    ep, en, first, ok = _segments(episode, ended, starts, index, n, every, valid)
    return gradient(theta, cells, n_axes, actor, critic, activation, core, gates, obs, act, logp_old, adv, ret, ep, en, first, valid=ok, **options)


def shard_sums_segments(theta, cells, n_axes, actor, critic, activation, core, gates, obs, act, logp_old, adv, ret, episode, ended, starts, index, n,
                        every, count_total, valid=None, **options):
    """``shard_sums`` over a segment minibatch, as ``gradient_segments`` is ``gradient``; ``count_total`` counts cells"""
    ep, en, first, ok = _segments(episode, ended, starts, index, n, every, valid)
    return shard_sums(theta, cells, n_axes, actor, critic, activation, core, gates, obs, act, logp_old, adv, ret, ep, en, first, count_total, valid=ok,
                      **options)
