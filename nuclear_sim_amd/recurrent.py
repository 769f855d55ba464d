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
front of slot 0 is in ``first`` already."""
import numpy as np

from . import policy
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
