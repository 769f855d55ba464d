"""The rollout (npb_set_rollout, include/npb.h) stated in numpy: what the device records per step, and the GAE recurrence over it.

``Recorder`` builds, from per-step inputs, the arrays ``BatchedPlantEnv.rollout()`` returns: time-major, slot t first.  ``pre`` is what the
pre kernel copies in front of step t, ``post`` what the post kernel writes behind features pass A and in front of the episode kernel, ``cut``
a restart the caller makes between two recorded steps.  The outcome of a transition is the episode kernel's rule: termination wins over
truncation, and a truncation is due when the carried length reaches ``max_episode_steps``.

``advantages`` is the recurrence in float64, step by step, every operation rounded on its own; the device produces its bits.  It is the
contract: no scan, no vectorisation along t."""
import numpy as np

HORIZON_MAX, EXTRAS_MAX = 4096, 8
TERMINATED, TRUNCATED, CUT = 1, 2, 4


def final_rows_bound(horizon: int, max_episode_steps) -> int:
    """The rows of ``final_obs`` a plant can need: truncations of one plant are at least ``max_episode_steps`` steps apart and the first
    can fall on slot 0, so ceil(horizon / max_episode_steps); 0 where no truncation can happen"""
    m = int(max_episode_steps or 0)
    return 0 if m <= 0 else -(-int(horizon) // m)


class Recorder:
    """``Recorder(horizon, n, stack=(K, C))``: ``obs`` [T, n, K, C], ``act`` [T, n, A] (None with ``axes`` 0), ``extra`` [T, n, E] float32,
    ``reward`` [T, n] float64, ``ended`` [T, n] uint8, ``episode`` [T, n] int32, ``final_row`` [T, n] int32, ``final_obs`` [n * R, K, C],
    the cursor ``t`` and ``n_final`` [n].  ``autoreset`` False: only bit 0 of ``ended`` can be set and ``episode`` is -1."""

    def __init__(self, horizon, n, stack, axes=0, extras=0, final_rows=0, autoreset=False, max_episode_steps=0, obs_dtype=np.float32,
                 act_dtype=np.float32):
        if not 1 <= horizon <= HORIZON_MAX:
            raise ValueError("the horizon must be 1 .. %d, not %r" % (HORIZON_MAX, horizon))
        if not 0 <= extras <= EXTRAS_MAX:
            raise ValueError("the extras count must be 0 .. %d, not %r" % (EXTRAS_MAX, extras))
        if final_rows < 0:
            raise ValueError("final_rows must be >= 0")
        K, C = stack
        self.T, self.n, self.R = int(horizon), int(n), int(final_rows)
        self.autoreset, self.max_steps = bool(autoreset), int(max_episode_steps or 0) if autoreset else 0
        if self.R < final_rows_bound(self.T, self.max_steps):
            raise ValueError("final_rows %d is below ceil(horizon / max_episode_steps) = %d" % (self.R, final_rows_bound(self.T, self.max_steps)))
        self.obs = np.zeros((self.T, self.n, K, C), dtype=obs_dtype)
        self.act = np.zeros((self.T, self.n, axes), dtype=act_dtype) if axes else None
        self.extra = np.zeros((self.T, self.n, extras), dtype=np.float32)
        self.reward = np.zeros((self.T, self.n), dtype=np.float64)
        self.ended = np.zeros((self.T, self.n), dtype=np.uint8)
        self.episode = np.zeros((self.T, self.n), dtype=np.int32)
        self.final_row = np.zeros((self.T, self.n), dtype=np.int32)
        self.final_obs = np.zeros((self.n * self.R, K, C), dtype=obs_dtype)
        self.length = np.zeros(self.n, dtype=np.int64)      # the carried length of every plant's running episode
        self.begin()

    def begin(self) -> None:
        """t = 0, no row of ``final_obs`` taken, ``final_row`` -1 everywhere (the carried lengths go on)"""
        self.t = 0
        self.n_final = np.zeros(self.n, dtype=np.int32)
        self.final_row[:] = -1

    def pre(self, features, act=None, extra=None) -> None:
        """in front of step t: the features tensor as the policy saw it, the controls input as it wrote it, its extras"""
        if self.t >= self.T:
            raise ValueError("the rollout is full: begin() rewinds it")
        self.obs[self.t] = features
        if self.act is not None:
            self.act[self.t] = act
        if self.extra.shape[2]:
            self.extra[self.t] = extra

    def post(self, reward, done, stack, episode=None) -> np.ndarray:
        """behind step t: its reward and done columns, the features tensor with this step's frame appended (``stack``, [n, K, C]) and the
        carried episode indices of the episodes the transitions belonged to.  Returns the slot's ``ended`` bits; t += 1"""
        t = self.t
        terminated = np.asarray(done) != 0
        truncated = np.zeros(self.n, dtype=bool)
        if self.autoreset:
            if self.max_steps > 0:
                truncated = (self.length + 1 >= self.max_steps) & ~terminated      # termination wins
            over = terminated | truncated
            self.length = np.where(over, 0, self.length + 1)
        self.reward[t] = reward
        self.ended[t] = terminated * TERMINATED + truncated * TRUNCATED
        self.episode[t] = episode if self.autoreset and episode is not None else -1
        for p in np.flatnonzero(truncated):
            if self.n_final[p] < self.R:
                row = p * self.R + self.n_final[p]
                self.n_final[p] += 1
                self.final_row[t, p] = row
                self.final_obs[row] = np.asarray(stack)[p]
        self.t = t + 1
        return self.ended[t]

    def cut(self, mask=None) -> None:
        """a restart the caller made between two recorded steps: bit 2 into the masked plants' (None = all) previous slot, nothing in front
        of slot 0; their carried length starts again"""
        m = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask) != 0
        self.length = np.where(m, 0, self.length)
        if self.t > 0:
            self.ended[self.t - 1] |= (m * CUT).astype(np.uint8)

    def arrays(self) -> dict:
        return {"obs": self.obs, "act": self.act, "extra": self.extra, "reward": self.reward, "ended": self.ended, "episode": self.episode,
                "final_row": self.final_row, "final_obs": self.final_obs, "t": self.t}


def advantages(reward, ended, final_row, values=None, last_value=None, final_values=None, gamma=0.99, lam=0.95, dtype=np.float32):
    """GAE over the slots ``reward`` holds ([t, n] float64; pass the recorded prefix): returns ``(adv, ret)``, [t, n] of ``dtype``.
    ``values`` [t, n], ``last_value`` [n] and ``final_values`` [n * R] are float32 (None = 0.0 everywhere); a truncated slot bootstraps
    from ``final_values[final_row]`` -- the value of the TERMINAL state -- a terminated or cut one from 0.  The carry is a select: a NaN
    in one episode never reaches the one in front of it."""
    if not (0.0 <= gamma <= 1.0 and 0.0 <= lam <= 1.0):
        raise ValueError("gamma and lam must lie in [0, 1]")
    reward = np.asarray(reward, dtype=np.float64)
    ended, final_row = np.asarray(ended), np.asarray(final_row)
    T, n = reward.shape
    if T == 0:
        raise ValueError("nothing recorded (t == 0)")
    gamma = np.float64(gamma)
    gl = gamma * np.float64(lam)
    zero = np.zeros(n, dtype=np.float64)
    wide = (lambda x: zero if x is None else np.asarray(x, dtype=np.float32).astype(np.float64))
    fin = None if final_values is None else np.asarray(final_values, dtype=np.float32).astype(np.float64)
    adv, ret = np.zeros((T, n), dtype=np.float64), np.zeros((T, n), dtype=np.float64)
    a_next = zero
    for t in range(T - 1, -1, -1):
        e = ended[t]
        v = zero if values is None else wide(values[t])
        behind = wide(last_value) if t == T - 1 else (zero if values is None else wide(values[t + 1]))
        row = final_row[t]
        have = (row >= 0) & (fin is not None)
        final = np.where(have, fin[np.where(have, row, 0)], 0.0) if fin is not None and fin.size else zero
        nv = np.where((e & (TERMINATED | CUT)) != 0, 0.0, np.where((e & TRUNCATED) != 0, final, behind))
        delta = (reward[t] + gamma * nv) - v
        carry = np.where((e & 7) != 0, 0.0, a_next)
        a = delta + gl * carry
        adv[t], ret[t] = a, a + v
        a_next = a
    with np.errstate(over="ignore"):
        return adv.astype(dtype), ret.astype(dtype)
