"""The rollout (npb_set_rollout, include/npb.h) stated in numpy: what the device records per step, and the GAE recurrence over it.

``Recorder`` builds, from per-step inputs, the arrays ``BatchedPlantEnv.rollout()`` returns: time-major, slot t first.  ``pre`` is what the
pre kernel copies in front of step t, ``post`` what the post kernel writes behind features pass A and in front of the episode kernel, ``cut``
a restart the caller makes between two recorded steps.  The outcome of a transition is the episode kernel's rule: termination wins over
truncation, and a truncation is due when the carried length reaches ``max_episode_steps``.

``advantages`` is the recurrence in float64, step by step, every operation rounded on its own; the device produces its bits.  It is the
contract: no scan, no vectorisation along t.

``moments``, ``permutation_keys``, ``permutation`` and ``minibatch`` state what happens between the advantages and the optimiser
(npb_rollout_moments, npb_rollout_permutation, npb_rollout_minibatch): the order of every addition of the moments is pinned, the shuffled
order is a function of (seed, epoch, position) alone, and the device produces their bits too.  ``moments_part``, ``moments_combine`` and
``moments_shards`` cut the moments where the pinned sums end, so that W shards form ONE mean and ONE spread (npb_rollout_moments_part,
npb_rollout_moments_combine)."""
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


# ------------------------------------------------------------------------------------------------ between advantages() and the optimiser
# What a PPO-style learner does with a finished rollout (npb_rollout_moments, npb_rollout_permutation, npb_rollout_minibatch): the
# advantages' mean and standard deviation with the order of every addition pinned, a shuffled order that is a function of (seed, epoch, i)
# alone -- no table, no sort --, and the gather of one minibatch.  The device produces these bits.
TREE_WIDTH = 256      # the pairwise tree's fan-in: one workgroup
ROUNDS = 6            # the Feistel network's rounds, one uint32 key each
N_MAX = 2 ** 31 - 1   # entries a permutation can have: an index is an int32
UNITS = {"transition": 0, "plant": 1, "segment": 2}      # NPB_MINIBATCH_TRANSITION / NPB_MINIBATCH_PLANT / NPB_MINIBATCH_SEGMENT


def _tree(c: np.ndarray) -> np.float64:
    """the pinned sum of a float64 vector: groups of 256 padded with +0.0, in each the halves 128, 64, ... 1 added onto each other, the
    groups' results the next level's vector, until one value is left; a vector of one value is that value"""
    c = np.asarray(c, dtype=np.float64)
    while c.size > 1:
        g = -(-c.size // TREE_WIDTH)
        padded = np.zeros(g * TREE_WIDTH, dtype=np.float64)
        padded[:c.size] = c
        c = padded.reshape(g, TREE_WIDTH)
        half = TREE_WIDTH // 2
        while half >= 1:
            c = c[:, :half] + c[:, half:2 * half]
            half //= 2
        c = c[:, 0]
    return np.float64(c[0])


def moments(x, ddof=1):
    """``(count, mean, var, std)`` of ``x`` [rows, cols] (float32 or float64) as float64, the order of every addition pinned: a column's
    rows are added in order into a double that starts at 0.0, the columns' sums go through ``_tree``; mean = that / count; a second pass
    adds the rounded squares of ``(double)x - mean`` the same way, var = that / (count - ddof), std = sqrt(var).  Division and root are
    IEEE, a NaN or an infinity propagates.  This is the contract: it is not restated as np.sum, whose order is numpy's own."""
    x = np.asarray(x)
    if x.ndim != 2 or x.dtype not in (np.float32, np.float64):
        raise ValueError("moments are taken of a [rows, cols] float32 or float64 array")
    rows, cols = x.shape
    count, ddof = rows * cols, int(ddof)
    if ddof < 0 or count <= ddof:
        raise ValueError("rows * cols = %d must exceed ddof = %d" % (count, ddof))
    with np.errstate(invalid="ignore", over="ignore"):
        col = np.zeros(cols, dtype=np.float64)
        for s in range(rows):
            col += x[s].astype(np.float64)
        mean = _tree(col) / np.float64(count)
        col2 = np.zeros(cols, dtype=np.float64)
        for s in range(rows):
            d = x[s].astype(np.float64) - mean
            col2 += d * d
        var = _tree(col2) / np.float64(count - ddof)
        std = np.sqrt(var)
    return np.float64(count), mean, var, std


SHARDS_MAX = 64       # NPB_PPO_SHARDS_MAX: the shards one combine takes


def moments_part(x, mean=None):
    """``(count, total)`` of one shard's ``x`` [rows, cols] (float32 or float64), both float64 (npb_rollout_moments_part): ``total`` is the
    undivided value ``moments`` has before its division -- a column's rows added in order onto 0.0, then ``_tree`` over the columns.  With
    ``mean`` given the summands are the rounded squares of ``(double)x - mean``."""
    x = np.asarray(x)
    if x.ndim != 2 or x.dtype not in (np.float32, np.float64):
        raise ValueError("moments are taken of a [rows, cols] float32 or float64 array")
    rows, cols = x.shape
    if rows < 1 or cols < 1:
        raise ValueError("rows and cols must be >= 1")
    with np.errstate(invalid="ignore", over="ignore"):
        col = np.zeros(cols, dtype=np.float64)
        for s in range(rows):
            w = x[s].astype(np.float64)
            if mean is not None:
                d = w - np.float64(mean)
                w = d * d
            col += w
        return np.float64(rows * cols), _tree(col)


def moments_combine(parts, ddof=1, squares=False):
    """W shards' parts [W, 2] added in ascending shard order (npb_rollout_moments_combine): ``C = 0.0; T = 0.0; for w ascending: C = C +
    count_w; T = T + total_w``.  ``squares`` false: ``(C, T / C)``, the count and the mean; true: ``(var, std)`` with ``var = T / (C -
    ddof)``, ``std = sqrt(var)``.  IEEE division and root; a NaN propagates."""
    parts = np.asarray(parts, dtype=np.float64)
    if parts.ndim != 2 or parts.shape[1] != 2 or not 1 <= parts.shape[0] <= SHARDS_MAX:
        raise ValueError("parts are [W, 2] with W 1 .. %d, not %r" % (SHARDS_MAX, parts.shape))
    ddof = int(ddof)
    if ddof < 0:
        raise ValueError("ddof must be >= 0")
    C, T = np.float64(0.0), np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for count, total in parts:
            C = C + count
            T = T + total
        if not C >= 1.0:
            raise ValueError("the shards' total count %r is below 1" % (float(C),))
        if not squares:
            return C, T / C
        if C <= ddof:
            raise ValueError("the shards' total count %d must exceed ddof = %d" % (int(C), ddof))
        var = T / (C - np.float64(ddof))
        return var, np.sqrt(var)


def moments_shards(xs, ddof=1):
    """``(count, mean, var, std)`` over W shards' arrays (``env.rollout_moments_shards``), the four steps in order: every shard's part,
    the combine, every shard's part around the GLOBAL mean, the combine.  ``moments_shards([x], ddof)`` has the bits of ``moments(x,
    ddof)``: no total is ever -0.0, so ``0.0 + T`` is ``T``."""
    xs = list(xs)
    count, mean = moments_combine([moments_part(x) for x in xs], ddof, False)
    if count <= int(ddof):
        raise ValueError("the shards' total count %d must exceed ddof = %d" % (int(count), int(ddof)))
    var, std = moments_combine([moments_part(x, mean) for x in xs], ddof, True)
    return count, mean, var, std


_M64 = (1 << 64) - 1


def _splitmix64(state: int):
    """one step of splitmix64: the next state and its output"""
    state = (state + 0x9E3779B97F4A7C15) & _M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return state, z ^ (z >> 31)


def permutation_keys(seed, epoch) -> np.ndarray:
    """the ROUNDS uint32 round keys of epoch ``epoch`` under ``seed`` (both taken modulo 2^64): a splitmix64 chain -- the first output
    from the seed, xor the epoch, is the state the next ROUNDS outputs are drawn from; a key is the high word of an output"""
    _, z = _splitmix64(int(seed) & _M64)
    state = z ^ (int(epoch) & _M64)
    keys = np.zeros(ROUNDS, dtype=np.uint32)
    for r in range(ROUNDS):
        state, z = _splitmix64(state)
        keys[r] = z >> 32
    return keys


def _mix(h: np.ndarray) -> np.ndarray:
    """murmur3's 32-bit finaliser, in uint32 arithmetic"""
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def permutation(N, keys, first=0, count=None) -> np.ndarray:
    """entries ``first .. first + count`` (default: to the end) of a permutation of range(N), 1 <= N <= 2^31 - 1, as int32; each entry is a
    function of its position alone.  b = max(bit_length(N - 1), 2), w = (b + 1) // 2; position i is split into L = i >> w and R = i & (2^w
    - 1), ROUNDS times ``L, R = R, L ^ (mix(R ^ key[r]) & (2^w - 1))``, and the result is L << w | R: a bijection on [0, 2^(2w)).  While
    the result is >= N the network is applied to it again (cycle walking): the walk from i < N stays on i's cycle, so it ends, and it is
    a bijection on [0, N)."""
    N = int(N)
    if not 1 <= N <= N_MAX:
        raise ValueError("a permutation has 1 .. 2^31 - 1 entries, not %r" % (N,))
    keys = np.asarray(keys, dtype=np.uint32)
    if keys.shape != (ROUNDS,):
        raise ValueError("%d round keys, not %r" % (ROUNDS, keys.shape))
    first = int(first)
    count = N - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > N:
        raise ValueError("entries [%d, %d) are not inside [0, %d)" % (first, first + count, N))
    w = np.uint32((max((N - 1).bit_length(), 2) + 1) // 2)
    mask = np.uint32((1 << int(w)) - 1)

    def network(x):
        L, R = x >> w, x & mask
        for r in range(ROUNDS):
            L, R = R, L ^ (_mix(R ^ keys[r]) & mask)
        return (L << w) | R
    with np.errstate(over="ignore"):
        x = network(np.arange(first, first + count, dtype=np.uint32))
        while True:
            out = np.flatnonzero(x >= np.uint32(N))
            if not out.size:
                break
            x[out] = network(x[out])
    return x.astype(np.int32)


def minibatch(arrays, t, adv, ret, keys, first, count, unit="transition", moments=None, eps=1e-8, every=None) -> dict:
    """What npb_rollout_minibatch returns for entries ``first .. first + count`` of the epoch ``keys`` belong to.  ``arrays``: what
    ``Recorder.arrays()`` / ``env.rollout()`` give, of which the first ``t`` slots count; ``adv``, ``ret``: [>= t, n].
    ``unit="transition"``: a permutation of the t * n cells; ``index[j]`` is the flat cell s * n + p, and ``obs`` [count, K, C], ``act``
    [count, A], ``extra`` [count, E], ``adv``, ``ret`` [count] are its rows.  ``unit="plant"``: a permutation of the n plants, every output
    time-major with the plants' sequences whole: ``src[:t, index]``, [t, count, ...].  ``moments`` (count, mean, var, std): adv becomes
    ``((double)adv - mean) / (std + eps)``, one subtraction, one addition and one IEEE division in double, narrowed once to adv's type.
    ``unit="segment"`` with ``every=L`` (npb_rollout_minibatch_segments; truncated segments of a recurrent policy): a permutation of the
    ``(t / L) * n`` segments; ``index[j]`` is the segment id ``g = c * n + p`` -- chunk c, plant p -- and every output is time-major
    [L, count, ...] with ``out[s][j] = src[c * L + s][p]``.  ``t % L != 0`` is refused: ragged last segments are not supported."""
    if unit not in UNITS:
        raise ValueError("a minibatch's unit is 'transition' or 'plant', not %r (or 'segment', with every=)" % (unit,))
    if (unit == "segment") != (every is not None):
        raise ValueError("every= is the slots of a segment: it goes with unit='segment', and only with it")
    t = int(t)
    if t < 1:
        raise ValueError("nothing recorded (t == 0)")
    if not float(eps) >= 0.0:
        raise ValueError("eps must be >= 0")
    obs = np.asarray(arrays["obs"])[:t]
    n = obs.shape[1]
    adv, ret = np.asarray(adv)[:t], np.asarray(ret)[:t]
    if unit == "segment":
        L = int(every)
        if L < 1 or L > t:
            raise ValueError("every must be 1 .. the recorded slots %d, not %r" % (t, every))
        if t % L:
            raise ValueError("the recorded slots %d are not a multiple of every = %d: ragged last segments are not supported" % (t, L))
    N = t * n if unit == "transition" else (n if unit == "plant" else (t // L) * n)
    if count < 1:
        raise ValueError("a minibatch has at least one entry")
    index = permutation(N, keys, first, count)
    if unit == "transition":
        def take(x):
            return None if x is None or x.shape[2:] == (0,) else x[:t].reshape((t * n,) + x.shape[2:])[index]
    elif unit == "plant":
        def take(x):
            return None if x is None or x.shape[2:] == (0,) else x[:t][:, index]
    else:
        slots = (index // n)[None, :] * L + np.arange(L)[:, None]      # [L, count]: the rollout's slot of every output cell

        def take(x):
            return None if x is None or x.shape[2:] == (0,) else x[:t][slots, (index % n)[None, :]]
    a = take(adv)
    if moments is not None:
        mean, std = np.float64(moments[1]), np.float64(moments[3])
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            a = ((a.astype(np.float64) - mean) / (std + np.float64(eps))).astype(adv.dtype)
    act, extra = arrays.get("act"), arrays.get("extra")
    return {"index": index, "obs": take(obs), "act": take(None if act is None else np.asarray(act)),
            "extra": take(None if extra is None else np.asarray(extra)), "adv": a, "ret": take(ret)}
