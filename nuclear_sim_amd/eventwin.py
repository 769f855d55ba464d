"""State windows around events, stated once in numpy: what the device captures behind every step while ``env.enable_event_windows`` is on
(npb_set_event_windows, nuclear_sim_amd/csrc/npd_event_windows.h), and the check of it.  Host only.

Every plant keeps the last ``H = pre + 1 + post`` samples of the recorded columns and of its clock.  A trigger compares this sample ``v`` of
its own column with the previous one ``prev``:

  ("bits", mask)       integer column: ``(v & mask) & ~(prev & mask) != 0``
  ("increase",)        ``v > prev``; a NaN on either side does not fire
  (">" | "<", limit)   the edge only: beyond the limit now and not beyond it at the previous sample

The first sample of a plant (after the start, a restart or a clear) only primes the triggers.  A trigger that finds the plant idle arms a
capture, taken ``post`` samples later, or when the episode ends first (``early``: flag bit 0, ``n_post`` short); a trigger that finds it
armed is counted in ``retriggers``.  A restart (the episode index changes) empties the ring and drops an armed capture.  A record's row k is
sample ``step + k - pre``; rows outside ``[pre - n_pre, pre + n_post]`` are NaN.  The window is copies: the device gives these bits exactly."""
from typing import Dict, Optional, Sequence

import numpy as np

MAX_COLUMNS = 16         # include/npb.h NPB_EVENT_WINDOW_COLS_MAX
MAX_TRIGGERS = 8         # NPB_EVENT_WINDOW_TRIGGERS_MAX
MAX_ROWS = 1024          # NPB_EVENT_WINDOW_ROWS_MAX
WORD_COLUMNS = ("plant", "episode", "trigger", "step", "n_pre", "n_post", "flags", "retriggers")      # int32 per record, in descriptor order
COLUMNS = WORD_COLUMNS + ("fired", "time", "times", "values")


def trigger_mode(t):
    """one trigger of ``record`` -> ("bits", mask) | ("increase",) | (">" | "<", limit); ValueError for anything else"""
    t = tuple(t)
    if len(t) == 2 and t[0] == "bits":
        mask = int(t[1])
        if not 0 < mask <= 0xFFFFFFFF:
            raise ValueError("a ('bits', mask) trigger needs 0 < mask < 2**32, not %r" % (t[1],))
        return ("bits", mask)
    if t == ("increase",):
        return t
    if len(t) == 2 and t[0] in (">", "<"):
        if np.isnan(float(t[1])):
            raise ValueError("the limit of a trigger is NaN")
        return (t[0], float(t[1]))
    raise ValueError("unknown trigger %r: ('bits', mask), ('increase',) or ('>' | '<', limit)" % (t,))


def empty(H: int, n_cols: int) -> Dict[str, np.ndarray]:
    """no records"""
    out = {name: np.zeros(0, dtype=np.int32) for name in WORD_COLUMNS}
    out.update(fired=np.zeros(0, dtype=np.uint32), time=np.zeros(0), times=np.zeros((0, H)), values=np.zeros((0, H, n_cols)),
               early=np.zeros(0, dtype=bool))
    return out


def record(values, clock, trigger_values, triggers: Sequence, pre: int, post: int, ended=None, episode_index=None) -> Dict[str, np.ndarray]:
    """The records of a run of S samples.  ``values`` [S, n_cols, n]: the recorded columns behind every step; ``clock`` [S, n]: the plant
    clock (prim.sim_time) behind it; ``trigger_values`` [S, T, n]: the trigger columns; ``triggers``: T modes (``trigger_mode``);
    ``ended`` [S, n] bool: the plant's episode ends on this step (None = never); ``episode_index`` [S, n]: the episode the step belonged
    to (None = one episode throughout).  Returns numpy columns of m records sorted by (capture step, plant): ``plant``, ``episode`` (0
    without an index), ``trigger`` (the lowest that fired), ``step`` (the trigger's sample), ``n_pre``, ``n_post``, ``flags``,
    ``retriggers`` (int32), ``fired`` (uint32 bit set), ``time`` (the clock at the trigger sample), ``times`` [m, H], ``values``
    [m, H, n_cols], and ``early`` = flags & 1."""
    values = np.asarray(values, dtype=np.float64)
    if values.ndim != 3:
        raise ValueError("values must be [steps, n_cols, n]")
    S, n_cols, n = values.shape
    clock = np.asarray(clock, dtype=np.float64).reshape(S, n)
    modes = [trigger_mode(t) for t in triggers]
    T = len(modes)
    if not 1 <= n_cols <= MAX_COLUMNS or not 1 <= T <= MAX_TRIGGERS:
        raise ValueError("event windows take 1 to %d columns and 1 to %d triggers" % (MAX_COLUMNS, MAX_TRIGGERS))
    pre, post = int(pre), int(post)
    H = pre + 1 + post
    if pre < 0 or post < 0 or H > MAX_ROWS:
        raise ValueError("pre >= 0, post >= 0 and pre + 1 + post <= %d" % MAX_ROWS)
    tv = np.asarray(trigger_values, dtype=np.float64).reshape(S, T, n)
    ended = None if ended is None else np.asarray(ended).astype(bool).reshape(S, n)
    index = None if episode_index is None else np.asarray(episode_index).astype(np.int64).reshape(S, n)
    valid = np.zeros(n, dtype=np.int64)                  # samples of this episode in the ring; 0 = unprimed
    due = np.full(n, -1, dtype=np.int64)                 # -1 = idle
    seen = np.zeros(n, dtype=np.int64) if index is None else index[0].copy()
    prev = np.zeros((T, n))
    armed = [None] * n                                   # [trigger, fired, step, clock, n_pre, retriggers]
    rows = []
    with np.errstate(invalid="ignore"):
        for s in range(S):
            for p in range(n):
                if index is not None and index[s, p] != seen[p]:         # 1. restarted since the last sample
                    seen[p], valid[p], due[p], armed[p] = index[s, p], 0, -1, None
                primed = valid[p] > 0                                     # 2. the sample is in the ring
                valid[p] = min(valid[p] + 1, H)
                fired = 0                                                 # 3. the triggers
                for t, mode in enumerate(modes):
                    v, pv = tv[s, t, p], prev[t, p]
                    prev[t, p] = v
                    if not primed:
                        continue
                    if mode[0] == "bits":
                        hit = ((int(v) & mode[1]) & ~(int(pv) & mode[1])) != 0
                    elif mode[0] == "increase":
                        hit = bool(v > pv)
                    elif mode[0] == ">":
                        hit = bool(v > mode[1]) and not bool(pv > mode[1])
                    else:
                        hit = bool(v < mode[1]) and not bool(pv < mode[1])
                    fired |= int(hit) << t
                if fired:                                                 # 4. arm, or count
                    if due[p] < 0:
                        due[p] = s + post
                        armed[p] = [(fired & -fired).bit_length() - 1, fired, s, clock[s, p], min(pre, int(valid[p]) - 1), 0]
                    else:
                        armed[p][5] += 1
                if due[p] >= 0:                                           # 5. due, or cut short by the episode's end
                    early = s != due[p] and ended is not None and bool(ended[s, p])
                    if s == due[p] or early:
                        trig, fset, s0, t0, n_pre, again = armed[p]
                        n_post = s - s0
                        win = np.full((H, n_cols), np.nan)
                        tim = np.full(H, np.nan)
                        for k in range(pre - n_pre, pre + n_post + 1):
                            win[k] = values[s0 + k - pre, :, p]
                            tim[k] = clock[s0 + k - pre, p]
                        rows.append((s, p, 0 if index is None else int(index[s, p]), trig, s0, n_pre, n_post, int(early), again, fset, t0, tim, win))
                        due[p], armed[p] = -1, None
    if not rows:
        return empty(H, n_cols)
    rows.sort(key=lambda r: (r[0], r[1]))
    out = {name: np.array([r[j] for r in rows], dtype=np.int32)
           for name, j in (("plant", 1), ("episode", 2), ("trigger", 3), ("step", 4), ("n_pre", 5), ("n_post", 6), ("flags", 7), ("retriggers", 8))}
    out["fired"] = np.array([r[9] for r in rows], dtype=np.uint32)
    out["time"] = np.array([r[10] for r in rows], dtype=np.float64)
    out["times"] = np.stack([r[11] for r in rows])
    out["values"] = np.stack([r[12] for r in rows])
    out["early"] = (out["flags"] & 1) != 0
    return out


def same(got: Dict[str, np.ndarray], want: Dict[str, np.ndarray], names=None) -> None:
    """the check: every column of ``names`` (default: those of ``want``) equal bit for bit, NaNs by their bits; AssertionError names the
    first cell"""
    for name in (names if names is not None else list(want)):
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        ia, ib = (a.view(np.int64), b.view(np.int64)) if a.dtype == np.float64 else (a, b)
        if not np.array_equal(ia, ib):
            bad = np.argwhere(ia != ib)
            where = tuple(int(x) for x in bad[0])
            raise AssertionError("%s differs in %d of %d cells, first at %r: %r vs %r" % (name, len(bad), a.size, where, a[where], b[where]))
