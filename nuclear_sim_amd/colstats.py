"""Per-plant column statistics, stated once in numpy: what the device folds behind every step while ``env.enable_column_stats`` is on
(npb_set_column_stats, nuclear_sim_amd/csrc/npd_column_stats.h), and the check of it.  Host only.

One sample per step and (column, plant), widened to double; the cells, per (column, plant) unless noted:

  n_samples     int32, per plant   samples folded
  min, max      float64            ``v < min ? v : min`` / ``v > max ? v : max``: a NaN sample replaces neither; empty +inf / -inf
  sum, sumsq    float64            ``sum + v`` / ``sumsq + v * v``, sequential adds in step order, the product rounded before its add;
                                   empty 0
  last          float64            the latest sample; empty NaN
  first_beyond  float64            columns with a limit only: the plant clock after the first step whose sample was beyond the limit
                                   (``>`` for direction +1, ``<`` for -1); empty +inf = never
  n_beyond      int32              columns with a limit only: samples that were beyond it; empty 0

The sums are plain sequential float64 adds, so the device (built without contraction of a * b + c) gives these bits exactly."""
from typing import Dict, Optional

import numpy as np

STATS = ("min", "max", "sum", "sumsq", "last", "first_beyond", "n_beyond")      # the per-cell tables, in descriptor order
LIMIT_STATS = ("first_beyond", "n_beyond")                                      # those that need a limit
DEFAULT_STATS = ("min", "max", "sum", "sumsq", "last")
MAX_COLUMNS = 32                                                                # include/npb.h NPB_COLUMN_STATS_MAX
EMPTY = {"min": np.inf, "max": -np.inf, "sum": 0.0, "sumsq": 0.0, "last": np.nan, "first_beyond": np.inf, "n_beyond": 0}


def empty(n_cols: int, n: int) -> Dict[str, np.ndarray]:
    """the tables before any sample"""
    out = {name: np.full((n_cols, n), EMPTY[name], dtype=np.int32 if name == "n_beyond" else np.float64) for name in STATS}
    out["n_samples"] = np.zeros(n, dtype=np.int32)
    return out


def directions(limits: Optional[dict], n_cols: int):
    """``{column_index: (">" | "<" | +1 | -1, value)}`` -> (direction int32[n_cols], limit float64[n_cols]); ValueError for an index outside
    the columns, an unknown direction or a NaN limit"""
    direction, limit = np.zeros(n_cols, dtype=np.int32), np.zeros(n_cols, dtype=np.float64)
    for c, (d, value) in (limits or {}).items():
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < n_cols:
            raise ValueError("limit on column %r: the columns are 0 .. %d" % (c, n_cols - 1))
        if d not in (">", "<", 1, -1):
            raise ValueError("limit direction %r of column %d: '>' or '<'" % (d, c))
        if np.isnan(float(value)):
            raise ValueError("the limit of column %d is NaN" % c)
        direction[c], limit[c] = (1 if d in (">", 1) else -1), float(value)
    return direction, limit


def fold(values, times, limits: Optional[dict] = None, into: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """Fold ``values`` [steps, n_cols, n] (one sample per step, behind that step) step by step into the tables; ``times`` [steps, n] is the
    plant clock (prim.sim_time) after each step, read for ``first_beyond``.  ``limits``: ``{column_index: (">" | "<", value)}``.  ``into``:
    tables to go on from (changed in place and returned), else the empty ones."""
    values = np.asarray(values, dtype=np.float64)
    if values.ndim != 3:
        raise ValueError("values must be [steps, n_cols, n]")
    steps, n_cols, n = values.shape
    times = np.asarray(times, dtype=np.float64).reshape(steps, n)
    direction, limit = directions(limits, n_cols)
    s = empty(n_cols, n) if into is None else into
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(steps):
            v = values[t]
            s["min"] = np.where(v < s["min"], v, s["min"])
            s["max"] = np.where(v > s["max"], v, s["max"])
            s["sum"] = s["sum"] + v
            s["sumsq"] = s["sumsq"] + v * v
            s["last"] = v.copy()
            beyond = ((direction[:, None] > 0) & (v > limit[:, None])) | ((direction[:, None] < 0) & (v < limit[:, None]))
            s["n_beyond"] = s["n_beyond"] + beyond.astype(np.int32)
            first = beyond & (s["first_beyond"] == np.inf)
            s["first_beyond"] = np.where(first, np.broadcast_to(times[t], (n_cols, n)), s["first_beyond"])
            s["n_samples"] = s["n_samples"] + np.int32(1)
    return s


def moments(stats: Dict[str, np.ndarray]):
    """(mean, variance) [n_cols, n] from ``sum``, ``sumsq`` and ``n_samples``: sum / k and sumsq / k - mean^2 (the population variance, not
    below 0); NaN where nothing was folded"""
    k = np.asarray(stats["n_samples"], dtype=np.float64)
    k = np.where(k > 0, k, np.nan)
    mean = np.asarray(stats["sum"], dtype=np.float64) / k
    return mean, np.maximum(np.asarray(stats["sumsq"], dtype=np.float64) / k - mean * mean, 0.0)


def same(got: Dict[str, np.ndarray], want: Dict[str, np.ndarray], names=None) -> None:
    """the check: every table of ``names`` (default: those in both) equal bit for bit, NaNs by their bits; AssertionError names the first cell"""
    for name in (names if names is not None else [k for k in want if k in got]):
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        ia, ib = (a.view(np.int64), b.view(np.int64)) if a.dtype == np.float64 else (a, b)
        if not np.array_equal(ia, ib):
            bad = np.argwhere(ia != ib)
            where = tuple(int(x) for x in bad[0])
            raise AssertionError("%s differs in %d of %d cells, first at %r: %r vs %r" % (name, len(bad), a.size, where, a[where], b[where]))
