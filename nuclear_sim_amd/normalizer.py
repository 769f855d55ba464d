"""Running observation and reward normalisation, stated once in numpy: what the device keeps behind every step while ``env.set_normalizer``
is on (npb_set_normalizer, nuclear_sim_amd/csrc/npd_normalizer.h and npb_minibatch.hip).  Host only.  The device gives these bits for
every n, storage type and launch geometry.

STREAMS.  ``Normalizer(spec, columns, n, reward=None, eps=1e-8)`` keeps S streams: the chosen columns of a features spec
(``features.py``; indices into ``spec["columns"]``, at most 64), then, last, the return stream if ``reward = {"gamma": g, "clip": c}`` is
given.  A chosen column must be ``"affine"`` with a constant ``ref``: a ``"bits"`` column and a column whose ``ref`` is a second column
are refused by name (``check``).  Per stream the state is three float64, ``count``, ``mean`` and ``M2``, all 0 at the start.

ONE FOLD over the n plants (``fold``), for stream c with raw samples x[p] -- the column's row of ``samples`` before any transform,
widened to float64 as the features widen it; for the return stream ``ret[p]``, below:

    shift = mean[c] if count[c] > 0 else the column's own ref (the return stream: 0.0)
    d = x - shift;  q = d * d                  each rounded on its own
    a sample counts iff q - q == 0.0           not a NaN, not an infinity, not a square that overflows; a sample that does not count
                                               contributes +0.0, +0.0 and count 0: one bad value never poisons a statistic
    s1 = _tree(d);  s2 = _tree(q)              in plant order through ``rollout._tree``: groups of 256 padded with +0.0, the halves
                                               128 .. 1, then the groups' results as the next level
    cnt = the samples that count;  N = count + cnt
    if cnt > 0:  mean = shift + s1 / N;  M2 = (M2 + s2) - (s1 * s1) / N, 0.0 where that is negative       (IEEE division)
    count = N

WHY THAT IS CHAN'S MERGE.  Chan, Golub and LeVeque merge a population A (n_a, mean_a, M2_a) with a batch B (n_b, mean_b, M2_b), N = n_a
+ n_b and delta = mean_b - mean_a, into mean = mean_a + delta * n_b / N and M2 = M2_a + M2_b + delta^2 * n_a * n_b / N.  Take the batch
around the running mean: with d = x - mean_a, s1 = sum d and s2 = sum d^2 the batch has mean_b = mean_a + s1 / n_b, so delta = s1 / n_b,
and M2_b = s2 - s1^2 / n_b (the shifted-data formula: a shift leaves the spread alone).  Then

    mean = mean_a + (s1 / n_b) * n_b / N                          = mean_a + s1 / N
    M2   = M2_a + s2 - s1^2 / n_b + (s1 / n_b)^2 * n_a * n_b / N  = M2_a + s2 - (s1^2 / n_b) * (1 - n_a / N)  = (M2_a + s2) - s1^2 / N

One subtraction of nearly equal numbers is left, s2 against s1^2 / N, and both are small: the differences are taken around the running
mean, so s1 / N is the batch's drift and not the column's level.  Rounding can leave M2 a hair below 0 for a constant column: the clamp.
THE FIRST FOLD, from count == 0, has no running mean and shifts by the column's ``ref`` instead.  There n_a = 0 and M2_a = 0, and the
algebraically correct form is the shifted-data formula itself, mean = ref + s1 / cnt and M2 = s2 - s1^2 / cnt: exactly what the lines
above compute with N = cnt and M2 = 0.0 -- no population stands on the other side of the merge whose mean the shift would have to be.
How well it is conditioned depends on how far ``ref`` lies from the data: the error of M2 / count is about u * (1 + ((mean - ref) / std)^2)
per level of the tree.

THE TABLE (``table``).  Where count > 0: ref = mean, scale = 1.0 / sqrt(M2 / count + eps), IEEE root and division; else the spec's own
ref and scale.  ``lo``, ``hi`` and ``nan_to`` stay the spec's: the clip of the normalised observation is the column's clip.  ``apply``
puts the table into a copy of the spec, with which ``features.Stack`` reproduces the device's stacks.  The fold comes BEFORE the features'
pass A: the frame the policy sees is normalised with statistics that include it.  FRESH frames (the features' pass B and the priming) are
not folded; they are normalised with the table as it stands.

THE RETURN STREAM.  Per plant ``ret`` (float64) and ``primed`` / ``seen`` as ``features.Stack`` uses them, and ``ended``, whether the
step before ended the plant's episode.  Behind a step with reward r, done flags and the carried episode indices:

    carry = primed and index == seen and not ended
    ret   = (ret * gamma if carry else 0.0) + r          ret * gamma rounded before the sum
    fold, merge                                          (training only)
    norm_reward = r * rscale, then y = -clip where y < -clip, y = clip where y > clip       a NaN passes both comparisons
    primed = 1;  seen = index;  ended = done != 0

rscale = 1.0 / sqrt(M2 / count + eps) of the return stream, 1.0 while its count is 0; the mean is not subtracted.  r and done are the
task's while a task is set, else the step's.  A truncation, an autoreset or a caller's reset / restore shows as a changed index.

FROZEN (``training = False``): no fold, no merge, no new table; ``norm_reward`` is still formed, with the frozen scale, and ``ret`` is
still carried.

``merge`` is Chan's merge of several states -- shards' --, host only and not bit-pinned.

ONE NORMALISER ACROSS SHARDS (``shard_delta``, ``combine``; npb_normalizer_shard_delta, npb_normalizer_apply_shards and
``env.normalizer_sync`` give these bits).  Every shard keeps, beside its state, the BASE: what all shards agreed on at the last
synchronisation, zeros before the first.  A synchronisation has two halves.  ``shard_delta(cur, base)`` is, per stream, the population
the shard folded since the base -- Chan's merge run backwards, every operation in float64 and rounded on its own:

    na, ma, Ma = base;  N, m, M = cur;  nb = N - na
    nb > 0:   mb = m + (m - ma) * (na / nb);   d = mb - ma
              Mb = (M - Ma) - (d * d) * ((na * nb) / N),   0.0 where that is negative
              delta = (nb, mb, Mb)
    else:     delta = (0.0, 0.0, 0.0)        (a frozen shard, or one that did not step)

The forward merge has m = ma + (mb - ma) * nb / N, so m - ma = (mb - ma) * nb / N and mb - m = (mb - ma) * na / N = (m - ma) * na / nb:
the first line; and M = Ma + Mb + d^2 * na * nb / N solved for Mb is the second.  With ``base == 0`` the delta is ``cur`` exactly: na = 0
makes the correction of the mean m * 0 and that of M2 d^2 * 0.  ``combine(base, deltas)`` starts from the base and goes through the
shards in ascending order; only a shard with nb > 0 is merged:

    N = n + nb;  d = mb - mean;  mean = mean + d * (nb / N)
    M2 = (M2 + Mb) + (d * d) * ((n * nb) / N);  n = N

The result is every shard's new state AND its new base; the features' table and the return stream's rscale follow it as they follow a
loaded state.  The per-plant return carry (``ret``, ``primed``, ``seen``, ``ended``) stays with its shard.  Shards that combine the same
deltas in the same order hold the same bits, so nothing is broadcast, and samples folded before the base are never counted twice.
ONE CONSEQUENCE: W = 1 is the identity only from a zero base.  From any other base the shard's own samples are un-merged and merged
again, and both round: the state after a synchronisation of one shard may differ from the state before it in the last bits.  That is
intended -- the price of every shard computing the same thing.

NOT here: statistics over fresh frames; per-plant statistics (``env.enable_column_stats`` has them); an exponential moving average; half
types; synchronising shards on the device; normalising ``bits`` or setpoint-error columns.  (Synchronising shards on the device has
since come: ``shard_delta`` and ``combine`` above state it.)"""
import copy
from typing import Dict, Optional, Sequence

import numpy as np

from . import features
from .rollout import _tree

COLS_MAX = features.COLS_MAX      # the streams of feature columns; the return stream is one more


def check(spec: Optional[Dict], columns: Sequence[int], reward: Optional[Dict] = None, eps: float = 1e-8) -> None:
    """ValueError, naming the reason, for what the device would refuse (npb_normalizer_check)"""
    columns = list(columns or ())
    if not columns and reward is None:
        raise ValueError("neither columns nor reward: nothing to normalise")
    if columns and spec is None:
        raise ValueError("columns chosen while no features are set")
    if len(columns) > COLS_MAX:
        raise ValueError("the normaliser takes at most %d columns, not %d" % (COLS_MAX, len(columns)))
    seen = set()
    for j in columns:
        if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 0 <= j < len(spec["columns"]):
            raise ValueError("column index %r is out of range: it names one of the features' %d columns" % (j, len(spec["columns"])))
        if j in seen:
            raise ValueError("column %d is named twice" % j)
        seen.add(int(j))
        D = spec["columns"][j]
        if D["kind"] != "affine":
            raise ValueError("column %d: a 'bits' column cannot be normalised" % j)
        if isinstance(D["ref"], tuple):
            raise ValueError("column %d: its ref is a second column (a setpoint error): it cannot be normalised" % j)
    if not float(eps) >= 0.0:
        raise ValueError("eps must be >= 0 (a NaN is not)")
    if reward is not None:
        if not 0.0 <= float(reward["gamma"]) <= 1.0:
            raise ValueError("gamma must lie in [0, 1]")
        if not float(reward["clip"]) > 0.0:
            raise ValueError("clip must be positive (a NaN is not)")


class Normalizer:
    """the running statistics of S streams over n plants, as the handle keeps them: ``count``, ``mean``, ``M2`` float64 [S]; with the
    return stream ``ret`` float64 [n], ``primed``, ``seen``, ``ended`` int32 [n]; ``training``"""

    def __init__(self, spec: Optional[Dict], columns: Sequence[int], n: int, reward: Optional[Dict] = None, eps: float = 1e-8):
        check(spec, columns, reward, eps)
        self.spec, self.columns, self.n, self.eps = spec, [int(j) for j in (columns or ())], int(n), np.float64(eps)
        self.reward = None if reward is None else {"gamma": np.float64(reward["gamma"]), "clip": np.float64(reward["clip"])}
        self.S = len(self.columns) + (reward is not None)
        self.ref0 = np.array([spec["columns"][j]["ref"] for j in self.columns] + [0.0] * (reward is not None), dtype=np.float64)
        self.scale0 = np.array([spec["columns"][j]["scale"] for j in self.columns] + [1.0] * (reward is not None), dtype=np.float64)
        self.count, self.mean, self.M2 = (np.zeros(self.S, dtype=np.float64) for _ in range(3))
        self.ret = np.zeros(self.n, dtype=np.float64)
        self.primed, self.seen, self.ended = (np.zeros(self.n, dtype=np.int32) for _ in range(3))
        self.training = True

    def _fold(self, c: int, x: np.ndarray) -> None:
        """stream c takes the n samples x"""
        with np.errstate(all="ignore"):
            shift = self.mean[c] if self.count[c] > 0 else self.ref0[c]
            d = np.asarray(x, dtype=np.float64) - shift
            q = d * d
            counts = (q - q) == 0.0
            s1, s2 = _tree(np.where(counts, d, 0.0)), _tree(np.where(counts, q, 0.0))
            cnt = np.float64(np.count_nonzero(counts))
            N = self.count[c] + cnt
            if cnt > 0:
                self.mean[c] = shift + s1 / N
                M2 = (self.M2[c] + s2) - (s1 * s1) / N
                self.M2[c] = np.float64(0.0) if M2 < 0.0 else M2
            self.count[c] = N

    def step(self, samples=None, reward=None, done=None, index=None) -> Optional[np.ndarray]:
        """behind a step, in front of the features' pass A: ``samples`` [n_rows, n] as ``features.frame`` takes them (may be None without
        columns), and with the return stream ``reward`` [n], ``done`` [n] and the carried episode ``index`` (None: the one seen).
        Returns ``norm_reward`` [n], or None without the return stream."""
        if self.training:
            for c, j in enumerate(self.columns):
                self._fold(c, np.asarray(samples, dtype=np.float64)[self.spec["columns"][j]["col"]])
        if self.reward is None:
            return None
        with np.errstate(all="ignore"):
            r = np.asarray(reward, dtype=np.float64)
            index = self.seen.copy() if index is None else np.asarray(index, dtype=np.int32)
            carry = (self.primed != 0) & (index == self.seen) & (self.ended == 0)
            kept = self.ret * self.reward["gamma"]
            self.ret = np.where(carry, kept, 0.0) + r
            if self.training:
                self._fold(self.S - 1, self.ret)
            y = r * self.table()[1][self.S - 1]
            clip = self.reward["clip"]
            y = np.where(y < -clip, -clip, y)
            y = np.where(y > clip, clip, y)
        self.primed[:] = 1
        self.seen[:] = index
        self.ended[:] = np.asarray(done) != 0
        return y

    def clear(self, mask=None) -> None:
        """the plants of mask (None = all) start a new return on their next step"""
        self.primed[slice(None) if mask is None else np.asarray(mask, dtype=bool)] = 0

    def table(self):
        """``(ref, scale)`` float64 [S]: what the features' table holds of every stream (the return stream's scale is rscale)"""
        with np.errstate(all="ignore"):
            on = self.count > 0
            var = self.M2 / np.where(on, self.count, 1.0)
            scale = np.float64(1.0) / np.sqrt(var + self.eps)
        return np.where(on, self.mean, self.ref0), np.where(on, scale, self.scale0)

    def apply(self, spec: Optional[Dict] = None) -> Dict:
        """the features spec with the table's ref and scale put in"""
        out = copy.deepcopy(self.spec if spec is None else spec)
        ref, scale = self.table()
        for c, j in enumerate(self.columns):
            out["columns"][j]["ref"], out["columns"][j]["scale"] = np.float64(ref[c]), np.float64(scale[c])
        return out

    def stats(self) -> Dict[str, np.ndarray]:
        """count, mean, var (M2 / count, 0 where count is 0) and scale (the table's), float64 [S]"""
        on = self.count > 0
        return {"count": self.count.copy(), "mean": self.mean.copy(), "var": np.where(on, self.M2 / np.where(on, self.count, 1.0), 0.0),
                "scale": self.table()[1]}

    def state(self) -> Dict[str, np.ndarray]:
        names = ("count", "mean", "M2") + (("ret", "primed", "seen", "ended") if self.reward is not None else ())
        return {name: getattr(self, name).copy() for name in names}

    def load_state(self, state: Dict) -> None:
        for name, value in state.items():
            getattr(self, name)[...] = value


def merge(states: Sequence[Dict]) -> Dict[str, np.ndarray]:
    """Chan's merge of several normalisers' ``count``, ``mean``, ``M2`` ([S] each; shards of one run): what one normaliser over all their
    samples holds, up to rounding.  Host only, not bit-pinned; the per-plant return carry stays with its shard."""
    count, mean, M2 = (np.array(states[0][k], dtype=np.float64) for k in ("count", "mean", "M2"))
    for B in states[1:]:
        nb, mb, Mb = (np.asarray(B[k], dtype=np.float64) for k in ("count", "mean", "M2"))
        N = count + nb
        safe = np.where(N > 0, N, 1.0)
        delta = mb - mean
        mean = np.where(nb > 0, mean + delta * (nb / safe), mean)
        M2 = M2 + Mb + delta * delta * (count * nb / safe)
        count = N
    return {"count": count, "mean": mean, "M2": M2}


SHARDS_MAX = 64       # NPB_PPO_SHARDS_MAX: the shards one combine takes


def _triple(state, who):
    """``{count, mean, M2}`` or an array [3, S] as three float64 [S] vectors"""
    if isinstance(state, dict):
        rows = [np.asarray(state[k], dtype=np.float64) for k in ("count", "mean", "M2")]
    else:
        a = np.asarray(state, dtype=np.float64)
        if a.ndim != 2 or a.shape[0] != 3:
            raise ValueError("%s: a state is {count, mean, M2} or an array [3, S], not an array %r" % (who, a.shape))
        rows = list(a)
    if any(r.ndim != 1 or r.shape != rows[0].shape for r in rows):
        raise ValueError("%s: count, mean and M2 must be vectors of one length" % who)
    return rows


def shard_delta(cur: Dict, base: Dict) -> Dict[str, np.ndarray]:
    """The population a shard folded since ``base`` (module docstring): ``{count, mean, M2}`` float64 [S]; zeros for a stream with nothing
    new.  ``shard_delta(cur, zeros)`` is ``cur`` by bits."""
    N, m, M = _triple(cur, "shard_delta")
    na, ma, Ma = _triple(base, "shard_delta")
    if N.shape != na.shape:
        raise ValueError("shard_delta: cur has %d streams and base %d" % (N.size, na.size))
    with np.errstate(all="ignore"):
        nb = N - na
        on = nb > 0
        safe = np.where(on, nb, 1.0)
        mb = m + (m - ma) * (na / safe)
        d = mb - ma
        Mb = (M - Ma) - (d * d) * ((na * nb) / np.where(on, N, 1.0))
        Mb = np.where(Mb < 0.0, 0.0, Mb)
    zero = np.zeros_like(nb)
    return {"count": np.where(on, nb, zero), "mean": np.where(on, mb, zero), "M2": np.where(on, Mb, zero)}


def combine(base: Dict, deltas: Sequence) -> Dict[str, np.ndarray]:
    """``base`` merged with the shards' deltas in ascending order (module docstring): every shard's new state and new base, ``{count,
    mean, M2}`` float64 [S].  ``deltas``: 1 .. 64 of what ``shard_delta`` returns, or an array [W, 3, S]."""
    n, mean, M2 = (r.copy() for r in _triple(base, "combine"))
    deltas = list(deltas)
    if not 1 <= len(deltas) <= SHARDS_MAX:
        raise ValueError("combine: 1 .. %d shards, not %d" % (SHARDS_MAX, len(deltas)))
    with np.errstate(all="ignore"):
        for D in deltas:
            nb, mb, Mb = _triple(D, "combine")
            if nb.shape != n.shape:
                raise ValueError("combine: a delta has %d streams and the base %d" % (nb.size, n.size))
            on = nb > 0
            N = n + nb
            safe = np.where(on, N, 1.0)
            d = mb - mean
            mean = np.where(on, mean + d * (nb / safe), mean)
            M2 = np.where(on, (M2 + Mb) + (d * d) * ((n * nb) / safe), M2)
            n = np.where(on, N, n)
    return {"count": n, "mean": mean, "M2": M2}
