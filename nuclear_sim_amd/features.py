"""Caller-defined policy inputs, stated once in numpy: the frame stack the device keeps behind every step while ``env.set_features`` is on
(npb_set_features, nuclear_sim_amd/csrc/npd_features.h), and a helper that turns column statistics into a normaliser.  Host only.

A ``spec`` is ``{"stack": K, "dtype": "float32" | "float64", "columns": [...]}`` over the rows of a ``samples`` array [n_rows, n] (every
value widened to float64, as the device widens it).  A column is ``{"col": row, "kind": k, ...}``, y by kind:

  "affine"    (v - ref) * scale        ``ref``: a number, or ("col", row) for a second column (a setpoint error); the subtraction is
                                       rounded before the product
  "bits"      integer column: 1.0 if (v & ``mask``) != 0 else 0.0

and behind the kind, in this order: a NaN becomes ``nan_to``, or where ``nan_to`` is a NaN itself THE quiet NaN (sign clear, no payload:
which NaN an ``inf - inf`` gives differs between machines, so the bits are fixed here); ``y = lo if y < lo else y``, then ``y = hi if y >
hi else y`` (a NaN passes both comparisons; -inf / +inf: no clip); float32 output is ``astype(float32)``: round to nearest even, overflow
to inf, subnormals kept.

A frame is the C values of one plant; ``out[p, k, c]`` holds the last K frames, ``k = K - 1`` the newest.  A FRESH frame is the frame of
a plant whose step outputs do not describe its current state (after a restore or a reset, before any step of the new episode): columns
with ``"live": True`` (state members, the observation) are read, every other column takes its raw value ``fresh`` (a second column without
``"ref_live"``: ``ref_fresh``) through the same transform.  ``Stack`` keeps the tensor and per plant a primed flag and the episode index
last seen, and states the three passes; the device gives these bits exactly."""
from typing import Dict, Optional, Sequence

import numpy as np

COLS_MAX = 64            # include/npb.h NPB_FEATURES_COLS_MAX
STACK_MAX = 16           # NPB_FEATURES_STACK_MAX
CELLS_MAX = 256          # NPB_FEATURES_CELLS_MAX
KINDS = ("affine", "bits")      # NPB_FEATURE_KIND_*, in order
DTYPES = ("float32", "float64")      # NPB_FEATURES_F32, NPB_FEATURES_F64
QUIET_NAN = np.array(0x7FF8000000000000, dtype=np.uint64).view(np.float64)[()]      # as float32: 0x7fc00000


def column(col: int, kind: str = "affine", scale: float = 1.0, ref=0.0, lo: float = -np.inf, hi: float = np.inf, nan_to: float = np.nan,
           mask: int = 0, fresh: float = 0.0, ref_fresh: float = 0.0, live: bool = False, ref_live: bool = False) -> Dict:
    """one column of a spec, with the defaults"""
    return {"col": col, "kind": kind, "scale": scale, "ref": ref, "lo": lo, "hi": hi, "nan_to": nan_to, "mask": mask, "fresh": fresh,
            "ref_fresh": ref_fresh, "live": live, "ref_live": ref_live}


def check(spec: Dict) -> None:
    """ValueError, naming the reason, for a spec the device would refuse (npb_features_check) as far as the host words show it"""
    cols, K = list(spec["columns"]), spec["stack"]
    if not 1 <= len(cols) <= COLS_MAX:
        raise ValueError("features take 1 to %d columns, not %d" % (COLS_MAX, len(cols)))
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= STACK_MAX:
        raise ValueError("the stack depth must be 1 .. %d, not %r" % (STACK_MAX, K))
    if K * len(cols) > CELLS_MAX:
        raise ValueError("stack * columns must be <= %d, not %d * %d" % (CELLS_MAX, K, len(cols)))
    if spec.get("dtype", "float32") not in DTYPES:
        raise ValueError("the output type must be float32 or float64 (no half types), not %r" % (spec.get("dtype"),))
    for c, D in enumerate(cols):
        if D["kind"] not in KINDS:
            raise ValueError("column %d: unknown kind %r: one of %r" % (c, D["kind"], KINDS))
        if D["kind"] == "bits" and not 0 < int(D["mask"]) <= 0xFFFFFFFF:
            raise ValueError("column %d: 'bits' needs 0 < mask < 2**32" % c)
        numbers = ("lo", "hi", "fresh") + (("scale", "ref_fresh") + (() if isinstance(D["ref"], tuple) else ("ref",)) if D["kind"] == "affine" else ())
        for name in numbers:
            if np.isnan(float(D[name])):
                raise ValueError("column %d: %s is NaN" % (c, name))
        if D["lo"] > D["hi"]:
            raise ValueError("column %d: a clip with lo > hi" % c)


def frame(samples: np.ndarray, spec: Dict, fresh: bool = False) -> np.ndarray:
    """the frame of every plant, [n, C] in the spec's dtype, from ``samples`` [n_rows, n]; ``fresh``: the fresh frame"""
    samples = np.asarray(samples, dtype=np.float64)
    n = samples.shape[1]
    out = np.empty((n, len(spec["columns"])), dtype=np.dtype(spec.get("dtype", "float32")))
    with np.errstate(all="ignore"):
        for c, D in enumerate(spec["columns"]):
            v = samples[D["col"]] if (not fresh or D["live"]) else np.full(n, float(D["fresh"]))
            if D["kind"] == "bits":
                y = np.where((v.astype(np.int64).astype(np.uint32) & np.uint32(D["mask"])) != 0, 1.0, 0.0)
            else:
                if isinstance(D["ref"], tuple):
                    ref = samples[D["ref"][1]] if (not fresh or D["ref_live"]) else np.full(n, float(D["ref_fresh"]))
                else:
                    ref = np.float64(D["ref"])
                d = v - ref                      # rounded before the product
                y = d * np.float64(D["scale"])
            nan_to = np.float64(D["nan_to"])
            y = np.where(np.isnan(y), QUIET_NAN if np.isnan(nan_to) else nan_to, y)
            y = np.where(y < np.float64(D["lo"]), np.float64(D["lo"]), y)
            y = np.where(y > np.float64(D["hi"]), np.float64(D["hi"]), y)
            out[:, c] = y.astype(out.dtype)
    return out


class Stack:
    """the frame stack of n plants and its bookkeeping, as the handle keeps them: ``out`` [n, K, C], ``final`` [n, K, C] or None,
    ``primed`` and ``seen`` int32 [n]"""

    def __init__(self, spec: Dict, n: int, final: bool = False, out: Optional[np.ndarray] = None, final_fill=0):
        check(spec)
        self.spec, self.n = spec, n
        K, C, dt = spec["stack"], len(spec["columns"]), np.dtype(spec.get("dtype", "float32"))
        self.out = np.zeros((n, K, C), dtype=dt) if out is None else np.array(out, dtype=dt).reshape(n, K, C)
        self.final = np.full((n, K, C), final_fill, dtype=dt) if final else None
        self.primed, self.seen = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)

    def _index(self, index) -> np.ndarray:
        return self.seen.copy() if index is None else np.asarray(index, dtype=np.int32)

    def step(self, samples, index=None) -> np.ndarray:
        """pass A, behind a step: shift and append where the plant is primed and of the episode seen, else fill; returns who filled"""
        index = self._index(index)
        f = frame(samples, self.spec)
        fill = (self.primed == 0) | (index != self.seen)
        self.out[~fill, :-1] = self.out[~fill, 1:]
        self.out[~fill, -1] = f[~fill]
        self.out[fill] = f[fill][:, None, :]
        self.primed[:] = 1
        self.seen[:] = index
        return fill

    def restart(self, samples, index) -> np.ndarray:
        """pass B, behind the episode kernel: the plants whose index differs from the one seen -- their stacks to ``final``, then the
        fresh frame of the restored state in every slot; returns who restarted"""
        index = self._index(index)
        restarted = index != self.seen
        if self.final is not None:
            self.final[restarted] = self.out[restarted]
        self.out[restarted] = frame(samples, self.spec, fresh=True)[restarted][:, None, :]
        self.seen[restarted] = index[restarted]
        self.primed[restarted] = 1
        return restarted

    def prime(self, samples, index=None) -> np.ndarray:
        """the unprimed plants: the fresh frame of the current state in every slot; returns who was primed"""
        index = self._index(index)
        todo = self.primed == 0
        self.out[todo] = frame(samples, self.spec, fresh=True)[todo][:, None, :]
        self.seen[todo] = index[todo]
        self.primed[todo] = 1
        return todo

    def clear(self, mask=None) -> None:
        """the plants of mask (None = all) unprimed"""
        self.primed[slice(None) if mask is None else np.asarray(mask, dtype=bool)] = 0


def spec_from_stats(column_stats: Dict, columns: Sequence[int]) -> list:
    """A normaliser from a dry run with ``env.enable_column_stats(..., stats=("sum", "sumsq"))``: per entry of ``columns`` (indices into the
    statistics' columns) ``{"ref": mean, "scale": 1 / std}`` over all plants' samples -- mean = sum / n_samples, std = sqrt(sumsq /
    n_samples - mean * mean), scale 1 where the variance is not positive -- the options ``env.set_features`` takes per column."""
    total = float(np.sum(np.asarray(column_stats["n_samples"], dtype=np.float64)))
    if total <= 0:
        raise ValueError("the column statistics hold no sample")
    out = []
    for c in columns:
        s = float(np.sum(np.asarray(column_stats["sum"], dtype=np.float64)[c]))
        q = float(np.sum(np.asarray(column_stats["sumsq"], dtype=np.float64)[c]))
        mean = s / total
        var = q / total - mean * mean
        out.append({"ref": mean, "scale": float(1.0 / np.sqrt(var)) if var > 0.0 else 1.0})
    return out
