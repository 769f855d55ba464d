"""The reference fixtures of scattered operator calls (tests/golden/operator_calls/*.npz, tools/make_scattered_calls_golden.py): per call
the reference's value of every schema member of the sections it may touch immediately before and after it, from a seeded draw of those
members, and the same again from the float32-rounded values.  No trajectory: a call stands alone."""
import collections
import glob
import json
import os

import numpy as np

from golden_util import GOLDEN_DIR
from nuclear_sim_amd.schema import SCHEMA

SUBDIR = "operator_calls"

ComponentCall = collections.namedtuple("ComponentCall", "called unit action cleaning success explicit")
PumpCall = collections.namedtuple("PumpCall", "pump action bearing target_level success explicit via target_is_level")


def scattered_fixture_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, SUBDIR, "*.npz")))


def same(a, b):
    """equal to the bit, NaN equal to NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


class ScatteredCalls:
    """the files of one kind ("components" / "pumps") as one list of calls: before / after (the reference's fp64 run) and before32 / after32
    (its run from the float32-rounded values), [K, ncol] each; labels are schema labels (components) or pump member names (pumps)"""

    def __init__(self, kind):
        self.kind = kind
        self.names = [n for n in scattered_fixture_names() if n.startswith("sc_%s_" % kind)]
        parts = [np.load(os.path.join(GOLDEN_DIR, SUBDIR, n + ".npz"), allow_pickle=False) for n in self.names]
        self.metas = [json.loads(str(z["meta"])) for z in parts]
        self.labels = [str(m) for m in parts[0]["labels"]]
        self.kinds = [str(m) for m in parts[0]["kinds"]]
        assert all([str(m) for m in z["labels"]] == self.labels for z in parts)
        before, after, before32, after32 = [], [], [], []
        real = np.array([k == "f64" for k in self.kinds])
        for z in parts:
            b = z["before"]
            a = b.copy(); a[z["after_at"][:, 0], z["after_at"][:, 1]] = z["after_val"]
            b32 = np.where(real[None, :], b.astype(np.float32).astype(np.float64), b)
            a32 = b32.copy(); a32[z["after32_at"][:, 0], z["after32_at"][:, 1]] = z["after32_val"]
            before.append(b); after.append(a); before32.append(b32); after32.append(a32)
        self.before, self.after = np.concatenate(before), np.concatenate(after)
        self.before32, self.after32 = np.concatenate(before32), np.concatenate(after32)
        self.expect_change = np.concatenate([z["expect_change"] for z in parts])
        rows = np.concatenate([z["calls"] for z in parts])
        if kind == "components":
            self.calls = [ComponentCall(int(r[0]), int(r[1]), int(r[2]), int(r[3]), bool(r[4]), bool(r[5])) for r in rows]
        else:
            self.calls = [PumpCall(int(r[0]), int(r[1]), int(r[2]), float(r[3]), bool(r[4]), bool(r[5]), int(r[6]), bool(r[7])) for r in rows]
        self.written = [c for m in self.metas for c in m["calls"]]         # the calls as the generator wrote them
        self.dropped = [d for d in self.metas[0]["dropped"]]
        self.col = {lab: j for j, lab in enumerate(self.labels)}
        for a in (self.before, self.after, self.before32, self.after32):
            a.setflags(write=False)

    def __len__(self):
        return len(self.calls)

    def changed(self, j, f32=False):
        return ~same(self.before32[j], self.after32[j]) if f32 else ~same(self.before[j], self.after[j])

    def slots(self, pump=None):
        """(kind, slot) of every label; for the pump fixture, of pump `pump`'s members"""
        by_label = {lab: (kind, slot) for kind, slot, lab, _p in SCHEMA.columns()}
        return [by_label[m if pump is None else "pump[%d].%s" % (pump, m)] for m in self.labels]
