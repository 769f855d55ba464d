"""The reference fixtures of operator-ordered maintenance of the turbine (tests/golden/operator_turbine/*.npz,
tools/make_turbine_maintenance_golden.py): a trajectory fixture (golden_util.Golden) plus the script of perform_maintenance calls made
between its steps, with the reference's value of turb.* and tstg.* immediately before and after each, and the closure check's result per
call.  ot5_not_offered holds the calls of the handlers that are NOT offered: the device does not replay it."""
import collections
import glob
import os

import numpy as np

from golden_util import GOLDEN_DIR, Golden

SUBDIR = "operator_turbine"
KINDS = ("turbine", "bearing", "lubrication", "stage")
UNITS = {"turbine": 1, "bearing": 4, "lubrication": 1, "stage": 14}
THRUST = 2
# include/npb_maint.h NPB_TURBINE_ACTIONS: the index the fixtures' ops carry (held against the header and the library by
# tests/test_turbine_maintenance_abi.py)
ACTIONS = tuple(
    [("turbine", a) for a in ("turbine_performance_test", "turbine_system_optimization", "turbine_protection_test", "thermal_stress_analysis",
                              "vibration_analysis", "routine_maintenance")] +
    [("bearing", a) for a in ("turbine_bearing_inspection", "turbine_bearing_replacement", "bearing_clearance_check", "bearing_alignment",
                              "thrust_bearing_adjustment", "turbine_oil_change", "routine_maintenance")] +
    [("lubrication", a) for a in ("turbine_oil_change", "turbine_oil_top_off", "oil_filter_replacement", "oil_cooler_cleaning",
                                  "lubrication_system_test", "routine_maintenance")] +
    [("stage", a) for a in ("blade_replacement", "overhaul")])
NOT_OFFERED = (("stage", "cleaning"),)
REPLAYED = ("ot1_degraded_turbine", "ot2_stages", "ot3_as_built", "ot4_long_run")
REFUSED_FIXTURE = "ot5_not_offered"

# called: the kind of the object the reference's call was made on; action: catalog index (len(ACTIONS) = a type outside the catalog)
Op = collections.namedtuple("Op", "step called unit action success")


def turbine_fixture_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, SUBDIR, "*.npz")))


def order_succeeds(kind, name, unit):
    """what the reference's result says of a catalogued order"""
    return 0 <= unit < UNITS[kind] and not (name == "thrust_bearing_adjustment" and unit != THRUST)


class TurbineGolden(Golden):
    def __init__(self, name):
        super().__init__(os.path.join(SUBDIR, name))
        z = np.load(os.path.join(GOLDEN_DIR, SUBDIR, name + ".npz"), allow_pickle=False)
        self.ops = [Op(int(r[0]), KINDS[int(r[1])], int(r[2]), int(r[3]), bool(r[6])) for r in z["ops"]]
        self.op_names = [o["action"] for o in self.meta["ops"]]
        self.op_before, self.op_after = z["op_before"], z["op_after"]
        self.op_labels = [str(m) for m in z["op_labels"]]
        self.op_expect_change = z["op_expect_change"]
        self.op_closed = z["op_closed"]
        by_label = {lab: (kind, slot) for kind, slot, lab, _p in self.cols}
        self.op_slots = [by_label[m] for m in self.op_labels]

    def ops_at(self, step):
        """(index, op) of the calls made after `step` steps, in call order"""
        return [(j, o) for j, o in enumerate(self.ops) if o.step == step]

    def kind_name(self, o):
        """(turbine kind, maintenance type) of a catalogued call, (None, None) of one outside the catalog"""
        return ACTIONS[o.action] if o.action < len(ACTIONS) else (None, None)


# ---- scattered calls (tests/golden/operator_calls/turbine/, tools/make_scattered_turbine_calls_golden.py): a call stands alone
SCATTERED_SUBDIR = os.path.join("operator_calls", "turbine")
TurbineCall = collections.namedtuple("TurbineCall", "called unit action success explicit")


def scattered_turbine_fixture_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, SCATTERED_SUBDIR, "sc_turbine_*.npz")))


class ScatteredTurbineCalls:
    """the files as one list of calls, in the layout of scattered_calls_golden.ScatteredCalls: before / after (the reference's fp64 run) and
    before32 / after32 (its run from the float32-rounded values), [K, ncol] each; labels are schema labels of turb and tstg"""

    def __init__(self):
        import json
        from nuclear_sim_amd.schema import SCHEMA
        from scattered_calls_golden import same
        self.names = scattered_turbine_fixture_names()
        parts = [np.load(os.path.join(GOLDEN_DIR, SCATTERED_SUBDIR, n + ".npz"), allow_pickle=False) for n in self.names]
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
        self.calls = [TurbineCall(KINDS[int(r[0])], int(r[1]), int(r[2]), bool(r[4]), bool(r[5])) for r in np.concatenate([z["calls"] for z in parts])]
        self.written = [c for m in self.metas for c in m["calls"]]         # the calls as the generator wrote them
        self.col = {lab: j for j, lab in enumerate(self.labels)}
        by_label = {lab: (kind, slot) for kind, slot, lab, _p in SCHEMA.columns()}
        self.slots = [by_label[m] for m in self.labels]
        self._same = same
        for a in (self.before, self.after, self.before32, self.after32):
            a.setflags(write=False)

    def __len__(self):
        return len(self.calls)

    def changed(self, j, f32=False):
        return ~self._same(self.before32[j], self.after32[j]) if f32 else ~self._same(self.before[j], self.after[j])
