"""The reference fixtures of operator-ordered maintenance (tests/golden/operator/*.npz, tools/make_operator_maintenance_golden.py): a
trajectory fixture (golden_util.Golden) plus the script of perform_maintenance calls made between its steps, with the reference's value
of the ordered pump's section immediately before and after each call."""
import collections
import glob
import os

import numpy as np

from golden_util import GOLDEN_DIR, Golden

SUBDIR = "operator"
# the action types the lubrication system's dispatcher has a handler for (pump_lubrication.py:642-656)
HANDLERS = ("oil_change", "oil_top_off", "bearing_replacement", "seal_replacement", "component_overhaul", "system_cleaning",
            "bearing_inspection", "impeller_inspection", "impeller_replacement", "lubrication_system_check", "motor_inspection",
            "oil_analysis", "vibration_analysis")
# include/npb_maint.h NPB_MAINT_ACTIONS: the index the fixtures' ops carry (held against the library by tests/test_operator_maintenance_abi.py)
ACTIONS = ("oil_change", "oil_top_off", "lubrication_system_check", "impeller_inspection", "impeller_replacement", "cavitation_analysis",
           "npsh_analysis", "bearing_replacement", "seal_replacement", "vibration_analysis", "lubrication_inspection", "motor_inspection",
           "component_overhaul", "comprehensive_system_inspection", "bearing_inspection", "oil_analysis", "system_cleaning",
           "routine_maintenance")

Op = collections.namedtuple("Op", "step pump action action_name bearing target_level success")


def operator_fixture_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, SUBDIR, "*.npz")))


class OperatorGolden(Golden):
    def __init__(self, name):
        super().__init__(os.path.join(SUBDIR, name))
        z = np.load(os.path.join(GOLDEN_DIR, SUBDIR, name + ".npz"), allow_pickle=False)
        self.actions = list(ACTIONS)
        self.ops = [Op(int(r[0]), int(r[1]), int(r[2]), ACTIONS[int(r[2])], int(r[3]), float(r[4]), bool(r[5])) for r in z["ops"]]
        self.op_before, self.op_after = z["op_before"], z["op_after"]
        self.op_labels = [str(m) for m in z["op_labels"]]
        self.op_expect_change = z["op_expect_change"]

    def ops_at(self, step):
        """(index, op) of the calls made after `step` steps, in call order"""
        return [(j, o) for j, o in enumerate(self.ops) if o.step == step]

    def pump_slots(self, pump):
        """(kind, slot) of each op_labels member of pump `pump`"""
        by_label = {lab: (kind, slot) for kind, slot, lab, _p in self.cols}
        return [by_label["pump[%d].%s" % (pump, m)] for m in self.op_labels]
