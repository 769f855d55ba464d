"""The reference fixtures of operator-ordered maintenance of steam generators and condenser (tests/golden/operator_components/*.npz,
tools/make_component_maintenance_golden.py): a trajectory fixture (golden_util.Golden) plus the script of perform_maintenance calls made
between its steps, with the reference's value of the sections a call may touch (sg[0..2], chem[0..1], cond, sec) immediately before and
after each, and the closure check's result per call."""
import collections
import glob
import os

import numpy as np

from golden_util import GOLDEN_DIR, Golden

SUBDIR = "operator_components"
KINDS = ("steam_generator", "steam_generator_system", "condenser", "ejector")
UNITS = {"steam_generator": 3, "steam_generator_system": 1, "condenser": 1, "ejector": 2}
# include/npb_maint.h NPB_COMPONENT_ACTIONS: the index the fixtures' ops carry (held against the header and the library by
# tests/test_component_maintenance_abi.py)
ACTIONS = tuple(
    [("steam_generator", a) for a in (
        "tsp_chemical_cleaning", "tsp_mechanical_cleaning", "tube_bundle_inspection", "moisture_separator_maintenance", "scale_removal",
        "water_chemistry_adjustment", "secondary_side_cleaning", "tsp_inspection", "tsp_flow_test", "tube_interior_inspection",
        "tube_interior_scale_cleaning", "tube_interior_eddy_current_testing", "primary_chemistry_optimization", "primary_scale_cleaning",
        "tube_eddy_current_testing", "routine_maintenance")] +
    [("steam_generator_system", a) for a in (
        "system_coordination_maintenance", "system_steam_quality_maintenance", "load_balancing_maintenance", "routine_maintenance")] +
    [("condenser", a) for a in (
        "condenser_tube_cleaning", "condenser_chemical_cleaning", "condenser_water_treatment", "vacuum_system_test", "vacuum_leak_detection")] +
    [("ejector", a) for a in (
        "vacuum_ejector_cleaning", "vacuum_ejector_nozzle_replacement", "vacuum_ejector_inspection", "vacuum_ejector_mechanical_cleaning",
        "routine_maintenance", "general")])
CLEANING_NAMES = {0: None, 1: "chemical", 2: "mechanical", 3: "hydroblast", 4: "replacement", 5: "some_other_method"}

# called: the kind of the object the reference's call was made on; unit: generator / ejector (for a call the system delegated, the
# generator its sg_index names); action: catalog index (len(ACTIONS) = a type outside the catalog); sg_index: -1 = none given
Op = collections.namedtuple("Op", "step called unit action cleaning tubes_to_plug success sg_index")


def component_fixture_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, SUBDIR, "*.npz")))


class ComponentGolden(Golden):
    def __init__(self, name):
        super().__init__(os.path.join(SUBDIR, name))
        z = np.load(os.path.join(GOLDEN_DIR, SUBDIR, name + ".npz"), allow_pickle=False)
        self.ops = [Op(int(r[0]), KINDS[int(r[1])], int(r[2]), int(r[3]), int(r[4]), float(r[5]), bool(r[6]), int(r[7])) for r in z["ops"]]
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
        """(component kind, maintenance type) of a catalogued call, (None, None) of one outside the catalog"""
        return ACTIONS[o.action] if o.action < len(ACTIONS) else (None, None)
