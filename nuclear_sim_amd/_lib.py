"""ctypes binding of libnpb.so (the HIP stepper's C ABI, include/npb.h).

There is no CPU fallback: if the shared library is missing or does not load, importing
this module raises.  Build it with ``make -C nuclear_sim_amd/csrc`` (or
``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from .orders_abi import CONTROL_ORDER_NEVER, CONTROL_ORDERS_MAX, ORDER_FAMILIES, NpbControlOrder, NpbControlOrdersDesc
from .ppo_abi import PPO_SHARD_ROWS, PPO_SHARDS_MAX, PPO_STATS_MORE, NpbPpoMore, NpbPpoShards
from .recurrent_abi import POLICY_GATES, NpbPolicyCore, NpbPpoSeq, NpbPpoSegments
from .schema import PARAMS, SCHEMA

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NPB_LIB", os.path.join(_HERE, "libnpb.so"))

NPB_KIND_F64, NPB_KIND_I32 = 0, 1
HEAT_CONSTANT, HEAT_REACTOR, HEAT_EXTERNAL = 0, 1, 2
STORAGE_F64, STORAGE_F32 = 0, 1
MODE_FULL, MODE_PRIMARY_SG, MODE_PRIMARY = 0, 1, 2
OBS_DIM, INFO_DIM = 22, 17   # include/npb.h NPB_OBS_DIM / NPB_INFO_DIM; checked against the library in load()
INFO_NRHO = 10   # include/npb.h NPB_INFO_NRHO
# include/npb.h NPB_DIAG_*: step-internal diagnostics, fourteen turbine stages each (TurbineStage.get_state_dict, stage_system.py:379-393)
DIAG_STAGE_VALUES = ("inlet_pressure", "inlet_temperature", "outlet_pressure", "outlet_temperature", "power_output", "loading_factor")
DIAG_SG_VALUES = ("primary_inlet_temp", "primary_outlet_temp", "overall_htc", "feedwater_flow_rate")   # steam_generator.py:943-985
DIAG_PUMP_VALUES = ("system_health_factor", "maintenance_action_occurred", "oil_top_off_occurred")   # per pump, FWP-1..4 (NPB_DIAG_PUMP_*)
DIAG_FW_VALUES = ("feedwater_avg_sg_level", "feedwater_avg_sg_pressure", "feedwater_total_steam_flow", "feedwater_avg_steam_quality")   # NPB_DIAG_FW_*
DIAG_ROTOR_VALUES = ("friction_torque", "net_torque", "rotor_acceleration")   # NPB_DIAG_ROTOR_*
# NPB_DIAG_COND_*, NPB_DIAG_SG_SCALE_FORMATION_RATE (x3), NPB_DIAG_FW_PERFORMANCE_FACTOR: (log column, row offset behind the rotor's)
DIAG_TAIL_COLUMNS = (("secondary.condenser_SECONDARY-COMP-001-COND.condenser_overall_htc", 0), ("secondary.condenser_SECONDARY-COMP-001-COND.tube_leak_rate", 1),
                     ("secondary.condenser.SJE-001_steam_flow", 2), ("secondary.condenser.SJE-001_steam_consumption", 3),
                     ("secondary.condenser.vacuum_system_steam_consumption", 4),
                     ("secondary.steam_generator_SG-0.tube_scale_formation_rate_mm_per_year", 5), ("secondary.steam_generator_SG-1.tube_scale_formation_rate_mm_per_year", 6),
                     ("secondary.steam_generator_SG-2.tube_scale_formation_rate_mm_per_year", 7),
                     ("secondary.feedwater_SECONDARY-COMP-001-FW.feedwater_performance_factor", 8),
                     # accumulators (NPB_DIAG_ROTOR_CLEARANCE_INCREASE x4, NPB_DIAG_ROTOR_OVERSPEED_EVENTS): since the diagnostics were switched on
                     ("secondary.turbine_SECONDARY-COMP-001-TURB.TB-001_clearance_increase", 9), ("secondary.turbine_SECONDARY-COMP-001-TURB.TB-002_clearance_increase", 10),
                     ("secondary.turbine_SECONDARY-COMP-001-TURB.TB-003_clearance_increase", 11), ("secondary.turbine_SECONDARY-COMP-001-TURB.TB-004_clearance_increase", 12),
                     ("secondary.turbine_SECONDARY-COMP-001-TURB.overspeed_events", 13),
                     # NPB_DIAG_BEARING_OIL_TEMP x4
                     ("secondary.turbine_SECONDARY-COMP-001-TURB.TB-001_oil_temp", 14), ("secondary.turbine_SECONDARY-COMP-001-TURB.TB-002_oil_temp", 15),
                     ("secondary.turbine_SECONDARY-COMP-001-TURB.TB-003_oil_temp", 16), ("secondary.turbine_SECONDARY-COMP-001-TURB.TB-004_oil_temp", 17),
                     # offset 18 = NPB_DIAG_STAGE_SYSTEM_EFFICIENCY: carried from step to step, not a log column of the reference's;
                     # NPB_DIAG_TURBINE_PERFORMANCE_FACTOR, NPB_DIAG_FW_ACTIVE_ALARMS
                     ("secondary.turbine_SECONDARY-COMP-001-TURB.enhanced_turbine_performance", 19),
                     ("secondary.feedwater_SECONDARY-COMP-001-FW.protection_active_alarms_count", 20))
# round 4 (include/npb.h NPB_DIAG_PUMP_MAINTENANCE_ACTION ...): rows by number
DIAG_PUMP_MAINTENANCE_ACTION = 136          # x4: catalog index + 1 of the action carried out on the pump in this step, 0 = none
DIAG_FW_ACTIVE_TRIPS, DIAG_FW_VALID_TRIP_COUNT, DIAG_FW_EMERGENCY_FEEDWATER, DIAG_FW_STEAM_DUMP = 140, 141, 142, 143
DIAG_STAGE_EXTRACTION_FLOW = 144            # x14
DIAG_COND_SJE_CAPACITY, DIAG_COND_SJE_STEAM_FLOW, DIAG_COND_SJE_STEAM_CONSUMPTION = 158, 160, 162    # x2 each
DIAG_COND_SJE_COMPRESSION_RATIO, DIAG_COND_SJE_OPERATING_HOURS, DIAG_COND_AIR_REMOVAL = 164, 166, 168
DIAG_STAGE_SYSTEM_TOTAL_POWER = 169
DIAG_STAGE_POWER_OUTPUT = 56                # x14 (NPB_DIAG_STAGE_POWER_OUTPUT)
# rows the step CARRIES in the caller's buffer from one step to the next (accumulators, latches, values kept while equipment
# rests): row -> value of a freshly constructed plant, in the order of include/npb.h NPB_DIAG_CARRIED (checked against the library in
# load(); the rows of BatchedPlantEnv.diagnostics_state()).  BatchedPlantEnv.enable_diagnostics / reset put them there.
DIAG_CARRIED_ROWS = {**{124 + q: 0.0 for q in range(5)}, 133: 0.0, DIAG_FW_VALID_TRIP_COUNT: 0.0, DIAG_FW_EMERGENCY_FEEDWATER: 0.0,
                     DIAG_FW_STEAM_DUMP: 0.0, DIAG_COND_SJE_COMPRESSION_RATIO: 1.0, DIAG_COND_SJE_COMPRESSION_RATIO + 1: 1.0,
                     DIAG_COND_SJE_OPERATING_HOURS: 0.0, DIAG_COND_SJE_OPERATING_HOURS + 1: 0.0}
DIAG_DIM = 170
assert 14 * len(DIAG_STAGE_VALUES) + 3 * len(DIAG_SG_VALUES) + 4 * len(DIAG_PUMP_VALUES) + len(DIAG_FW_VALUES) + len(DIAG_ROTOR_VALUES) + len(DIAG_TAIL_COLUMNS) + 1 == DIAG_PUMP_MAINTENANCE_ACTION
REACTIVITY_COMPONENTS = ("control_rods", "boron", "doppler", "moderator_temp", "moderator_void", "pressure", "xenon", "samarium",
                         "fuel_depletion", "burnable_poisons")   # reactivity_model.py:87-121, NPB_RHO_*


class NpbError(RuntimeError):
    pass


def _make_params_struct():
    fields = [(name, ctypes.c_double) for name, _d, _p in PARAMS]
    fields += [("dt", ctypes.c_double), ("heat_source", ctypes.c_int), ("hs_noise_enabled", ctypes.c_int),
               ("mode", ctypes.c_int), ("maint_enabled", ctypes.c_int), ("info_reactivity_components", ctypes.c_int), ("kinetics_rk4_substeps", ctypes.c_int)]
    return type("NpbParams", (ctypes.Structure,), {"_fields_": fields})


NpbParams = _make_params_struct()

MAINT_NPARAM, MAINT_NACT = 16, 18


class NpbMaintTable(ctypes.Structure):
    """npb_maint_table_t (include/npb_maint.h): one row per catalogued threshold parameter"""
    _fields_ = [("threshold", ctypes.c_double * MAINT_NPARAM), ("cooldown_hours", ctypes.c_double * MAINT_NPARAM),
                ("rank", ctypes.c_int * MAINT_NPARAM), ("comparison", ctypes.c_int * MAINT_NPARAM),
                ("action", ctypes.c_int * MAINT_NPARAM), ("priority", ctypes.c_int * MAINT_NPARAM),
                ("bearing", ctypes.c_int * MAINT_NPARAM)]


def __getattr__(name):
    """MAINT_PARAMS / MAINT_ACTIONS: the catalogs of include/npb_maint.h, read from the library itself (npb_maint_param_name /
    npb_maint_action_name) the first time they are asked for -- the package needs no header beside it."""
    if name in ("MAINT_PARAMS", "MAINT_ACTIONS"):
        L = load()
        params = [L.npb_maint_param_name(k).decode() for k in range(L.npb_maint_num_params())]
        actions = [L.npb_maint_action_name(a).decode() for a in range(L.npb_maint_num_actions())]
        if len(params) != MAINT_NPARAM or len(actions) != MAINT_NACT:
            raise NpbError("libnpb.so's maintenance catalogs (%d parameters, %d actions) are not the %d / %d this binding's "
                           "NpbMaintTable is laid out for: rebuild" % (len(params), len(actions), MAINT_NPARAM, MAINT_NACT))
        if tuple(actions) != MAINT_ACTION_NAMES:
            raise NpbError("libnpb.so's action catalog is not this binding's MAINT_ACTION_NAMES: rebuild")
        globals()["MAINT_PARAMS"], globals()["MAINT_ACTIONS"] = params, actions
        return globals()[name]
    raise AttributeError(name)


MAINT_COMPARISONS = ("greater_than", "less_than", "greater_equal", "less_equal", "equals", "not_equals")
MAINT_PRIORITIES = {"LOW": 1, "MEDIUM": 2, "HIGH": 3, "CRITICAL": 4, "EMERGENCY": 5}
MAINT_BEARINGS = {None: 0, "all": 0, "motor_bearings": 1, "pump_bearings": 2, "thrust_bearing": 3}
MAINT_ACTION_NONE = -1     # npb_perform_maintenance: nothing ordered for this plant
# include/npb_maint.h NPB_MAINT_ACTIONS, for the checks that must not need the library (an unknown name is refused before any device
# is looked for); load() holds it against the library's own catalog
MAINT_ACTION_NAMES = ("oil_change", "oil_top_off", "lubrication_system_check", "impeller_inspection", "impeller_replacement",
                      "cavitation_analysis", "npsh_analysis", "bearing_replacement", "seal_replacement", "vibration_analysis",
                      "lubrication_inspection", "motor_inspection", "component_overhaul", "comprehensive_system_inspection",
                      "bearing_inspection", "oil_analysis", "system_cleaning", "routine_maintenance")
PUMP_IDS = ("FWP-1", "FWP-2", "FWP-3", "FWP-4")


def maint_action_index(action) -> int:
    """an action name of the catalog, or an index, -> index; ValueError for an unknown name (host only, no library needed)"""
    if isinstance(action, str):
        if action not in MAINT_ACTION_NAMES:
            raise ValueError("unknown maintenance action %r: not in the action catalog (include/npb_maint.h)" % (action,))
        return MAINT_ACTION_NAMES.index(action)
    return int(action)


# include/npb_maint.h NPB_COMPONENT_ACTIONS: the catalog of npb_perform_component_maintenance, (component kind, maintenance type) per
# index -- a type string may occur under several kinds ("routine_maintenance"), the index names one handler; load() holds it
# against the library's own catalog
COMPONENT_KINDS = ("steam_generator", "steam_generator_system", "condenser", "ejector")
COMPONENT_ACTIONS = tuple(
    [("steam_generator", a) for a in (
        "tsp_chemical_cleaning", "tsp_mechanical_cleaning", "tube_bundle_inspection", "moisture_separator_maintenance", "scale_removal",
        "water_chemistry_adjustment", "secondary_side_cleaning", "tsp_inspection", "tsp_flow_test",
        "tube_interior_inspection", "tube_interior_scale_cleaning", "tube_interior_eddy_current_testing", "primary_chemistry_optimization",
        "primary_scale_cleaning", "tube_eddy_current_testing", "routine_maintenance")] +
    [("steam_generator_system", a) for a in (
        "system_coordination_maintenance", "system_steam_quality_maintenance", "load_balancing_maintenance", "routine_maintenance")] +
    [("condenser", a) for a in (
        "condenser_tube_cleaning", "condenser_chemical_cleaning", "condenser_water_treatment", "vacuum_system_test", "vacuum_leak_detection")] +
    [("ejector", a) for a in (
        "vacuum_ejector_cleaning", "vacuum_ejector_nozzle_replacement", "vacuum_ejector_inspection", "vacuum_ejector_mechanical_cleaning",
        "routine_maintenance", "general")])
COMPONENT_UNITS = {"steam_generator": 3, "steam_generator_system": 1, "condenser": 1, "ejector": 2}
EJECTOR_IDS = ("SJE-001", "SJE-002")
# the cleaning_type kwarg as npb_perform_component_maintenance's option column carries it (NPB_CLEANING_*); a string that is none of
# these is the handlers' "anything else" branch
CLEANING_TYPES = {None: 0, "chemical": 1, "mechanical": 2, "hydroblast": 3, "replacement": 4}
CLEANING_OTHER = 5
# handlers of the reference that are NOT offered, with the reason (DESIGN.md "Operator-ordered maintenance of steam generators and
# condenser"): refused by name, with this message, apart from an unknown name
COMPONENT_ACTIONS_NOT_OFFERED = {
    ("steam_generator", "eddy_current_testing"):
        "the reference's handler raises KeyError ('operating_years' is not a key of TSPFoulingModel.get_state_dict, "
        "steam_generator/steam_generator.py:1224): there is no result to restate",
    ("condenser", "condenser_tube_plugging"):
        "the reference's handler raises AttributeError ('CondenserConfig' object has no attribute 'tube_count', condenser/physics.py:1245) "
        "after it has moved the tube counts: there is no result to restate",
}


def component_action_index(component, action) -> int:
    """(component kind, maintenance type name or index) -> index into COMPONENT_ACTIONS; ValueError for an unknown kind or name, and for
    a handler that is not offered (host only, no library needed).  An index is taken as it is."""
    if component not in COMPONENT_KINDS:
        raise ValueError("unknown component %r: one of %r" % (component, COMPONENT_KINDS))
    if not isinstance(action, str):
        return int(action)
    if (component, action) in COMPONENT_ACTIONS_NOT_OFFERED:
        raise ValueError("%s maintenance %r is not offered on the device: %s" % (component, action, COMPONENT_ACTIONS_NOT_OFFERED[(component, action)]))
    if (component, action) not in COMPONENT_ACTIONS:
        raise ValueError("unknown %s maintenance %r: not in the component catalog (include/npb_maint.h)" % (component, action))
    return COMPONENT_ACTIONS.index((component, action))


# include/npb_maint.h NPB_TURBINE_ACTIONS: the catalog of npb_perform_turbine_maintenance, (turbine kind, maintenance type) per index;
# load() holds it against the library's own catalog.  Kinds: the turbine itself (EnhancedTurbinePhysics), one of its four bearings, its
# bearing-lubrication system, one of its fourteen stages.
TURBINE_KINDS = ("turbine", "bearing", "lubrication", "stage")
TURBINE_ACTIONS = tuple(
    [("turbine", a) for a in (
        "turbine_performance_test", "turbine_system_optimization", "turbine_protection_test", "thermal_stress_analysis", "vibration_analysis",
        "routine_maintenance")] +
    [("bearing", a) for a in (
        "turbine_bearing_inspection", "turbine_bearing_replacement", "bearing_clearance_check", "bearing_alignment", "thrust_bearing_adjustment",
        "turbine_oil_change", "routine_maintenance")] +
    [("lubrication", a) for a in (
        "turbine_oil_change", "turbine_oil_top_off", "oil_filter_replacement", "oil_cooler_cleaning", "lubrication_system_test",
        "routine_maintenance")] +
    [("stage", a) for a in ("blade_replacement", "overhaul")])
TURBINE_UNITS = {"turbine": 1, "bearing": 4, "lubrication": 1, "stage": 14}
TURBINE_THRUST_BEARING = 2     # thrust_bearing_adjustment succeeds on this bearing only (rotor_dynamics.py:829)
# handlers of the reference that are NOT offered because they are not closed over the carried state (DESIGN.md "Operator-ordered
# maintenance of the turbine"; tests/golden/operator_turbine/ot5_not_offered.npz): refused by name, with this message
TURBINE_ACTIONS_NOT_OFFERED = {
    ("stage", "cleaning"):
        "the reference's handler resets the stage's fouling_factor but leaves its blade_condition_factor and actual_efficiency at the "
        "values of the fouled stage (turbine/stage_system.py:353-359); the next step's expansion reads both (:221-224) before it derives "
        "them anew (:321-326), and no schema column carries them",
}


def turbine_action_index(component, action) -> int:
    """(turbine kind, maintenance type name or index) -> index into TURBINE_ACTIONS; ValueError for an unknown kind or name, and for a
    handler that is not offered (host only, no library needed).  An index is taken as it is."""
    if component not in TURBINE_KINDS:
        raise ValueError("unknown turbine component %r: one of %r" % (component, TURBINE_KINDS))
    if not isinstance(action, str):
        return int(action)
    if (component, action) in TURBINE_ACTIONS_NOT_OFFERED:
        raise ValueError("%s maintenance %r is not offered on the device: %s" % (component, action, TURBINE_ACTIONS_NOT_OFFERED[(component, action)]))
    if (component, action) not in TURBINE_ACTIONS:
        raise ValueError("unknown %s maintenance %r: not in the turbine catalog (include/npb_maint.h)" % (component, action))
    return TURBINE_ACTIONS.index((component, action))


def cleaning_type_index(cleaning_type) -> int:
    """the reference's cleaning_type kwarg -> NPB_CLEANING_*; an index is taken as it is"""
    if cleaning_type is None or isinstance(cleaning_type, str):
        return CLEANING_TYPES.get(cleaning_type, CLEANING_OTHER)
    return int(cleaning_type)


def maint_table_from_thresholds(thresholds: dict) -> "NpbMaintTable":
    """The reference's thresholds dict of a feedwater pump (maintenance_system.component_configs.feedwater.thresholds of
    the configuration, = StateManager.maintenance_thresholds['FWP-1'], in ITS order) -> table.  Names that do not
    resolve in a pump's state log are dropped, as the reference's scan drops them (state_manager.py:1371-1411)."""
    t = NpbMaintTable()
    MAINT_PARAMS, MAINT_ACTIONS = __getattr__("MAINT_PARAMS"), __getattr__("MAINT_ACTIONS")
    for k in range(MAINT_NPARAM):
        t.rank[k] = -1
    for rank, (name, cfg) in enumerate(thresholds.items()):
        if name not in MAINT_PARAMS or cfg.get("threshold") is None:
            continue
        k = MAINT_PARAMS.index(name)
        action = cfg.get("action")
        if action not in MAINT_ACTIONS:
            raise NpbError("maintenance action %r of threshold %r is not in the action catalog (include/npb_maint.h)" % (action, name))
        t.rank[k] = rank
        t.threshold[k] = float(cfg["threshold"])
        t.cooldown_hours[k] = float(cfg.get("cooldown_hours", 24.0))
        t.comparison[k] = MAINT_COMPARISONS.index(cfg.get("comparison", "greater_than"))
        t.action[k] = MAINT_ACTIONS.index(action)
        t.priority[k] = MAINT_PRIORITIES.get(str(cfg.get("priority", "MEDIUM")).upper(), 2)
        t.bearing[k] = MAINT_BEARINGS.get(cfg.get("component_id"), 0)
    return t

# include/npb_maint.h NPB_CMAINT_PARAMS: the rows of the automatic maintenance of steam generators and condenser
# (npb_set_component_maintenance), (component kind, name in the state log) per index; load() holds it against the library's own catalog
CMAINT_PARAMS = (("steam_generator", "tsp_fouling_fraction"), ("steam_generator", "tube_wall_temperature"), ("steam_generator", "steam_quality"),
                 ("condenser", "fouling_resistance"), ("condenser", "tube_leak_rate"))
# the one action a row may name from outside COMPONENT_ACTIONS (NPB_CA_AUTO_CONDENSER_TUBE_PLUGGING): the composer's tube_leak_rate row orders
# condenser_tube_plugging, whose handler raises in the reference; as a work order it is created, counted and completed without success
CMAINT_AUTO_ACTIONS = {("condenser", "condenser_tube_plugging"): len(COMPONENT_ACTIONS)}
CMAINT_NPARAM = len(CMAINT_PARAMS)
CMAINT_COMPONENTS = ("SG-0", "SG-1", "SG-2", "condenser")      # the scan order behind FWP-1..4; slot = component * CMAINT_NROW + row
CMAINT_NROW = 3
CMAINT_STATE_MEMBERS = ("last_violation_time", "wo_order", "wo_created", "wo_planned_start", "wo_priority", "last_trigger_time")   # NPB_CMS_*
CMAINT_SIDE_DOUBLES = len(CMAINT_STATE_MEMBERS) * len(CMAINT_COMPONENTS) * CMAINT_NROW
# rows of the reference's configuration for these components whose parameter never resolves in the component's state-log row
# (StateManager._find_parameter_in_row_data gives None: never compared): dropped, as the reference's scan drops them
CMAINT_ROWS_UNRESOLVED = {"steam_generator": ("efficiency",), "condenser": ("tube_cleanliness", "vacuum_level", "thermal_performance_factor")}
# rows that DO resolve on the reference and are not scanned on the device, with the reason (DESIGN.md "Automatic maintenance of steam
# generators and condenser"): dropped by component_maint_table_from_thresholds
CMAINT_ROWS_NOT_SCANNED = {}
# component kinds of the reference's configuration whose rows are not scanned, with the measured reason: a table that carries one is refused
_TURBINE_REASON = ("the only row of the turbine's stages and of the turbine that resolves on the reference is `efficiency` (< 0.30, efficiency_analysis), "
                   "and the reference cannot fire it: every step leaves a stage's actual_efficiency at max(0.7, design - degradation) "
                   "(turbine/stage_system.py:323-326), 0.7 at the lowest with the degradation, deposits and blade wear poked to their worst "
                   "(tests/golden/auto_components/silent_rows.json, turbine_efficiency_probe); a table with a turbine row that could fire "
                   "would need the stages in the scan, which they are not")
CMAINT_KINDS_NOT_SCANNED = {"turbine": _TURBINE_REASON, "turbine_stage": _TURBINE_REASON}


class NpbComponentMaintTable(ctypes.Structure):
    """npb_component_maint_table_t (include/npb_maint.h): one row per parameter of CMAINT_PARAMS, the generators' rows shared by SG-0..2"""
    _fields_ = [("threshold", ctypes.c_double * CMAINT_NPARAM), ("cooldown_hours", ctypes.c_double * CMAINT_NPARAM),
                ("rank", ctypes.c_int * CMAINT_NPARAM), ("comparison", ctypes.c_int * CMAINT_NPARAM),
                ("action", ctypes.c_int * CMAINT_NPARAM), ("priority", ctypes.c_int * CMAINT_NPARAM)]


def component_maint_table_from_thresholds(thresholds: dict) -> "NpbComponentMaintTable":
    """{"steam_generator": {...}, "condenser": {...}} -- each the reference's thresholds dict of that component
    (StateManager.maintenance_thresholds['SG-0'] / ['SECONDARY-COMP-001-COND'], in ITS order) -> table (host only, no library needed).  A
    missing kind has no rows.  Rows of CMAINT_ROWS_UNRESOLVED and CMAINT_ROWS_NOT_SCANNED are dropped; any other name outside
    CMAINT_PARAMS, a comparison or priority the reference does not know, and an action outside that component's part of
    COMPONENT_ACTIONS are refused (NpbError)."""
    t = NpbComponentMaintTable()
    for k in range(CMAINT_NPARAM):
        t.rank[k] = -1
    for kind, rows in thresholds.items():
        if kind in CMAINT_KINDS_NOT_SCANNED:
            raise NpbError("component thresholds of %r are not scanned on the device: %s" % (kind, CMAINT_KINDS_NOT_SCANNED[kind]))
        if kind not in ("steam_generator", "condenser"):
            raise NpbError("component thresholds of %r: the automatic maintenance covers 'steam_generator' and 'condenser'" % (kind,))
        for rank, (name, cfg) in enumerate(rows.items()):
            if name in CMAINT_ROWS_UNRESOLVED[kind] or (kind, name) in CMAINT_ROWS_NOT_SCANNED or cfg.get("threshold") is None:
                continue
            if (kind, name) not in CMAINT_PARAMS:
                raise NpbError("unknown %s threshold parameter %r: not in the component parameter catalog (include/npb_maint.h NPB_CMAINT_PARAMS)" % (kind, name))
            k = CMAINT_PARAMS.index((kind, name))
            action, comparison = cfg.get("action"), cfg.get("comparison", "greater_than")
            if (kind, action) not in COMPONENT_ACTIONS and (kind, action) not in CMAINT_AUTO_ACTIONS:
                raise NpbError("maintenance action %r of %s threshold %r is not in the component catalog (include/npb_maint.h)" % (action, kind, name))
            if comparison not in MAINT_COMPARISONS:
                raise NpbError("unknown comparison %r of %s threshold %r" % (comparison, kind, name))
            t.rank[k] = rank
            t.threshold[k] = float(cfg["threshold"])
            t.cooldown_hours[k] = float(cfg.get("cooldown_hours", 24.0))
            t.comparison[k] = MAINT_COMPARISONS.index(comparison)
            t.action[k] = CMAINT_AUTO_ACTIONS[(kind, action)] if (kind, action) in CMAINT_AUTO_ACTIONS else COMPONENT_ACTIONS.index((kind, action))
            t.priority[k] = MAINT_PRIORITIES.get(str(cfg.get("priority", "MEDIUM")).upper(), 2)
    return t


# include/npb.h NPB_SAMPLE_*: element types of a sampler's side sources
SAMPLE_TYPES = {"f64": 0, "f32": 1, "i32": 2, "u8": 3}


class NpbSampleSource(ctypes.Structure):
    """npb_sample_source_t (include/npb.h): a caller-owned device buffer of per-plant rows, strides in elements"""
    _fields_ = [("base", ctypes.c_void_p), ("type", ctypes.c_int), ("rows", ctypes.c_int),
                ("row_stride", ctypes.c_int64), ("plant_stride", ctypes.c_int64)]


class NpbSamplerDesc(ctypes.Structure):
    """npb_sampler_desc_t (include/npb.h): the request of npb_sampler_create; every array on the host"""
    _fields_ = [("n_watched", ctypes.c_int), ("plants", ctypes.POINTER(ctypes.c_int32)),
                ("n_fields", ctypes.c_int), ("kinds", ctypes.POINTER(ctypes.c_int)), ("slots", ctypes.POINTER(ctypes.c_int)),
                ("n_sources", ctypes.c_int), ("sources", ctypes.POINTER(NpbSampleSource))]


# include/npb_maint.h npb_maint_summary_desc_t: the per-plant work-order summary (npb_set_maintenance_summary)
SUMMARY_MAX_KEYS = 16
SUMMARY_CATALOGS = ("feedwater", "component", "turbine")      # NPB_MAINT_CATALOG_*
# the record kinds (NPB_MAINT_EVENT_*) of each catalog: (work-order kinds, operator kinds); every kind of a catalog but its creation
# kind feeds the completed pair
SUMMARY_KINDS = {"feedwater": ((0, 1), (2,)), "component": ((5, 6), (3,)), "turbine": ((), (4,))}
SUMMARY_CREATION_KINDS = (0, 5)


class NpbMaintSummaryKey(ctypes.Structure):
    """npb_maint_summary_key_t"""
    _fields_ = [("catalog", ctypes.c_int32), ("action", ctypes.c_int32), ("unit", ctypes.c_int32), ("kinds", ctypes.c_uint32)]


class NpbMaintSummaryDesc(ctypes.Structure):
    """npb_maint_summary_desc_t: the keys, the caller's four [n_keys][n_plants] device tables and its two bookkeeping words"""
    _fields_ = [("n_keys", ctypes.c_int32), ("consume", ctypes.c_int32), ("since_minutes", ctypes.c_double),
                ("keys", NpbMaintSummaryKey * SUMMARY_MAX_KEYS),
                ("first_created", ctypes.c_void_p), ("first_completed", ctypes.c_void_p),
                ("n_created", ctypes.c_void_p), ("n_completed", ctypes.c_void_p),
                ("folded", ctypes.c_void_p), ("dropped", ctypes.c_void_p)]


def summary_key(key, operator: bool = False):
    """One key of ``BatchedPlantEnv.enable_maintenance_summary`` -> (catalog, action, unit, kinds) as npb_maint_summary_key_t holds them
    (host only, no library needed).  ``key`` is a plain action name of the feedwater catalog, or (catalog_name, action_name_or_None,
    unit_or_None); a component or turbine action may be given as (kind, name), as ``component_action_index`` / ``turbine_action_index``
    take it, since a bare name can occur under several kinds; an index is taken as it is.  The kinds are the work-order kinds of the
    catalog; ``operator`` adds the operator kinds.  ValueError for an unknown catalog or name and for a key that can match nothing (the
    turbine has no work orders: its keys need ``operator=True``)."""
    if isinstance(key, str):
        key = ("feedwater", key, None)
    catalog, action, unit = key
    if catalog not in SUMMARY_CATALOGS:
        raise ValueError("unknown catalog %r: one of %r" % (catalog, SUMMARY_CATALOGS))
    if action is None:
        a = -1
    elif catalog == "feedwater":
        a = maint_action_index(action)
    elif isinstance(action, tuple):
        a = CMAINT_AUTO_ACTIONS[action] if catalog == "component" and action in CMAINT_AUTO_ACTIONS else \
            component_action_index(*action) if catalog == "component" else turbine_action_index(*action)
    elif isinstance(action, str):
        names = [k for k, (_kind, name) in enumerate(COMPONENT_ACTIONS if catalog == "component" else TURBINE_ACTIONS) if name == action]
        names += [v for (k, name), v in CMAINT_AUTO_ACTIONS.items() if catalog == "component" and name == action]
        if len(names) != 1:
            raise ValueError("%s maintenance %r names %d entries of the %s catalog: give it as (kind, name)" % (catalog, action, len(names), catalog))
        a = names[0]
    else:
        a = int(action)
    work, oper = SUMMARY_KINDS[catalog]
    kinds = sum(1 << k for k in work + (oper if operator else ()))
    if not kinds:
        raise ValueError("a key of the %s catalog matches nothing without operator=True: it has no work orders" % catalog)
    return SUMMARY_CATALOGS.index(catalog), a, -1 if unit is None else int(unit), kinds


class NpbEpisodeStreamsDesc(ctypes.Structure):
    """npb_episode_streams_desc_t: the block size, the optional per-bank-entry seed tables (host int64) and the caller's three output columns"""
    _fields_ = [("block", ctypes.c_int), ("bank_noise_seeds", ctypes.c_void_p), ("bank_profile_seeds", ctypes.c_void_p),
                ("n_bank_seeds", ctypes.c_int), ("noise_out", ctypes.c_void_p), ("setpoint_out", ctypes.c_void_p), ("target_out", ctypes.c_void_p)]


class NpbEpisodeRecordsDesc(ctypes.Structure):
    """npb_episode_records_desc_t: the caller's record columns (device, ``capacity`` entries each), the optional terminal-observation block
    and summary tables, and the cursor word"""
    _fields_ = [("capacity", ctypes.c_int32), ("clear_summary", ctypes.c_int32)] + \
               [(name, ctypes.c_void_p) for name in ("plant", "episode", "start", "length", "flags", "trip_flags", "step", "ret", "end_time", "final_obs",
                                                     "first_created", "first_completed", "n_created", "n_completed", "cursor")]


# the record's mandatory columns in descriptor order, with their numpy types (BatchedPlantEnv.enable_episode_records)
EPISODE_RECORD_COLUMNS = (("plant", np.int32), ("episode", np.int32), ("start", np.int32), ("length", np.int32), ("flags", np.int32),
                          ("trip_flags", np.uint32), ("step", np.int32), ("ret", np.float64), ("end_time", np.float64))


# include/npb.h npb_column_stats_desc_t: per-plant column statistics folded on the device (npb_set_column_stats)
COLUMN_STATS_MAX = 32
COLUMN_STATS = ("min", "max", "sum", "sumsq", "last", "first_beyond", "n_beyond")      # the per-cell tables in descriptor order (colstats.STATS)
COLUMN_STATS_NEED_LIMIT = ("first_beyond", "n_beyond")


class NpbColumnStatsDesc(ctypes.Structure):
    """npb_column_stats_desc_t: arena members and one-row side sources (host arrays), the limits (host arrays) and the caller's device tables"""
    _fields_ = [("n_fields", ctypes.c_int), ("kinds", ctypes.POINTER(ctypes.c_int)), ("slots", ctypes.POINTER(ctypes.c_int)),
                ("n_sources", ctypes.c_int), ("sources", ctypes.POINTER(NpbSampleSource)),
                ("direction", ctypes.POINTER(ctypes.c_int)), ("limit", ctypes.POINTER(ctypes.c_double))] + \
               [(name, ctypes.c_void_p) for name in COLUMN_STATS + ("n_samples",)]


class NpbEpisodeRecordStatsDesc(ctypes.Structure):
    """npb_episode_record_stats_desc_t: the record-side columns [n_cols][capacity] of each statistic, n_samples [capacity], and ``clear``"""
    _fields_ = [(name, ctypes.c_void_p) for name in COLUMN_STATS + ("n_samples",)] + [("clear", ctypes.c_int)]


def _bit_mask(x, who, through_int: bool = False) -> int:
    """THE mask check of the bit triggers, terms and rules.  ``through_int``: the triggers pass their word through int() first (4.0 and True
    are masks there), the task does not"""
    mask = int(x) if through_int else x
    if isinstance(mask, bool) or not isinstance(mask, (int, np.integer)) or not 0 < int(mask) <= 0xFFFFFFFF:
        raise ValueError("%s needs 0 < mask < 2**32, not %r" % (who, x))
    return int(mask)


def _summary_side(word, k, summary_keys, what):
    """THE check of ``("work_order" | "completed", key_index)``, and the side row it names: the summary's n_created / n_completed row of that
    key.  ``what``: "trigger" or "column", for the message"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("the %r %s takes the index of a summary key, not %r" % (word, what, k))
    if summary_keys < 1:
        raise ValueError("the %r %s reads the maintenance summary: enable_maintenance_summary() first" % (word, what))
    if not 0 <= k < summary_keys:
        raise ValueError("the %r %s: the summary's keys are 0 .. %d, not %d" % (word, what, summary_keys - 1, k))
    return ("n_created" if word == "work_order" else "n_completed", int(k), 1, "i32")


def column_word(col, info_columns=None, task: bool = False, integer_sides: bool = False, summary_keys: int = 0, controls: int = 0,
                orders: int = 0) -> dict:
    """THE resolver of a per-plant column word, for ``column_stats_request``, ``event_windows_request``, ``task_request`` and whoever reads
    a column next; a pure function, an unknown word is refused (ValueError).  Every vocabulary has the state members as ``set_fields`` keys
    them (``name``, ``(name, instance)`` or ``(name, instance, k)``), ``("info", column_name)``, ``("obs", i)`` and ``"reward"``.  ``task``:
    a task is set, so ``"task_reward"`` is a word too (statistics and windows; a task's own columns never admit it).  ``integer_sides``:
    the task's further words ``"flags"``, ``"done"``, ``"maintenance"`` and ``("work_order" | "completed", key_index)`` with ``summary_keys``
    keys in the summary.  ``controls``: the axis count while controls are set (``BatchedPlantEnv.set_controls``), so ``("control", a)`` and
    ``("control_prev", a)`` -- axis a's row of the held and of the previous action, real-valued -- are words too.  ``orders``: the rule
    count while order rules are set (``BatchedPlantEnv.set_control_orders``), so ``("order", r)`` -- 1.0 where rule r fired on this step,
    else 0.0 -- is a word too.  Returns {"member": (kind, slot) -- 0 f64 / 1 i32, as npb_gather_fields takes them -- or None, "side": (buffer,
    element offset, plant stride, element type) over the buffers of ``BatchedPlantEnv._side_buffers`` or None, "integer": bool}."""
    if info_columns is None:
        from .env import INFO_COLUMNS as info_columns
    key = (col,) if isinstance(col, str) else tuple(col)
    member = side = None
    if integer_sides and key in (("flags",), ("done",)):
        side = (key[0], 0, 1, "i32" if key[0] == "flags" else "u8")
    elif integer_sides and len(key) == 2 and key[0] in ("work_order", "completed"):
        side = _summary_side(key[0], key[1], summary_keys, "column")
    elif key == ("reward",):
        side = ("reward", 0, 1, "f64")
    elif controls and len(key) == 2 and key[0] in ("control", "control_prev"):
        if isinstance(key[1], bool) or not isinstance(key[1], (int, np.integer)) or not 0 <= key[1] < controls:
            raise ValueError("the column %r: the controls' axes are 0 .. %d, not %r" % (key[0], controls - 1, key[1]))
        side = (key[0], int(key[1]), 1, "f64")
    elif orders and len(key) == 2 and key[0] == "order":
        if isinstance(key[1], bool) or not isinstance(key[1], (int, np.integer)) or not 0 <= key[1] < orders:
            raise ValueError("the column 'order': the order rules are 0 .. %d, not %r" % (orders - 1, key[1]))
        side = ("order", int(key[1]), 1, "f64")
    elif key == ("task_reward",):
        if not task:
            raise ValueError("the column 'task_reward' needs a task: set_task() first")
        side = ("task_reward", 0, 1, "f64")
    elif key and key[0] == "info":
        if len(key) != 2 or key[1] not in info_columns:
            raise ValueError("unknown info column %r: one of %r" % (key[1:], tuple(info_columns)))
        side = ("info", list(info_columns).index(key[1]), len(info_columns), "f64")
    elif key and key[0] == "obs":
        if len(key) != 2 or isinstance(key[1], bool) or not isinstance(key[1], (int, np.integer)) or not 0 <= key[1] < OBS_DIM:
            raise ValueError("unknown obs column %r: ('obs', i) with 0 <= i < %d" % (key[1:], OBS_DIM))
        side = ("obs", int(key[1]), OBS_DIM, "f64")
    else:
        if integer_sides and key == ("maintenance",):
            key = ("maint.maintenance_actions_performed",)
        if not key or not isinstance(key[0], str) or key[0] not in SCHEMA.by_name or len(key) > 3:
            raise ValueError("unknown column %r: a state member (name, (name, instance) or (name, instance, k)), ('info', name), "
                             "('obs', i) or 'reward'" % (col,))
        try:
            kind, slot = SCHEMA.slot(key[0], *[int(x) for x in key[1:]])
        except IndexError:
            raise ValueError("column %r: no such instance or element of %s" % (col, key[0])) from None
        member = (0 if kind == "f64" else 1, slot)
    return {"member": member, "side": side, "integer": member[0] == 1 if member else side[3] in ("i32", "u8")}


def column_stats_request(columns, limits=None, stats=("min", "max", "sum", "sumsq", "last"), info_columns=None, task: bool = False,
                         controls: int = 0, orders: int = 0) -> dict:
    """What ``BatchedPlantEnv.enable_column_stats`` asks of npb_set_column_stats, from the caller's words; a pure function, host only, so an
    unknown name, index or statistic is refused (ValueError) before any device work.  ``columns``: a state member as ``set_fields`` keys it
    (``name``, ``(name, instance)`` or ``(name, instance, k)``), ``("info", column_name)``, ``("obs", i)`` or ``"reward"``.  ``limits``:
    ``{column_index: (">" | "<", value)}``, the index into ``columns``.  ``stats``: names of ``COLUMN_STATS``.  ``task``: a task is set
    (``BatchedPlantEnv.set_task``), so ``"task_reward"`` -- the task's reward column, buffer "task_reward" -- is a column too.
    Returns {"members": [(kind, slot)] -- 0 f64 / 1 i32, as npb_gather_fields takes them --, "sides": [(buffer, element offset, plant stride)]
    with buffer "info" | "obs" | "reward" (float64 device buffers of the env), "order": for every entry of ``columns`` its column on the
    device (members come first there, then the side rows), "direction" / "limit": lists per DEVICE column, "stats": the tables kept, in
    descriptor order}."""
    columns = list(columns)
    if not 1 <= len(columns) <= COLUMN_STATS_MAX:
        raise ValueError("column statistics take 1 to %d columns, not %d" % (COLUMN_STATS_MAX, len(columns)))
    stats = (stats,) if isinstance(stats, str) else tuple(stats)
    for name in stats:
        if name not in COLUMN_STATS:
            raise ValueError("unknown statistic %r: one of %r" % (name, COLUMN_STATS))
    members, sides, where = [], [], []
    for col in columns:
        C = column_word(col, info_columns, task, controls=controls, orders=orders)
        if C["member"]:
            where.append(("member", len(members))); members.append(C["member"])
        else:
            where.append(("side", len(sides))); sides.append(C["side"][:3])      # (every side of this vocabulary is a float64 buffer)
    order = [i if kind == "member" else len(members) + i for kind, i in where]
    direction, limit = [0] * len(columns), [0.0] * len(columns)
    for c, lim in (limits or {}).items():
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < len(columns):
            raise ValueError("limit on column %r: the columns are 0 .. %d" % (c, len(columns) - 1))
        if not isinstance(lim, (tuple, list)) or len(lim) != 2 or lim[0] not in (">", "<"):
            raise ValueError("the limit of column %d must be ('>' | '<', value), not %r" % (c, lim))
        if np.isnan(float(lim[1])):
            raise ValueError("the limit of column %d is NaN" % c)
        direction[order[c]], limit[order[c]] = (1 if lim[0] == ">" else -1), float(lim[1])
    if any(name in COLUMN_STATS_NEED_LIMIT for name in stats) and not any(direction):
        raise ValueError("the statistics %r need a limit on some column" % (COLUMN_STATS_NEED_LIMIT,))
    return {"members": members, "sides": sides, "order": order, "direction": direction, "limit": limit,
            "stats": tuple(name for name in COLUMN_STATS if name in stats)}


# include/npb.h npb_event_windows_desc_t: state windows around events, captured on the device (npb_set_event_windows)
EVENT_WINDOW_COLS_MAX, EVENT_WINDOW_TRIGGERS_MAX, EVENT_WINDOW_ROWS_MAX = 16, 8, 1024
TRIGGER_MODES = {"bits_rise": 0, "increase": 1, "beyond": 2}      # NPB_TRIGGER_MODE_*
EVENT_WINDOW_WORDS = ("plant", "episode", "trigger", "step", "n_pre", "n_post", "flags", "retriggers")      # the int32 record columns (eventwin.WORD_COLUMNS)


class NpbEventTrigger(ctypes.Structure):
    """npb_event_trigger_t: the trigger's column (an arena member, or a one-row side source) and its mode"""
    _fields_ = [("from_source", ctypes.c_int), ("kind", ctypes.c_int), ("slot", ctypes.c_int), ("source", NpbSampleSource),
                ("mode", ctypes.c_int), ("mask", ctypes.c_uint32), ("direction", ctypes.c_int), ("limit", ctypes.c_double)]


class NpbEventWindowsDesc(ctypes.Structure):
    """npb_event_windows_desc_t: recorded columns and triggers (host arrays), the window shape, and the caller's device record columns"""
    _fields_ = [("n_fields", ctypes.c_int), ("kinds", ctypes.POINTER(ctypes.c_int)), ("slots", ctypes.POINTER(ctypes.c_int)),
                ("n_sources", ctypes.c_int), ("sources", ctypes.POINTER(NpbSampleSource)),
                ("n_triggers", ctypes.c_int), ("triggers", ctypes.POINTER(NpbEventTrigger)),
                ("pre", ctypes.c_int), ("post", ctypes.c_int), ("capacity", ctypes.c_int)] + \
               [(name, ctypes.c_void_p) for name in EVENT_WINDOW_WORDS + ("fired", "time", "times", "values", "cursor")]


def event_windows_request(columns, triggers, pre, post, info_columns=None, summary_keys: int = 0, task: bool = False, controls: int = 0,
                          orders: int = 0) -> dict:
    """What ``BatchedPlantEnv.enable_event_windows`` asks of npb_set_event_windows, from the caller's words; a pure function, host only, so
    an unknown name or a trigger that cannot work is refused (ValueError) before any device work.  ``columns`` as ``column_stats_request``
    takes them, 1 to 16.  ``triggers``: 1 to 8, each ``("trip", mask)`` (rising bits of the step's trip flags), ``("done",)``,
    ``("work_order", key_index)`` / ``("completed", key_index)`` (the summary's n_created / n_completed row of that key goes up: needs
    ``summary_keys`` > key_index, the keys of ``enable_maintenance_summary``), ``("maintenance",)`` (the event count goes up) or
    ``(column, ">" | "<", value)`` (the edge of a limit on any column).  ``task``: a task is set (``BatchedPlantEnv.set_task``), so
    ``"task_reward"`` is a column and ``("task", mask)`` -- rising bits of the task's cause column, side buffer "task_cause" -- a trigger.
    Returns {"members", "sides", "order": as ``column_stats_request``; "triggers": per trigger {"member": (kind, slot) or None, "side":
    (buffer, element offset, plant stride, element type) or None, "mode": "bits_rise" | "increase" | "beyond", "mask", "direction",
    "limit"} with the side buffers "info" | "obs" | "reward" | "flags" | "done" | "n_created" | "n_completed" (for the last two the
    offset is the key's row); "numpy": the triggers as ``eventwin.record`` takes them; "pre", "post"}."""
    columns = list(columns)
    if not 1 <= len(columns) <= EVENT_WINDOW_COLS_MAX:
        raise ValueError("event windows take 1 to %d columns, not %d" % (EVENT_WINDOW_COLS_MAX, len(columns)))
    req = column_stats_request(columns, None, ("last",), info_columns, task, controls, orders)
    triggers = list(triggers)
    if not 1 <= len(triggers) <= EVENT_WINDOW_TRIGGERS_MAX:
        raise ValueError("event windows take 1 to %d triggers, not %d" % (EVENT_WINDOW_TRIGGERS_MAX, len(triggers)))
    pre, post = int(pre), int(post)
    if pre < 0 or post < 0 or pre + 1 + post > EVENT_WINDOW_ROWS_MAX:
        raise ValueError("event windows need pre >= 0, post >= 0 and pre + 1 + post <= %d" % EVENT_WINDOW_ROWS_MAX)
    out, as_numpy = [], []
    for t in triggers:
        t = (t,) if isinstance(t, str) else tuple(t)
        T = {"member": None, "side": None, "mode": "increase", "mask": 0, "direction": 0, "limit": 0.0}
        if len(t) == 2 and t[0] == "trip":
            mask = _bit_mask(t[1], "the ('trip', mask) trigger", through_int=True)
            T.update(side=("flags", 0, 1, "i32"), mode="bits_rise", mask=mask)
            as_numpy.append(("bits", mask))
        elif len(t) == 2 and t[0] == "task":
            int(t[1])      # (a mask that is no number is refused first, then the missing task, then the range: the order is kept)
            if not task:
                raise ValueError("the ('task', mask) trigger needs a task: set_task() first")
            mask = _bit_mask(t[1], "the ('task', mask) trigger", through_int=True)
            T.update(side=("task_cause", 0, 1, "i32"), mode="bits_rise", mask=mask)
            as_numpy.append(("bits", mask))
        elif t == ("done",):
            T.update(side=("done", 0, 1, "u8"), mode="bits_rise", mask=1)
            as_numpy.append(("bits", 1))
        elif len(t) == 2 and t[0] in ("work_order", "completed"):
            T.update(side=_summary_side(t[0], t[1], summary_keys, "trigger"))
            as_numpy.append(("increase",))
        elif t == ("maintenance",):
            T.update(member=column_word("maintenance", info_columns, integer_sides=True)["member"])
            as_numpy.append(("increase",))
        elif len(t) == 3 and t[1] in (">", "<"):
            if np.isnan(float(t[2])):
                raise ValueError("the limit of trigger %r is NaN" % (t,))
            C = column_word(t[0], info_columns, task, controls=controls, orders=orders)
            T.update(member=C["member"], side=C["side"], mode="beyond", direction=1 if t[1] == ">" else -1, limit=float(t[2]))
            as_numpy.append((t[1], float(t[2])))
        else:
            raise ValueError("unknown trigger %r: ('trip', mask), ('done',), ('work_order', key_index), ('completed', key_index), "
                             "('maintenance',) or (column, '>' | '<', value)" % (t,))
        out.append(T)
    return {"members": req["members"], "sides": req["sides"], "order": req["order"], "triggers": out, "numpy": as_numpy, "pre": pre, "post": post}


# include/npb.h npb_task_desc_t: the caller's reward terms and termination rules, formed on the device behind every step (npb_set_task)
TASK_TERMS_MAX, TASK_RULES_MAX = 16, 8
TASK_KINDS = {"value": 0, "abs_err": 1, "sq_err": 2, "beyond": 3, "excess": 4, "bits": 5, "delta": 6}      # NPB_TASK_* (task.KINDS)
TASK_MODES = {"bits_any": 0, "beyond": 1, "nonfinite": 2}                                                # NPB_TASK_RULE_MODE_* (task.MODES)


class NpbTaskColumn(ctypes.Structure):
    """npb_task_column_t: an arena member, or a one-row side source"""
    _fields_ = [("from_source", ctypes.c_int), ("kind", ctypes.c_int), ("slot", ctypes.c_int), ("source", NpbSampleSource)]


class NpbTaskTerm(ctypes.Structure):
    """npb_task_term_t: one reward term"""
    _fields_ = [("column", NpbTaskColumn), ("weight", ctypes.c_double), ("kind", ctypes.c_int), ("ref_from_column", ctypes.c_int),
                ("ref", ctypes.c_double), ("ref_column", NpbTaskColumn), ("direction", ctypes.c_int), ("limit", ctypes.c_double),
                ("mask", ctypes.c_uint32)]


class NpbTaskRule(ctypes.Structure):
    """npb_task_rule_t: one termination rule"""
    _fields_ = [("column", NpbTaskColumn), ("mode", ctypes.c_int), ("mask", ctypes.c_uint32), ("direction", ctypes.c_int),
                ("limit", ctypes.c_double), ("terminal_reward", ctypes.c_double)]


class NpbTaskDesc(ctypes.Structure):
    """npb_task_desc_t: the terms and rules (host arrays), the bias and the caller's device output columns"""
    _fields_ = [("n_terms", ctypes.c_int), ("terms", ctypes.POINTER(NpbTaskTerm)), ("n_rules", ctypes.c_int), ("rules", ctypes.POINTER(NpbTaskRule)),
                ("bias", ctypes.c_double), ("reward", ctypes.c_void_p), ("done", ctypes.c_void_p), ("cause", ctypes.c_void_p),
                ("terms_out", ctypes.c_void_p)]


def task_request(reward=(), terminate=(), bias: float = 0.0, info_columns=None, summary_keys: int = 0, controls: int = 0,
                 orders: int = 0) -> dict:
    """What ``BatchedPlantEnv.set_task`` asks of npb_set_task, from the caller's words; a pure function, host only, so a word that cannot
    work is refused (ValueError, naming it) before any device work.
    A column is keyed as ``column_stats_request`` keys it -- a state member, ``("info", name)``, ``("obs", i)``, ``"reward"`` (the step's
    own reward) -- or is one of the integer sides ``"flags"`` (the step's trip flags), ``"done"`` (the reference's scram pulse),
    ``("work_order", key_index)`` / ``("completed", key_index)`` (the summary's n_created / n_completed row of that key: needs
    ``summary_keys`` > key_index) and ``"maintenance"`` (the event count).
    ``reward``: 0 to 16 terms, ``(column, weight)`` (the value itself) or ``(column, weight, kind, ...)``: ``"value"``; ``"abs_err", ref``
    / ``"sq_err", ref`` with ref a number or a second column; ``"beyond", ">" | "<", limit`` / ``"excess", ">" | "<", limit``; ``"bits",
    mask`` on an integer column; ``"delta"``.  ``terminate``: 0 to 8 rules, ``("done",)`` (the reference's scram pulse), ``("trip",
    mask)`` (any of those trip flags set), ``(column, ">" | "<", value)`` or ``(column, "nonfinite")``, each with an optional trailing
    terminal reward.
    Returns {"columns": per column read {"member": (kind, slot) or None, "side": (buffer, element offset, plant stride, element type) or
    None, "integer": bool} with the side buffers of ``event_windows_request``; "terms": per term {"col", "weight", "kind", "ref" (a number,
    or ("col", index)), "direction", "limit", "mask"}; "rules": per rule {"col", "mode", "mask", "direction", "limit", "terminal_reward"};
    "bias"} -- "terms", "rules" and "bias" are the spec ``task.evaluate`` takes, over the rows of "columns"."""
    reward, terminate = list(reward or ()), list(terminate or ())
    if len(reward) > TASK_TERMS_MAX:
        raise ValueError("a task takes 0 to %d reward terms, not %d" % (TASK_TERMS_MAX, len(reward)))
    if len(terminate) > TASK_RULES_MAX:
        raise ValueError("a task takes 0 to %d termination rules, not %d" % (TASK_RULES_MAX, len(terminate)))
    if not reward and not terminate:
        raise ValueError("a task needs a reward term or a termination rule")
    bias = float(bias)
    if np.isnan(bias):
        raise ValueError("the bias is NaN")
    columns, index = [], {}

    def column(col):
        key = (col,) if isinstance(col, str) else tuple(col)
        if key in index:
            return index[key]
        C = column_word(col, info_columns, integer_sides=True, summary_keys=summary_keys, controls=controls, orders=orders)      # (an unknown word is refused there)
        index[key] = len(columns)
        columns.append(C)
        return index[key]

    def number(x, what, where):
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError("%s: %s must be a number, not %r" % (where, what, x))
        if np.isnan(float(x)):
            raise ValueError("%s: %s is NaN" % (where, what))
        return float(x)

    terms = []
    for i, term in enumerate(reward):
        where = "reward term %d %r" % (i, term)
        if not isinstance(term, (tuple, list)) or len(term) < 2:
            raise ValueError("%s: a term is (column, weight) or (column, weight, kind, ...)" % where)
        term = tuple(term)
        T = {"col": column(term[0]), "weight": number(term[1], "the weight", where), "kind": term[2] if len(term) > 2 else "value",
             "ref": 0.0, "direction": 0, "limit": 0.0, "mask": 0}
        kind, rest = T["kind"], term[3:]
        if not isinstance(kind, str) or kind not in TASK_KINDS:
            raise ValueError("%s: unknown kind %r: one of %r" % (where, kind, tuple(TASK_KINDS)))
        if kind in ("value", "delta"):
            if rest:
                raise ValueError("%s: a %r term takes nothing behind its kind" % (where, kind))
        elif kind in ("abs_err", "sq_err"):
            if len(rest) != 1:
                raise ValueError("%s: a %r term is (column, weight, %r, ref)" % (where, kind, kind))
            T["ref"] = ("col", column(rest[0])) if isinstance(rest[0], (str, tuple, list)) else number(rest[0], "the ref", where)
        elif kind in ("beyond", "excess"):
            if len(rest) != 2 or rest[0] not in (">", "<"):
                raise ValueError("%s: a %r term is (column, weight, %r, '>' | '<', limit)" % (where, kind, kind))
            T["direction"], T["limit"] = (1 if rest[0] == ">" else -1), number(rest[1], "the limit", where)
        else:
            if len(rest) != 1:
                raise ValueError("%s: a 'bits' term is (column, weight, 'bits', mask)" % where)
            if not columns[T["col"]]["integer"]:
                raise ValueError("%s: a 'bits' term needs an integer column" % where)
            T["mask"] = _bit_mask(rest[0], where + ":")
        terms.append(T)
    rules = []
    for i, rule in enumerate(terminate):
        where = "termination rule %d %r" % (i, rule)
        t = (rule,) if isinstance(rule, str) else tuple(rule)
        R = {"col": None, "mode": None, "mask": 0, "direction": 0, "limit": 0.0, "terminal_reward": 0.0}
        if len(t) in (2, 3) and isinstance(t[1], str) and t[1] == "nonfinite":
            R.update(col=column(t[0]), mode="nonfinite")
            tail = t[2:]
        elif len(t) in (3, 4) and isinstance(t[1], str) and t[1] in (">", "<"):
            R.update(col=column(t[0]), mode="beyond", direction=1 if t[1] == ">" else -1, limit=number(t[2], "the limit", where))
            tail = t[3:]
        elif len(t) in (2, 3) and t[0] == "trip":
            R.update(col=column("flags"), mode="bits_any", mask=_bit_mask(t[1], where + ":"))
            tail = t[2:]
        elif len(t) in (1, 2) and t[0] == "done":
            R.update(col=column("done"), mode="bits_any", mask=0xFF)
            tail = t[1:]
        else:
            raise ValueError("%s: a rule is ('done',), ('trip', mask), (column, '>' | '<', value) or (column, 'nonfinite'), each with an "
                             "optional trailing terminal reward" % where)
        if tail:
            R["terminal_reward"] = number(tail[0], "the terminal reward", where)
        rules.append(R)
    return {"columns": columns, "terms": terms, "rules": rules, "bias": bias}


# include/npb.h npb_features_desc_t: the caller's policy inputs, a stack of transformed frames kept on the device (npb_set_features)
FEATURES_COLS_MAX, FEATURES_STACK_MAX, FEATURES_CELLS_MAX = 64, 16, 256
FEATURE_KINDS = {"affine": 0, "bits": 1}               # NPB_FEATURE_KIND_* (features.KINDS)
FEATURE_DTYPES = {"float32": 0, "float64": 1}          # NPB_FEATURES_F32 / NPB_FEATURES_F64 (features.DTYPES)
FEATURE_OPTIONS = ("scale", "ref", "clip", "nan_to", "bits", "fresh", "ref_fresh")


class NpbFeatureColumn(ctypes.Structure):
    """npb_feature_column_t: one column and its transform"""
    _fields_ = [("column", NpbTaskColumn), ("kind", ctypes.c_int), ("mask", ctypes.c_uint32), ("scale", ctypes.c_double),
                ("ref_from_column", ctypes.c_int), ("ref", ctypes.c_double), ("ref_column", NpbTaskColumn), ("lo", ctypes.c_double),
                ("hi", ctypes.c_double), ("nan_to", ctypes.c_double), ("fresh", ctypes.c_double), ("fresh_live", ctypes.c_int),
                ("ref_fresh_live", ctypes.c_int)]


class NpbFeaturesDesc(ctypes.Structure):
    """npb_features_desc_t: the columns (a host array), the stack depth, the output type and the caller's device tensors"""
    _fields_ = [("n_columns", ctypes.c_int), ("columns", ctypes.POINTER(NpbFeatureColumn)), ("stack", ctypes.c_int), ("out_type", ctypes.c_int),
                ("out", ctypes.c_void_p), ("final", ctypes.c_void_p)]


def features_request(columns, stack: int = 1, dtype="float32", info_columns=None, task: bool = False, summary_keys: int = 0,
                     controls: int = 0, orders: int = 0) -> dict:
    """What ``BatchedPlantEnv.set_features`` asks of npb_set_features, from the caller's words; a pure function, host only, so a word that
    cannot work is refused (ValueError, naming it) before any device work.
    ``columns``: 1 to 64, each a column word or ``(word, options)``.  A word is what ``column_word`` resolves: a state member,
    ``("info", name)``, ``("obs", i)``, ``"reward"``, ``"flags"``, ``"done"``, ``"maintenance"``, ``("work_order" | "completed", key_index)``
    (``summary_keys`` > key_index) and, with ``task``, ``"task_reward"``.  ``options``: a dict of ``"scale"``, ``"ref"`` (a number, or a
    second column word: a setpoint error), ``"clip": (lo, hi)`` (None = that side open), ``"nan_to"``, ``"bits": mask`` (an integer column:
    1.0 where any of the bits is set; it excludes scale and ref), ``"fresh"`` (the raw value a side column takes in a fresh frame, default
    0.0) and ``"ref_fresh"`` (the same for a second column).  ``stack``: K, 1 to 16 with K * C <= 256.  ``dtype``: float32 or float64, as
    a name, a numpy dtype or a torch dtype.
    Returns {"columns": per column read what ``column_word`` answers, "spec": {"stack", "dtype", "columns"} -- what ``features.Stack`` and
    ``features.frame`` take, over the rows of "columns"; a member and the observation are ``live`` in a fresh frame}."""
    columns = list(columns) if isinstance(columns, (list, tuple)) else [columns]
    if not 1 <= len(columns) <= FEATURES_COLS_MAX:
        raise ValueError("features take 1 to %d columns, not %d" % (FEATURES_COLS_MAX, len(columns)))
    if isinstance(stack, bool) or not isinstance(stack, (int, np.integer)) or not 1 <= stack <= FEATURES_STACK_MAX:
        raise ValueError("the stack depth must be 1 .. %d, not %r" % (FEATURES_STACK_MAX, stack))
    if stack * len(columns) > FEATURES_CELLS_MAX:
        raise ValueError("stack * columns must be <= %d, not %d * %d" % (FEATURES_CELLS_MAX, stack, len(columns)))
    try:
        name = np.dtype(dtype).name
    except TypeError:      # (a torch dtype: "torch.float32")
        name = str(dtype).rsplit(".", 1)[-1]
    if name not in FEATURE_DTYPES:
        raise ValueError("the output type must be float32 or float64 (no half types), not %r" % (dtype,))
    rows, index = [], {}

    def row(col):
        key = (col,) if isinstance(col, str) else tuple(col)
        if key not in index:
            C = column_word(col, info_columns, task, integer_sides=True, summary_keys=summary_keys, controls=controls, orders=orders)      # (an unknown word is refused there)
            index[key] = len(rows)
            rows.append(C)
        return index[key]

    def live(r):
        return rows[r]["member"] is not None or rows[r]["side"][0] == "obs"

    def number(x, what, where, nan_ok=False):
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError("%s: %s must be a number, not %r" % (where, what, x))
        if not nan_ok and np.isnan(float(x)):
            raise ValueError("%s: %s is NaN" % (where, what))
        return float(x)

    spec = []
    for i, col in enumerate(columns):
        where = "feature column %d %r" % (i, col)
        word, opts = col, {}
        if isinstance(col, (tuple, list)) and len(col) == 2 and isinstance(col[1], dict):
            word, opts = col
        for key in opts:
            if key not in FEATURE_OPTIONS:
                raise ValueError("%s: unknown option %r: one of %r" % (where, key, FEATURE_OPTIONS))
        r = row(word)
        D = {"col": r, "kind": "affine", "scale": 1.0, "ref": 0.0, "lo": -np.inf, "hi": np.inf, "nan_to": np.nan, "mask": 0, "fresh": 0.0,
             "ref_fresh": 0.0, "live": live(r), "ref_live": False}
        if "bits" in opts:
            if "scale" in opts or "ref" in opts:
                raise ValueError("%s: 'bits' excludes 'scale' and 'ref'" % where)
            if not rows[r]["integer"]:
                raise ValueError("%s: 'bits' needs an integer column" % where)
            D["kind"], D["mask"] = "bits", _bit_mask(opts["bits"], where + ":")
        else:
            D["scale"] = number(opts.get("scale", 1.0), "the scale", where)
            ref = opts.get("ref", 0.0)
            if isinstance(ref, (str, tuple, list)):
                rr = row(ref)
                D["ref"], D["ref_live"] = ("col", rr), live(rr)
                D["ref_fresh"] = number(opts.get("ref_fresh", 0.0), "ref_fresh", where)
            else:
                D["ref"] = number(ref, "the ref", where)
        if "clip" in opts:
            clip = opts["clip"]
            if not isinstance(clip, (tuple, list)) or len(clip) != 2:
                raise ValueError("%s: 'clip' is (lo, hi), either None for an open side" % where)
            D["lo"] = -np.inf if clip[0] is None else number(clip[0], "the lower clip limit", where)
            D["hi"] = np.inf if clip[1] is None else number(clip[1], "the upper clip limit", where)
            if D["lo"] > D["hi"]:
                raise ValueError("%s: a clip with lo > hi" % where)
        D["nan_to"] = number(opts.get("nan_to", np.nan), "nan_to", where, nan_ok=True)
        D["fresh"] = number(opts.get("fresh", 0.0), "fresh", where)
        spec.append(D)
    return {"columns": rows, "spec": {"stack": int(stack), "dtype": name, "columns": spec}}


# include/npb.h npb_controls_desc_t: the caller's policy outputs, decoded on the device in front of every step (npb_set_controls)
CONTROLS_AXES_MAX, CONTROLS_INTERVAL_MAX = 8, 64
CONTROL_KINDS = {"rate": 0, "target": 1, "column": 2, "value": 3}                  # NPB_CONTROL_KIND_* (controls.KINDS)
CONTROL_ACTUATORS = {"rod": 0, "flow": 1, "valve": 2, "boron": 3}      # NPB_ACTUATOR_* (controls.ACTUATORS)
CONTROL_INPUTS = {"power_setpoint": 0, "cooling_water_temp": 1}        # NPB_CONTROL_INPUT_* (controls.INPUTS)
CONTROL_DTYPES = {"float32": 0, "float64": 1}                          # NPB_CONTROLS_F32 / NPB_CONTROLS_F64 (controls.DTYPES)
CONTROL_OPTIONS = ("scale", "offset", "clip", "nan_to", "deadband", "max_magnitude")


class NpbControlAxis(ctypes.Structure):
    """npb_control_axis_t: one axis, its transform and what it moves or fills"""
    _fields_ = [("kind", ctypes.c_int), ("target", ctypes.c_int), ("scale", ctypes.c_double), ("offset", ctypes.c_double), ("lo", ctypes.c_double),
                ("hi", ctypes.c_double), ("nan_to", ctypes.c_double), ("deadband", ctypes.c_double), ("max_magnitude", ctypes.c_double)]


class NpbControlsDesc(ctypes.Structure):
    """npb_controls_desc_t: the axes (a host array), the hold interval, the input type and the caller's device tensors (``input``: the
    header's ``in``)"""
    _fields_ = [("n_axes", ctypes.c_int), ("axes", ctypes.POINTER(NpbControlAxis)), ("interval", ctypes.c_int), ("in_type", ctypes.c_int),
                ("input", ctypes.c_void_p), ("held", ctypes.c_void_p), ("prev", ctypes.c_void_p)]



# include/npb.h npb_control_orders_desc_t: order rules on the controls' VALUE axes (npb_set_control_orders)
# (CONTROL_ORDERS_MAX, CONTROL_ORDER_NEVER, ORDER_FAMILIES and the two structures: orders_abi.py)
ORDER_OPTIONS = ("unit", "threshold", "min_interval", "bearing", "target_level", "cleaning_type", "tubes_to_plug")
# include/npb_maint.h NPB_MAINT_ACTIONS' handler column: the pump actions the dispatcher has a handler for (load() holds it against the library's)
MAINT_ACTION_HANDLERS = (1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 0)
MAINT_BEARING_REPLACEMENT = MAINT_ACTION_NAMES.index("bearing_replacement")
TURBINE_THRUST_ADJUSTMENT = TURBINE_ACTIONS.index(("bearing", "thrust_bearing_adjustment"))


def control_orders_request(orders) -> list:
    """What ``BatchedPlantEnv.set_control_orders`` asks of npb_set_control_orders, from the caller's words; a pure function, host only.
    ``orders``: 1 to 8, each ``(axis, component, action)`` or ``(axis, component, action, options)``.  ``component``: ``"pump"``, a kind of
    ``COMPONENT_KINDS`` or a kind of ``TURBINE_KINDS``; ``action``: a name of that component's catalog or its index, resolved by
    ``maint_action_index`` / ``component_action_index`` / ``turbine_action_index`` (whose refusals, "not offered" among them, keep their
    messages).  ``options``: ``"unit"`` (default 0), ``"threshold"`` (0.0), ``"min_interval"`` (1), ``"bearing"`` (a pump's bearing
    replacement; a name of ``MAINT_BEARINGS`` or NPB_BEARING_*), ``"target_level"`` (a pump's oil top-off, default 95.0),
    ``"cleaning_type"`` (the component family; a name or NPB_CLEANING_*), ``"tubes_to_plug"``.  Returns the rules ``controls.Orders``
    takes: [{"axis", "family", "action", "unit", "option", "amount", "threshold", "min_interval"}]; what only the controls' axes, the
    plant count and the mode can refuse is ``controls.orders_check``'s."""
    orders = list(orders)
    if not 1 <= len(orders) <= CONTROL_ORDERS_MAX:
        raise ValueError("order rules: 1 to %d, not %d" % (CONTROL_ORDERS_MAX, len(orders)))
    rules = []
    for r, o in enumerate(orders):
        where = "order rule %d %r" % (r, o)
        if not isinstance(o, (tuple, list)) or len(o) not in (3, 4):
            raise ValueError("%s: (axis, component, action) or (axis, component, action, options)" % where)
        axis, component, action = o[0], o[1], o[2]
        opt = dict(o[3]) if len(o) == 4 else {}
        unknown = sorted(set(opt) - set(ORDER_OPTIONS))
        if unknown:
            raise ValueError("%s: unknown option(s) %r: of %r" % (where, unknown, ORDER_OPTIONS))
        if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)):
            raise ValueError("%s: the axis is an index into the controls' axes" % where)
        option, amount = 0, 0.0
        if component == "pump":
            family, a = "pump", maint_action_index(action)
            bearing = opt.get("bearing")
            if isinstance(bearing, str) and bearing not in MAINT_BEARINGS:
                raise ValueError("%s: unknown bearing %r: one of %r" % (where, bearing, [k for k in MAINT_BEARINGS if k]))
            option = MAINT_BEARINGS[bearing] if bearing is None or isinstance(bearing, str) else int(bearing)
            amount = float(opt.get("target_level", 95.0))
        elif component in COMPONENT_KINDS:
            family, a = "component", component_action_index(component, action)
            option = cleaning_type_index(opt.get("cleaning_type"))
            amount = float(opt.get("tubes_to_plug", 0.0))
        elif component in TURBINE_KINDS:
            family, a = "turbine", turbine_action_index(component, action)
        else:
            raise ValueError("%s: unknown component %r: 'pump', one of %r or one of %r" % (where, component, COMPONENT_KINDS, TURBINE_KINDS))
        if not isinstance(action, str):      # an index must name an action of the component given
            catalog = COMPONENT_ACTIONS if family == "component" else TURBINE_ACTIONS if family == "turbine" else None
            if catalog is not None and 0 <= a < len(catalog) and catalog[a][0] != component:
                raise ValueError("%s: index %d of the %s catalog is a %s action, not a %s one" % (where, a, family, catalog[a][0], component))
        rules.append({"axis": int(axis), "family": family, "action": int(a), "unit": int(opt.get("unit", 0)), "option": int(option),
                      "amount": amount, "threshold": float(opt.get("threshold", 0.0)), "min_interval": opt.get("min_interval", 1)})
    return rules


# include/npb.h npb_rollout_desc_t: what the policy saw, did and got for a horizon of steps, recorded on the device (npb_set_rollout)
ROLLOUT_HORIZON_MAX, ROLLOUT_EXTRAS_MAX = 4096, 8
ROLLOUT_BITS = {"terminated": 1, "truncated": 2, "cut": 4}             # NPB_ROLLOUT_TERMINATED / _TRUNCATED / _CUT (rollout.TERMINATED ...)
ROLLOUT_DTYPES = {"float32": 0, "float64": 1}                          # NPB_ROLLOUT_F32 / NPB_ROLLOUT_F64


class NpbRolloutDesc(ctypes.Structure):
    """npb_rollout_desc_t: the horizon, the extras count, the rows of final_obs per plant and the caller's device buffers"""
    _fields_ = [("horizon", ctypes.c_int), ("n_extras", ctypes.c_int), ("final_rows", ctypes.c_int), ("extras_in", ctypes.c_void_p),
                ("obs", ctypes.c_void_p), ("act", ctypes.c_void_p), ("extra", ctypes.c_void_p), ("reward", ctypes.c_void_p),
                ("ended", ctypes.c_void_p), ("episode", ctypes.c_void_p), ("final_row", ctypes.c_void_p), ("final_obs", ctypes.c_void_p)]


class NpbRolloutAdvantagesDesc(ctypes.Structure):
    """npb_rollout_advantages_desc_t: gamma, lambda, the value column (base and strides in elements), the last and final values, the
    output type and the two outputs"""
    _fields_ = [("gamma", ctypes.c_double), ("lam", ctypes.c_double), ("value", ctypes.c_void_p), ("value_time_stride", ctypes.c_int64),
                ("value_plant_stride", ctypes.c_int64), ("last_value", ctypes.c_void_p), ("final_value", ctypes.c_void_p),
                ("out_type", ctypes.c_int), ("adv", ctypes.c_void_p), ("ret", ctypes.c_void_p)]


# include/npb.h npb_moments_desc_t / npb_minibatch_desc_t: the pinned moments and one shuffled minibatch of the rollout (npb_rollout_moments,
# npb_rollout_minibatch)
MINIBATCH_ROUNDS = 6
MINIBATCH_UNITS = {"transition": 0, "plant": 1, "segment": 2}          # NPB_MINIBATCH_TRANSITION / _PLANT / _SEGMENT (rollout.UNITS)


class NpbMomentsDesc(ctypes.Structure):
    """npb_moments_desc_t: a contiguous device [rows, cols] tensor, its type, ddof and the four doubles count, mean, var, std"""
    _fields_ = [("src", ctypes.c_void_p), ("type", ctypes.c_int), ("ddof", ctypes.c_int), ("rows", ctypes.c_int64), ("cols", ctypes.c_int64),
                ("out", ctypes.c_void_p)]


class NpbMinibatchDesc(ctypes.Structure):
    """npb_minibatch_desc_t: the unit, the epoch's round keys, the window of the permutation, the advantages and returns with their type,
    the moments (or NULL), eps, the outputs and the most workgroups the launch may have (0: the launcher's bound)"""
    _fields_ = [("unit", ctypes.c_int), ("keys", ctypes.c_uint32 * MINIBATCH_ROUNDS), ("type", ctypes.c_int), ("first", ctypes.c_int64),
                ("count", ctypes.c_int64), ("adv", ctypes.c_void_p), ("ret", ctypes.c_void_p), ("moments", ctypes.c_void_p),
                ("eps", ctypes.c_double), ("index", ctypes.c_void_p), ("obs", ctypes.c_void_p), ("act", ctypes.c_void_p),
                ("extra", ctypes.c_void_p), ("adv_out", ctypes.c_void_p), ("ret_out", ctypes.c_void_p), ("max_blocks", ctypes.c_int)]


class NpbNormalizerDesc(ctypes.Structure):
    """npb_normalizer_desc_t: the chosen feature columns (a host array of indices), eps, and the return stream's gamma, clip and output"""
    _fields_ = [("n_columns", ctypes.c_int), ("columns", ctypes.POINTER(ctypes.c_int)), ("eps", ctypes.c_double), ("reward", ctypes.c_int),
                ("gamma", ctypes.c_double), ("clip", ctypes.c_double), ("norm_reward", ctypes.c_void_p)]


# include/npb.h npb_policy_desc_t: an MLP actor-critic with Gaussian sampling between the features and the controls' input (npb_set_policy)
POLICY_HIDDEN_MAX, POLICY_WIDTH_MAX = 3, 128
POLICY_ACTIVATIONS = {"relu": 0, "tanh": 1}                            # NPB_POLICY_RELU / NPB_POLICY_TANH (policy.ACTIVATIONS)


class NpbPolicyDesc(ctypes.Structure):
    """npb_policy_desc_t: the hidden widths of both nets, the activation, the noise's seed and first plant, the caller's value and logp
    buffers and the rollout's extras input with the two slots (-1 = none)"""
    _fields_ = [("actor_layers", ctypes.c_int), ("actor_width", ctypes.c_int * POLICY_HIDDEN_MAX), ("critic_layers", ctypes.c_int),
                ("critic_width", ctypes.c_int * POLICY_HIDDEN_MAX), ("activation", ctypes.c_int), ("deterministic", ctypes.c_int),
                ("seed", ctypes.c_uint64), ("first_plant", ctypes.c_int64), ("value", ctypes.c_void_p), ("logp", ctypes.c_void_p),
                ("extras_in", ctypes.c_void_p), ("n_extras", ctypes.c_int), ("value_slot", ctypes.c_int), ("logp_slot", ctypes.c_int)]


# include/npb.h npb_ppo_desc_t: one minibatch and the hyper-parameters of the policy's training step (npb_policy_grad, npb_policy_update)
PPO_STATS = 8                                                          # NPB_PPO_STATS (ppo.STATS)


class NpbPpoDesc(ctypes.Structure):
    """npb_ppo_desc_t: the five input tensors with their types, the row count, the three optional per-row outputs, the hyper-parameters,
    the statement's rows_per_chain and the launch's max_blocks"""
    _fields_ = [("obs", ctypes.c_void_p), ("obs_type", ctypes.c_int), ("act", ctypes.c_void_p), ("act_type", ctypes.c_int),
                ("logp_old", ctypes.c_void_p), ("adv", ctypes.c_void_p), ("ret", ctypes.c_void_p), ("adv_type", ctypes.c_int),
                ("count", ctypes.c_int), ("logp_new", ctypes.c_void_p), ("value_new", ctypes.c_void_p), ("ratio", ctypes.c_void_p),
                ("clip", ctypes.c_double), ("vf_coef", ctypes.c_double), ("ent_coef", ctypes.c_double), ("max_grad_norm", ctypes.c_double),
                ("rows_per_chain", ctypes.c_int), ("max_blocks", ctypes.c_int)]


# npb_ppo_more_t, the options of one update, and NPB_PPO_STATS_MORE: nuclear_sim_amd/ppo_abi.py (tests/test_ppo_options_abi.py holds its layout)


def controls_request(axes, interval: int = 1, dtype="float32", heat_source: int = 0) -> dict:
    """What ``BatchedPlantEnv.set_controls`` asks of npb_set_controls, from the caller's words; a pure function, host only, so an axis that
    cannot work is refused (ValueError, naming it) before any device work.
    ``axes``: 1 to 8, each ``(target, kind)`` or ``(target, kind, options)``: ``("rod" | "flow" | "valve" | "boron", "rate" | "target")`` or
    ``("power_setpoint" | "cooling_water_temp", "column")``, or ``(None, "value")`` for an output that moves nothing and is only held, for
    the task and the features to read.  ``options``: a dict of ``"scale"`` and ``"offset"`` (y = x * scale + offset),
    ``"clip": (lo, hi)`` (None = that side open; a rate's default is (-1, 1)), ``"nan_to"`` (what a NaN x becomes, default 0.0),
    ``"deadband"`` (a rate: |y| below it gives 0) and ``"max_magnitude"`` (a target: the magnitude of one step's move, default 1.0).
    ``interval``: K, 1 to 64, the steps a decoded row is held.  ``dtype``: float32 or float64, as a name, a numpy dtype or a torch dtype.
    ``heat_source``: the handle's (a "power_setpoint" axis is refused under the external heat source, whose plugin owns that column).
    Returns the spec ``controls.Decoder`` takes: {"interval", "dtype", "axes": [{"kind", "target", "scale", "offset", "lo", "hi", "nan_to",
    "deadband", "max_magnitude"}]}."""
    axes = list(axes)
    if not 1 <= len(axes) <= CONTROLS_AXES_MAX:
        raise ValueError("controls take 1 to %d axes, not %d" % (CONTROLS_AXES_MAX, len(axes)))
    if isinstance(interval, bool) or not isinstance(interval, (int, np.integer)) or not 1 <= interval <= CONTROLS_INTERVAL_MAX:
        raise ValueError("the interval must be 1 .. %d, not %r" % (CONTROLS_INTERVAL_MAX, interval))
    try:
        name = np.dtype(dtype).name
    except TypeError:      # (a torch dtype: "torch.float32")
        name = str(dtype).rsplit(".", 1)[-1]
    if name not in CONTROL_DTYPES:
        raise ValueError("the input type must be float32 or float64 (no half types), not %r" % (dtype,))

    def number(x, what, where):
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError("%s: %s must be a number, not %r" % (where, what, x))
        if not np.isfinite(float(x)):
            raise ValueError("%s: %s must be finite, not %r" % (where, what, x))
        return float(x)

    spec, taken = [], {}
    for a, ax in enumerate(axes):
        where = "control axis %d %r" % (a, ax)
        if not isinstance(ax, (tuple, list)) or len(ax) not in (2, 3) or (len(ax) == 3 and not isinstance(ax[2], dict)):
            raise ValueError("%s: an axis is (target, kind) or (target, kind, options)" % where)
        target, kind, opts = ax[0], ax[1], (ax[2] if len(ax) == 3 else {})
        if kind not in CONTROL_KINDS:
            raise ValueError("%s: unknown kind %r: one of %r" % (where, kind, tuple(CONTROL_KINDS)))
        names = CONTROL_INPUTS if kind == "column" else CONTROL_ACTUATORS if kind != "value" else (None,)
        if target not in names:
            raise ValueError("%s: unknown %s %r: one of %r" % (where, "input" if kind == "column" else "actuator", target, tuple(names)))
        if target is not None and target in taken:
            raise ValueError("%s: %r is already taken by axis %d" % (where, target, taken[target]))
        taken[target] = a
        for key in opts:
            if key not in CONTROL_OPTIONS:
                raise ValueError("%s: unknown option %r: one of %r" % (where, key, CONTROL_OPTIONS))
        if "deadband" in opts and kind != "rate":
            raise ValueError("%s: 'deadband' is a rate's option" % where)
        if "max_magnitude" in opts and kind != "target":
            raise ValueError("%s: 'max_magnitude' is a target's option" % where)
        D = {"kind": kind, "target": target, "scale": number(opts.get("scale", 1.0), "the scale", where),
             "offset": number(opts.get("offset", 0.0), "the offset", where), "lo": -1.0 if kind == "rate" else -np.inf,
             "hi": 1.0 if kind == "rate" else np.inf, "nan_to": number(opts.get("nan_to", 0.0), "nan_to", where),
             "deadband": number(opts.get("deadband", 0.0), "the deadband", where),
             "max_magnitude": number(opts.get("max_magnitude", 1.0), "max_magnitude", where)}
        if D["deadband"] < 0:
            raise ValueError("%s: a negative deadband" % where)
        if D["max_magnitude"] < 0:
            raise ValueError("%s: a negative max_magnitude" % where)
        if "clip" in opts:
            clip = opts["clip"]
            if not isinstance(clip, (tuple, list)) or len(clip) != 2:
                raise ValueError("%s: 'clip' is (lo, hi), either None for an open side" % where)
            for side, x, open_side in (("lo", clip[0], -np.inf), ("hi", clip[1], np.inf)):
                if x is None:
                    D[side] = open_side
                elif isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or np.isnan(float(x)):
                    raise ValueError("%s: the clip limits must be numbers (or None), not %r" % (where, x))
                else:
                    D[side] = float(x)
            if D["lo"] > D["hi"]:
                raise ValueError("%s: a clip with lo > hi" % where)
        if target == "power_setpoint" and heat_source == HEAT_EXTERNAL:
            raise ValueError("%s: under the external heat source the power_setpoint column carries the plugin's power" % where)
        spec.append(D)
    return {"interval": int(interval), "dtype": name, "axes": spec}


def episode_streams_desc(block, bank_noise_seeds=None, bank_profile_seeds=None, outputs=(None, None, None)):
    """(desc, keep): an NpbEpisodeStreamsDesc and the host arrays it points into (host only, no library needed).  A table is a sequence of
    seeds, one per bank entry; both tables, where both are given, have the same length.  ``outputs``: three device addresses or None."""
    tables = [None if t is None else np.ascontiguousarray(np.asarray(t, dtype=np.int64).reshape(-1)) for t in (bank_noise_seeds, bank_profile_seeds)]
    sizes = {t.size for t in tables if t is not None}
    if len(sizes) > 1:
        raise ValueError("bank_noise_seeds and bank_profile_seeds: one seed per bank entry each (%s)" % sorted(sizes))
    d = NpbEpisodeStreamsDesc()
    d.block = int(block)
    d.bank_noise_seeds, d.bank_profile_seeds = (None if t is None else t.ctypes.data for t in tables)
    d.n_bank_seeds = sizes.pop() if sizes else 0
    d.noise_out, d.setpoint_out, d.target_out = outputs
    return d, tables


_vp, _ci, _cd, _sz, _cs, _i64, _u64 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int64,
                                       ctypes.c_uint64)
_P = ctypes.POINTER
# THE statement of the C ABI's Python signatures (include/npb.h; tests/test_binding_cpu.py holds every row against its prototype):
# (the symbol whose presence detects the group -- None: the core, always there --, {name: (restype, argtypes)}).  A restype of None
# leaves ctypes' int (the header's int and void), argtypes of None leave the function as ctypes hands it out (no parameters).  A group
# absent from an older or ablated build is skipped; NPB_VERSION does not move with a new group.
ENTRY_POINTS = (
    (None, {
        "npb_version": (_ci, None), "npb_num_f64": (_ci, None), "npb_num_i32": (_ci, None),
        "npb_state_bytes": (_sz, None), "npb_step_bytes_per_plant": (_sz, None),
        "npb_default_params": (None, [_P(NpbParams)]),
        "npb_create": (None, [_P(NpbParams), _ci, _ci, _P(_vp)]),
        "npb_create_storage": (None, [_P(NpbParams), _ci, _ci, _ci, _P(_vp)]),
        "npb_storage": (None, [_vp]),
        "npb_handle_step_bytes_per_plant": (_sz, [_vp]),
        "npb_destroy": (None, [_vp]),
        "npb_last_error": (_cs, [_vp]),
        "npb_num_plants": (None, [_vp]),
        "npb_set_params": (None, [_vp, _P(NpbParams)]),
        "npb_reset": (None, [_vp, _vp, _vp]),
        "npb_set_step_kernel": (None, [_vp, _ci]),
        "npb_set_maintenance_table": (None, [_vp, _P(NpbMaintTable)]),
        "npb_default_maintenance_table": (None, [_P(NpbMaintTable)]),
        "npb_reset_reference": (None, [_vp, _vp, _ci, _vp]),
        "npb_get_field": (None, [_vp, _ci, _ci, _vp, _ci, _vp]),
        "npb_set_field": (None, [_vp, _ci, _ci, _vp, _ci, _vp]),
        "npb_state_arena": (None, [_vp, _P(_vp), _P(_sz), _P(_ci)]),
        "npb_gather_fields": (None, [_vp, _ci, _vp, _vp, _vp, _vp]),
        "npb_locate_field": (None, [_vp, _ci, _ci, _P(_ci), _P(_ci), _P(_ci)]),
        "npb_step": (None, [_vp] * 12),
        "npb_observe": (None, [_vp, _vp, _vp]),
        "npb_debug_touch": (None, [_vp, _vp])}),
    ("npb_debug_last_step_kernel", {     # ABI 140
        "npb_debug_last_step_kernel": (None, [_vp]),
        "npb_step_kernel_name": (_cs, [_ci]),
        "npb_maint_param_name": (_cs, [_ci]), "npb_maint_action_name": (_cs, [_ci]),
        "npb_maint_num_params": (None, None), "npb_maint_num_actions": (None, None),
        "npb_obs_dim": (None, None), "npb_info_dim": (None, None), "npb_info_nrho": (None, None), "npb_diag_dim": (None, None)}),
    ("npb_set_diagnostics", {     # (absent from builds older than ABI 133: tools/ab_kernel.py loads those)
        "npb_set_diagnostics": (None, [_vp, _vp, _sz])}),
    ("npb_set_maintenance_count_buffer", {
        "npb_set_maintenance_count_buffer": (None, [_vp, _vp])}),
    ("npb_state_arena_layout", {     # ABI 142
        "npb_state_arena_layout": (None, [_vp, _P(_vp), _P(_sz), _P(_sz), _P(_ci), _P(_ci)])}),
    ("npb_state_arena_segment", {    # ABI 141
        "npb_state_arena_segment": (_sz, [_vp])}),
    ("npb_snapshot", {     # ABI 143: episodes
        "npb_snapshot": (None, [_vp, _vp]),
        "npb_restore": (None, [_vp, _vp, _vp]),
        "npb_set_autoreset": (None, [_vp, _ci, _ci]),
        "npb_set_episode_buffers": (None, [_vp, _vp, _vp, _vp, _vp])}),
    ("npb_set_start_bank", {     # ABI 144: restarts from a bank of start states
        "npb_set_start_bank": (None, [_vp, _vp, _vp]),
        "npb_set_start_slots": (None, [_vp, _vp, _vp, _ci]),
        "npb_restore_bank": (None, [_vp, _vp, _vp]),
        "npb_set_episode_start_buffer": (None, [_vp, _vp])}),
    ("npb_set_maintenance_log", {     # ABI 146: the maintenance event log
        "npb_set_maintenance_log": (None, [_vp, _vp, _ci, _vp]),
        "npb_maint_event_bytes": (_sz, None),
        "npb_maint_action_has_handler": (None, [_ci])}),
    ("npb_perform_maintenance", {     # ABI 147: maintenance the caller orders
        "npb_perform_maintenance": (None, [_vp] * 7)}),
    ("npb_perform_component_maintenance", {     # ABI 148: maintenance of steam generators, condenser and ejectors the caller orders
        "npb_perform_component_maintenance": (None, [_vp] * 7),
        "npb_component_num_actions": (None, None),
        "npb_component_action_name": (_cs, [_ci]),
        "npb_component_kind_name": (_cs, [_ci]),
        "npb_component_action_kind": (None, [_ci])}),
    ("npb_perform_turbine_maintenance", {     # ABI 149: maintenance of the turbine the caller orders
        "npb_perform_turbine_maintenance": (None, [_vp] * 5),
        "npb_turbine_num_actions": (None, None),
        "npb_turbine_action_name": (_cs, [_ci]),
        "npb_turbine_kind_name": (_cs, [_ci]),
        "npb_turbine_action_kind": (None, [_ci])}),
    ("npb_set_component_maintenance", {     # ABI 150: automatic maintenance of steam generators and condenser
        "npb_set_component_maintenance": (None, [_vp, _P(NpbComponentMaintTable)]),
        "npb_default_component_maintenance_table": (None, [_P(NpbComponentMaintTable)]),
        "npb_component_maint_num_params": (None, None),
        "npb_component_maint_param_name": (_cs, [_ci]),
        "npb_component_maint_param_kind": (None, [_ci]),
        "npb_component_maintenance_state_bytes": (_sz, [_vp]),
        "npb_get_component_maintenance_state": (None, [_vp, _vp, _vp]),
        "npb_set_component_maintenance_state": (None, [_vp, _vp, _vp])}),
    ("npb_carry_diagnostics", {     # ABI 151: the carried diagnostics rows travel with restores, resets and checkpoints
        "npb_carry_diagnostics": (None, [_vp, _ci]),
        "npb_diag_num_carried": (None, None),
        "npb_diag_carried_row": (None, [_ci]),
        "npb_diag_carried_fresh": (_cd, [_ci]),
        "npb_get_diagnostics_state": (None, [_vp, _vp, _vp]),
        "npb_set_diagnostics_state": (None, [_vp, _vp, _vp]),
        "npb_set_episode_index_buffer": (None, [_vp, _vp])}),
    ("npb_noise_seed", {     # ABI 145: heat-source noise streams on the device
        "npb_noise_seed": (None, [_vp, _vp, _vp]),
        "npb_noise_fill": (None, [_vp, _ci, _vp, _vp]),
        "npb_noise_get_state": (None, [_vp] * 6),
        "npb_noise_set_state": (None, [_vp] * 6)}),
    ("npb_profile_seed", {     # ABI 152: the data-gen runner's power profile on the device
        "npb_profile_seed": (None, [_vp, _vp, _ci, _vp, _ci, _vp, _ci, _vp]),
        "npb_profile_fill": (None, [_vp, _ci, _vp, _vp, _vp, _vp]),
        "npb_profile_ramp": (None, [_vp, _ci, _vp, _vp, _vp]),
        "npb_profile_get_state": (None, [_vp] * 8),
        "npb_profile_set_state": (None, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _vp])}),
    ("npb_sampler_create", {     # ABI 153: a state log samples a watch list of plants
        "npb_sampler_create": (None, [_vp, _P(NpbSamplerDesc), _P(_ci)]),
        "npb_sampler_sample": (None, [_vp, _ci, _vp, _vp]),
        "npb_sampler_destroy": (None, [_vp, _ci])}),
    ("npb_set_maintenance_summary", {     # ABI 154: the event log folded into a per-plant work-order summary
        "npb_set_maintenance_summary": (None, [_vp, _P(NpbMaintSummaryDesc)]),
        "npb_maint_summary_check": (_cs, [_P(NpbMaintSummaryDesc), _ci, _ci]),
        "npb_maint_summary_fold": (None, [_vp, _vp]),
        "npb_maint_summary_clear": (None, [_vp, _vp, _vp])}),
    ("npb_set_episode_streams", {     # (ABI 154 still) each plant's noise and power profile restart with its episode
        "npb_set_episode_streams": (None, [_vp, _P(NpbEpisodeStreamsDesc), _vp]),
        "npb_episode_streams_check": (_cs, [_P(NpbEpisodeStreamsDesc), _ci, _ci]),
        "npb_profile_get_positions": (None, [_vp, _vp, _vp, _vp])}),
    ("npb_set_episode_records", {     # a device-side log of finished episodes, with their work-order summary
        "npb_set_episode_records": (None, [_vp, _P(NpbEpisodeRecordsDesc)]),
        "npb_episode_records_check": (_cs, [_P(NpbEpisodeRecordsDesc), _ci, _ci])}),
    ("npb_set_column_stats", {     # per-plant column statistics folded behind every step, and their copy into the episode records
        "npb_set_column_stats": (None, [_vp, _P(NpbColumnStatsDesc)]),
        "npb_column_stats_check": (_cs, [_P(NpbColumnStatsDesc), _ci]),
        "npb_column_stats_fold": (None, [_vp, _vp]),
        "npb_column_stats_clear": (None, [_vp, _vp, _vp]),
        "npb_set_episode_record_stats": (None, [_vp, _P(NpbEpisodeRecordStatsDesc)])}),
    ("npb_set_task", {     # the caller's reward terms and termination rules, formed behind every step
        "npb_set_task": (None, [_vp, _P(NpbTaskDesc)]),
        "npb_task_check": (_cs, [_P(NpbTaskDesc), _ci]),
        "npb_task_clear": (None, [_vp, _vp, _vp]),
        "npb_task_get_state": (None, [_vp] * 5),
        "npb_task_set_state": (None, [_vp] * 5),
        "npb_set_episode_record_task": (None, [_vp, _vp])}),
    ("npb_set_features", {     # the caller's policy inputs: a stack of transformed frames kept behind every step
        "npb_set_features": (None, [_vp, _P(NpbFeaturesDesc)]),
        "npb_features_check": (_cs, [_P(NpbFeaturesDesc), _ci]),
        "npb_features_prime": (None, [_vp, _vp]),
        "npb_features_clear": (None, [_vp, _vp, _vp]),
        "npb_features_get_state": (None, [_vp] * 4),
        "npb_features_set_state": (None, [_vp] * 4)}),
    ("npb_set_controls", {     # the caller's policy outputs: decoded in front of every step
        "npb_set_controls": (None, [_vp, _P(NpbControlsDesc)]),
        "npb_controls_check": (_cs, [_P(NpbControlsDesc), _ci, _ci]),
        "npb_controls_clear": (None, [_vp, _vp, _vp]),
        "npb_controls_get_state": (None, [_vp] * 7),
        "npb_controls_set_state": (None, [_vp] * 7)}),
    ("npb_set_control_orders", {     # order rules on the controls' VALUE axes: a policy orders maintenance
        "npb_set_control_orders": (None, [_vp, _P(NpbControlOrdersDesc)]),
        "npb_control_orders_check": (_cs, [_P(NpbControlOrdersDesc), _P(NpbControlsDesc), _ci, _ci]),
        "npb_control_orders_get_state": (None, [_vp] * 3),
        "npb_control_orders_set_state": (None, [_vp] * 3)}),
    ("npb_set_rollout", {     # the rollout: trajectories recorded on the device, and their GAE advantages
        "npb_set_rollout": (None, [_vp, _P(NpbRolloutDesc)]),
        "npb_rollout_check": (_cs, [_P(NpbRolloutDesc), _ci, _ci, _ci]),
        "npb_rollout_begin": (None, [_vp, _vp]),
        "npb_rollout_steps": (None, [_vp]),
        "npb_rollout_cut": (None, [_vp, _vp, _vp]),
        "npb_rollout_advantages": (None, [_vp, _P(NpbRolloutAdvantagesDesc), _vp])}),
    ("npb_set_normalizer", {     # running observation and reward normalisation, folded behind every step
        "npb_set_normalizer": (None, [_vp, _P(NpbNormalizerDesc)]),
        "npb_normalizer_check": (_cs, [_P(NpbNormalizerDesc), _ci, _P(NpbFeaturesDesc)]),
        "npb_normalizer_training": (None, [_vp, _ci]),
        "npb_normalizer_clear": (None, [_vp, _vp, _vp]),
        "npb_normalizer_get_state": (None, [_vp] * 9),
        "npb_normalizer_set_state": (None, [_vp] * 9)}),
    ("npb_set_policy", {     # the policy on the device: actor, critic, the Gaussian draw, K steps in one call
        "npb_set_policy": (None, [_vp, _P(NpbPolicyDesc)]),
        "npb_policy_check": (_cs, [_P(NpbPolicyDesc), _ci, _ci, _ci]),
        "npb_policy_count": (_i64, [_P(NpbPolicyDesc), _ci, _ci]),
        "npb_policy_load": (None, [_vp, _vp, _ci, _vp]),
        "npb_policy_values": (None, [_vp, _vp, _ci, _ci, _vp, _vp]),
        "npb_policy_noise": (None, [_vp, _u64, _vp, _vp, _vp]),
        "npb_policy_get_state": (None, [_vp, _P(_u64)]),
        "npb_policy_set_state": (None, [_vp, _u64]),
        "npb_collect": (None, [_vp, _ci] + [_vp] * 6)}),
    ("npb_set_policy_core", {     # the recurrent policy: a GRU cell in front of actor and critic, its hidden state carried per plant
        "npb_set_policy_core": (None, [_vp, _P(NpbPolicyDesc), _P(NpbPolicyCore)]),
        "npb_policy_core_check": (_cs, [_P(NpbPolicyCore), _ci, _ci]),
        "npb_policy_core_count": (_i64, [_P(NpbPolicyDesc), _P(NpbPolicyCore), _ci, _ci]),
        "npb_policy_values_hidden": (None, [_vp, _vp, _ci, _ci, _vp, _vp, _vp]),
        "npb_policy_core_get_state": (None, [_vp] * 5),
        "npb_policy_core_set_state": (None, [_vp] * 5)}),
    ("npb_policy_grad", {     # training the policy: the PPO loss, its gradient and the Adam step
        "npb_ppo_check": (_cs, [_P(NpbPpoDesc), _ci, _ci]),
        "npb_policy_grad": (None, [_vp, _P(NpbPpoDesc), _vp]),
        "npb_policy_adam": (None, [_vp, _cd, _cd, _cd, _cd, _vp]),
        "npb_policy_update": (None, [_vp, _P(NpbPpoDesc), _cd, _cd, _cd, _cd, _vp]),
        "npb_policy_get_grad": (None, [_vp, _vp, _vp]),
        "npb_policy_get_stats": (None, [_vp, _vp, _vp]),
        "npb_policy_get_theta": (None, [_vp, _vp, _vp]),
        "npb_policy_optimizer_get_state": (None, [_vp, _vp, _vp, _P(_u64), _vp]),
        "npb_policy_optimizer_set_state": (None, [_vp, _vp, _vp, _u64, _vp])}),
    ("npb_policy_grad_more", {     # training's options: value-loss clipping, the target_kl gate, more statistics
        "npb_ppo_more_check": (_cs, [_P(NpbPpoMore), _ci]),
        "npb_policy_grad_more": (None, [_vp, _P(NpbPpoDesc), _P(NpbPpoMore), _vp]),
        "npb_policy_update_more": (None, [_vp, _P(NpbPpoDesc), _P(NpbPpoMore), _cd, _cd, _cd, _cd, _vp]),
        "npb_policy_train_begin": (None, [_vp, _vp]),
        "npb_policy_train_end": (None, [_vp, _P(ctypes.c_uint32), _vp]),
        "npb_policy_get_stats_more": (None, [_vp, _vp, _vp])}),
    ("npb_policy_shard_sums", {     # one policy across shards: a handle's pinned double sums and the combine of W of them
        "npb_ppo_shard_count": (_i64, [_i64, _ci]),
        "npb_ppo_shards_check": (_cs, [_P(NpbPpoShards), _i64, _ci]),
        "npb_policy_shard_sums": (None, [_vp, _P(NpbPpoDesc), _P(NpbPpoMore), _i64, _vp, _vp]),
        "npb_policy_apply_shards": (None, [_vp, _P(NpbPpoShards), _cd, _cd, _cd, _cd, _vp]),
        "npb_policy_combine_shards": (None, [_vp, _P(NpbPpoShards), _vp])}),
    ("npb_policy_grad_seq", {     # training through time: whole sequences through the recurrent core
        "npb_ppo_seq_check": (_cs, [_P(NpbPpoDesc), _P(NpbPpoSeq), _ci, _ci]),
        "npb_policy_grad_seq": (None, [_vp, _P(NpbPpoDesc), _P(NpbPpoMore), _P(NpbPpoSeq), _vp]),
        "npb_policy_update_seq": (None, [_vp, _P(NpbPpoDesc), _P(NpbPpoMore), _P(NpbPpoSeq), _cd, _cd, _cd, _cd, _vp]),
        "npb_policy_shard_sums_seq": (None, [_vp, _P(NpbPpoDesc), _P(NpbPpoMore), _P(NpbPpoSeq), _i64, _vp, _vp])}),
    ("npb_policy_core_segments", {     # truncated segments: stored start states, segment minibatches, their gradient, the refresh
        "npb_policy_core_segments": (None, [_vp, _ci, _vp, _ci]),
        "npb_policy_core_segments_check": (_cs, [_ci, _vp, _ci, _ci, _ci]),
        "npb_rollout_minibatch_segments": (None, [_vp, _P(NpbMinibatchDesc), _ci, _vp]),
        "npb_minibatch_segments_check": (_cs, [_P(NpbMinibatchDesc), _ci, _ci, _ci, _ci, _ci, _ci]),
        "npb_ppo_segments_check": (_cs, [_P(NpbPpoDesc), _P(NpbPpoSeq), _P(NpbPpoSegments), _ci, _ci]),
        "npb_policy_grad_segments": (None, [_vp, _P(NpbPpoDesc), _P(NpbPpoMore), _P(NpbPpoSeq), _P(NpbPpoSegments), _vp]),
        "npb_policy_update_segments": (None, [_vp, _P(NpbPpoDesc), _P(NpbPpoMore), _P(NpbPpoSeq), _P(NpbPpoSegments), _cd, _cd, _cd, _cd, _vp]),
        "npb_policy_shard_sums_segments": (None, [_vp, _P(NpbPpoDesc), _P(NpbPpoMore), _P(NpbPpoSeq), _P(NpbPpoSegments), _i64, _vp, _vp]),
        "npb_policy_segment_starts": (None, [_vp, _ci, _vp])}),
    ("npb_normalizer_apply_shards", {     # one normaliser and one set of advantage moments across shards
        "npb_normalizer_shard_count": (None, [_vp]),
        "npb_normalizer_shards_check": (_cs, [_vp, _ci]),
        "npb_normalizer_shard_delta": (None, [_vp, _vp, _vp]),
        "npb_normalizer_apply_shards": (None, [_vp, _vp, _ci, _vp]),
        "npb_normalizer_get_base": (None, [_vp, _vp, _vp]),
        "npb_normalizer_set_base": (None, [_vp, _vp, _vp]),
        "npb_moments_shards_check": (_cs, [_P(NpbMomentsDesc), _vp, _vp, _ci, _ci, _vp]),
        "npb_rollout_moments_part": (None, [_vp, _P(NpbMomentsDesc), _ci, _vp, _vp]),
        "npb_rollout_moments_combine": (None, [_vp, _vp, _ci, _ci, _ci, _vp, _vp])}),
    ("npb_rollout_minibatch", {     # pinned moments, the keyed permutation and the minibatch gather over a rollout
        "npb_rollout_moments": (None, [_vp, _P(NpbMomentsDesc), _vp]),
        "npb_rollout_permutation": (None, [_vp, _i64, _P(ctypes.c_uint32), _i64, _i64, _vp, _vp]),
        "npb_rollout_minibatch": (None, [_vp, _P(NpbMinibatchDesc), _vp]),
        "npb_minibatch_check": (_cs, [_P(NpbMinibatchDesc), _ci, _ci, _ci, _ci, _ci])}),
    ("npb_set_event_windows", {     # state windows around events, captured behind every step
        "npb_set_event_windows": (None, [_vp, _P(NpbEventWindowsDesc)]),
        "npb_event_windows_check": (_cs, [_P(NpbEventWindowsDesc), _ci, _ci]),
        "npb_event_windows_clear": (None, [_vp, _vp, _vp]),
        "npb_event_windows_bytes": (_sz, [_P(NpbEventWindowsDesc), _ci])}),
)

_lib = None


def load():
    """Load libnpb.so and declare its entry points from ENTRY_POINTS; raises NpbError when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NpbError("%s not found: build the HIP extension first (make -C nuclear_sim_amd/csrc); "
                       "there is no CPU fallback" % LIB_PATH)
    # PyTorch-ROCm bundles its own HIP runtime; import it first so that libnpb.so binds to the one
    # runtime already in the process (two HIP runtimes in one process do not see the device).
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    for detect, functions in ENTRY_POINTS:
        if detect is not None and not hasattr(L, detect):
            continue
        for name, (restype, argtypes) in functions.items():
            if restype is not None:
                getattr(L, name).restype = restype
            if argtypes is not None:
                getattr(L, name).argtypes = argtypes
    if hasattr(L, "npb_debug_last_step_kernel"):
        # the widths this binding allocates its output blocks with must be the library's: a library that writes more info
        # columns than the caller allocated overruns the buffer (what crashed a round-2 test run on the host side)
        got = (L.npb_obs_dim(), L.npb_info_dim(), L.npb_info_nrho(), L.npb_diag_dim())
        if got != (OBS_DIM, INFO_DIM, INFO_NRHO, DIAG_DIM):
            raise NpbError("libnpb.so writes obs / info / reactivity / diagnostics blocks of width %r, this binding allocates %r: "
                           "rebuild the library or update nuclear_sim_amd/_lib.py" % (got, (OBS_DIM, INFO_DIM, INFO_NRHO, DIAG_DIM)))
    if hasattr(L, "npb_set_control_orders") and \
            tuple(int(L.npb_maint_action_has_handler(a) != 0) for a in range(L.npb_maint_num_actions())) != MAINT_ACTION_HANDLERS:
        raise NpbError("libnpb.so's pump action handlers are not this binding's MAINT_ACTION_HANDLERS: rebuild")
    if hasattr(L, "npb_perform_component_maintenance"):
        catalog = tuple((L.npb_component_kind_name(L.npb_component_action_kind(a)).decode(), L.npb_component_action_name(a).decode())
                        for a in range(L.npb_component_num_actions()))
        if catalog != COMPONENT_ACTIONS:
            raise NpbError("libnpb.so's component catalog is not this binding's COMPONENT_ACTIONS: rebuild")
    if hasattr(L, "npb_perform_turbine_maintenance"):
        catalog = tuple((L.npb_turbine_kind_name(L.npb_turbine_action_kind(a)).decode(), L.npb_turbine_action_name(a).decode())
                        for a in range(L.npb_turbine_num_actions()))
        if catalog != TURBINE_ACTIONS:
            raise NpbError("libnpb.so's turbine catalog is not this binding's TURBINE_ACTIONS: rebuild")
    if hasattr(L, "npb_set_component_maintenance"):
        catalog = tuple((L.npb_component_kind_name(L.npb_component_maint_param_kind(k)).decode(), L.npb_component_maint_param_name(k).decode())
                        for k in range(L.npb_component_maint_num_params()))
        if catalog != CMAINT_PARAMS:
            raise NpbError("libnpb.so's component parameter catalog is not this binding's CMAINT_PARAMS: rebuild")
    if hasattr(L, "npb_carry_diagnostics"):
        table = {L.npb_diag_carried_row(k): L.npb_diag_carried_fresh(k) for k in range(L.npb_diag_num_carried())}
        if table != DIAG_CARRIED_ROWS or list(table) != list(DIAG_CARRIED_ROWS):
            raise NpbError("libnpb.so carries the diagnostics rows %r (include/npb.h NPB_DIAG_CARRIED), this binding's DIAG_CARRIED_ROWS is %r: "
                           "rebuild the library or update nuclear_sim_amd/_lib.py" % (table, DIAG_CARRIED_ROWS))
    if L.npb_num_f64() != SCHEMA.total_f64 or L.npb_num_i32() != SCHEMA.total_i32:
        raise NpbError("libnpb.so was built against a different include/npb_fields.h (%d/%d vs %d/%d): rebuild"
                       % (L.npb_num_f64(), L.npb_num_i32(), SCHEMA.total_f64, SCHEMA.total_i32))
    _lib = L
    return L


def default_params() -> "NpbParams":
    p = NpbParams()
    load().npb_default_params(ctypes.byref(p))
    return p


def check(rc, handle=None):
    if rc != 0:
        msg = load().npb_last_error(handle)
        raise NpbError("libnpb error %d: %s" % (rc, msg.decode() if msg else "?"))
