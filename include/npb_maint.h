/*
 * npb_maint.h -- automatic maintenance of the feedwater pumps (public ABI vocabulary).
 *
 * The reference's control plane for this is three layers (state manager -> orchestrator -> AutoMaintenanceSystem ->
 * component handlers); what a run observes of it is restated in nuclear_sim_amd/csrc/npd_maintenance.h.  This header
 * holds the vocabulary both sides of the C ABI share:
 *
 *  - the PARAMETER catalog: the threshold names of the maintenance configuration that resolve to a value in the
 *    state log of a feedwater pump (StateManager._find_parameter_in_row_data, simulator/state/state_manager.py:1371-1411,
 *    against FeedwaterPump.get_state_dict feedwater/pump_system.py:1062-1086 + FeedwaterPumpLubricationSystem.get_state_dict
 *    feedwater/pump_lubrication.py:1582-1644).  The configuration names 28 more thresholds for the same component
 *    (pump_head, suction_pressure, oil_water_content ...) that never resolve and therefore never fire; they have no
 *    entry here.
 *  - the ACTION catalog: every action those thresholds, the orchestrator's promotions (maintenance_orchestrator.py
 *    :469-524) and the lubrication system's dispatcher (pump_lubrication.py:625-674) can produce.
 *  - the COMPONENT catalog: the maintenance types a user can call directly on steam generators, condenser and ejectors
 *    (npb_perform_component_maintenance); no threshold, work order or table row names them.
 *  - the TURBINE catalog: the maintenance types a user can call directly on the turbine, its bearings, its bearing-lubrication system
 *    and its stages (npb_perform_turbine_maintenance); a catalog of its own, because the COMPONENT catalog's size and kinds are fixed.
 *  - the threshold TABLE a handle carries (npb_set_maintenance_table): per catalogued parameter its rank in the
 *    configuration's dict order (the scan order; -1 = absent), threshold, comparison, action, priority, cooldown and,
 *    for bearing_replacement, which bearing.  npb_maint_table_default() is the table of the data-gen action-test
 *    configuration (data_gen/config_engine/templates/nuclear_plant_comprehensive_config.yaml:682-1010 after the
 *    composer, as the live StateManager.maintenance_thresholds['FWP-1'] holds it; tests/golden/maint_table.json is
 *    that dict dumped from the reference and tests/test_maintenance_cpu.py checks this function against it).
 */
#ifndef NPB_MAINT_H
#define NPB_MAINT_H
#include <stdint.h>

#define NPB_MAINT_NPARAM 16
#define NPB_MAINT_NACT 18

/* parameter catalog: X(id, "name in the state log") */
#define NPB_MAINT_PARAMS(X) \
  X(OIL_LEVEL,               "oil_level") \
  X(OIL_CONTAMINATION_LEVEL, "oil_contamination_level") \
  X(LUBRICATION_EFFECTIVENESS, "lubrication_effectiveness") \
  X(IMPELLER_WEAR,           "impeller_wear") \
  X(CAVITATION_DAMAGE,       "cavitation_damage") \
  X(CAVITATION_INTENSITY,    "cavitation_intensity") \
  X(NPSH_AVAILABLE,          "npsh_available") \
  X(MOTOR_BEARING_WEAR,      "motor_bearing_wear") \
  X(PUMP_BEARING_WEAR,       "pump_bearing_wear") \
  X(THRUST_BEARING_WEAR,     "thrust_bearing_wear") \
  X(SEAL_WEAR,               "seal_wear") \
  X(VIBRATION_LEVEL,         "vibration_level") \
  X(OIL_TEMPERATURE,         "oil_temperature") \
  X(MOTOR_TEMPERATURE,       "motor_temperature") \
  X(SEAL_LEAKAGE_RATE,       "seal_leakage_rate") \
  X(SUM_WEAR_LEVEL,          "sum_wear_level")

/* action catalog: X(id, "MaintenanceActionType value", has_handler) -- has_handler = the lubrication system's
 * perform_maintenance knows it (pump_lubrication.py:642-656); the others execute as "Unknown maintenance type",
 * change no plant state, but are created, queued and counted like any other work order */
#define NPB_MAINT_ACTIONS(X) \
  X(OIL_CHANGE,               "oil_change", 1) \
  X(OIL_TOP_OFF,              "oil_top_off", 1) \
  X(LUBRICATION_SYSTEM_CHECK, "lubrication_system_check", 1) \
  X(IMPELLER_INSPECTION,      "impeller_inspection", 1) \
  X(IMPELLER_REPLACEMENT,     "impeller_replacement", 1) \
  X(CAVITATION_ANALYSIS,      "cavitation_analysis", 0) \
  X(NPSH_ANALYSIS,            "npsh_analysis", 0) \
  X(BEARING_REPLACEMENT,      "bearing_replacement", 1) \
  X(SEAL_REPLACEMENT,         "seal_replacement", 1) \
  X(VIBRATION_ANALYSIS,       "vibration_analysis", 1) \
  X(LUBRICATION_INSPECTION,   "lubrication_inspection", 0) \
  X(MOTOR_INSPECTION,         "motor_inspection", 1) \
  X(COMPONENT_OVERHAUL,       "component_overhaul", 1) \
  X(COMPREHENSIVE_SYSTEM_INSPECTION, "comprehensive_system_inspection", 0) \
  X(BEARING_INSPECTION,       "bearing_inspection", 1) \
  X(OIL_ANALYSIS,             "oil_analysis", 1) \
  X(SYSTEM_CLEANING,          "system_cleaning", 1) \
  X(ROUTINE_MAINTENANCE,      "routine_maintenance", 0)

/* system_cleaning is a handler of the lubrication system but not a value of the reference's MaintenanceActionType enum
 * (systems/maintenance/maintenance_actions.py): a threshold naming it fires, is recorded, and creates no work order */
#define NPB_MAINT_ACTION_IS_TYPE(a) ((a) != NPB_MA_SYSTEM_CLEANING)

enum {
#define NPB__X(id, name) NPB_MP_##id,
  NPB_MAINT_PARAMS(NPB__X)
#undef NPB__X
  NPB_MP_COUNT_
};
enum {
#define NPB__X(id, name, handler) NPB_MA_##id,
  NPB_MAINT_ACTIONS(NPB__X)
#undef NPB__X
  NPB_MA_COUNT_
};

/* COMPONENT catalog (npb_perform_component_maintenance): the maintenance types a user can call directly on a steam generator, the
 * steam-generator system, the condenser and a steam-jet ejector -- X(KIND, id, "maintenance type string").  The index names the handler:
 * a type string may occur under several kinds ("routine_maintenance").  Dispatchers: SteamGenerator.perform_maintenance
 * steam_generator/steam_generator.py:1092-1326, EnhancedSteamGeneratorPhysics.perform_maintenance steam_generator/enhanced_physics.py
 * :1062-1191, EnhancedCondenserPhysics.perform_maintenance condenser/physics.py:1188-1372, SteamJetEjector.perform_maintenance
 * condenser/vacuum_pump.py:338-362 ("general" = its fall-through for every other type); restated in
 * nuclear_sim_amd/csrc/npd_component_maintenance.h.  Every entry has a handler; the inspections and tests among them read state only.
 * Not in the catalog because the live reference raises instead of returning a result: a generator's eddy_current_testing (KeyError
 * 'operating_years', steam_generator.py:1224) and condenser_tube_plugging (AttributeError: CondenserConfig has no tube_count,
 * physics.py:1245). */
#define NPB_COMPONENT_NACT 31
enum { NPB_COMPONENT_SG = 0, NPB_COMPONENT_SGSYS = 1, NPB_COMPONENT_COND = 2, NPB_COMPONENT_EJECTOR = 3, NPB_COMPONENT_NKIND = 4 };
#define NPB_COMPONENT_ACTIONS(X) \
  X(SG, TSP_CHEMICAL_CLEANING,              "tsp_chemical_cleaning") \
  X(SG, TSP_MECHANICAL_CLEANING,            "tsp_mechanical_cleaning") \
  X(SG, TUBE_BUNDLE_INSPECTION,             "tube_bundle_inspection") \
  X(SG, MOISTURE_SEPARATOR_MAINTENANCE,     "moisture_separator_maintenance") \
  X(SG, SCALE_REMOVAL,                      "scale_removal") \
  X(SG, WATER_CHEMISTRY_ADJUSTMENT,         "water_chemistry_adjustment") \
  X(SG, SECONDARY_SIDE_CLEANING,            "secondary_side_cleaning") \
  X(SG, TSP_INSPECTION,                     "tsp_inspection") \
  X(SG, TSP_FLOW_TEST,                      "tsp_flow_test") \
  X(SG, TUBE_INTERIOR_INSPECTION,           "tube_interior_inspection") \
  X(SG, TUBE_INTERIOR_SCALE_CLEANING,       "tube_interior_scale_cleaning") \
  X(SG, TUBE_INTERIOR_EDDY_CURRENT_TESTING, "tube_interior_eddy_current_testing") \
  X(SG, PRIMARY_CHEMISTRY_OPTIMIZATION,     "primary_chemistry_optimization") \
  X(SG, PRIMARY_SCALE_CLEANING,             "primary_scale_cleaning") \
  X(SG, TUBE_EDDY_CURRENT_TESTING,          "tube_eddy_current_testing") \
  X(SG, ROUTINE_MAINTENANCE,                "routine_maintenance") \
  X(SGSYS, SYSTEM_COORDINATION_MAINTENANCE,  "system_coordination_maintenance") \
  X(SGSYS, SYSTEM_STEAM_QUALITY_MAINTENANCE, "system_steam_quality_maintenance") \
  X(SGSYS, LOAD_BALANCING_MAINTENANCE,       "load_balancing_maintenance") \
  X(SGSYS, ROUTINE_MAINTENANCE,              "routine_maintenance") \
  X(COND, CONDENSER_TUBE_CLEANING,          "condenser_tube_cleaning") \
  X(COND, CONDENSER_CHEMICAL_CLEANING,      "condenser_chemical_cleaning") \
  X(COND, CONDENSER_WATER_TREATMENT,        "condenser_water_treatment") \
  X(COND, VACUUM_SYSTEM_TEST,               "vacuum_system_test") \
  X(COND, VACUUM_LEAK_DETECTION,            "vacuum_leak_detection") \
  X(EJECTOR, VACUUM_EJECTOR_CLEANING,            "vacuum_ejector_cleaning") \
  X(EJECTOR, VACUUM_EJECTOR_NOZZLE_REPLACEMENT,  "vacuum_ejector_nozzle_replacement") \
  X(EJECTOR, VACUUM_EJECTOR_INSPECTION,          "vacuum_ejector_inspection") \
  X(EJECTOR, VACUUM_EJECTOR_MECHANICAL_CLEANING, "vacuum_ejector_mechanical_cleaning") \
  X(EJECTOR, ROUTINE_MAINTENANCE,                "routine_maintenance") \
  X(EJECTOR, GENERAL,                            "general")
enum {
#define NPB__X(kind, id, name) NPB_CA_##kind##_##id,
  NPB_COMPONENT_ACTIONS(NPB__X)
#undef NPB__X
  NPB_CA_COUNT_
};
/* units per kind: generators, -, -, ejectors */
#define NPB_COMPONENT_UNITS(kind) ((kind) == NPB_COMPONENT_SG ? 3 : (kind) == NPB_COMPONENT_EJECTOR ? 2 : 1)
/* the cleaning_type kwarg as the option column carries it: DEFAULT = the handler's default argument ("chemical" in all three handlers that
 * take one), OTHER = any string the handler does not name (its "else" branch) */
enum { NPB_CLEANING_DEFAULT = 0, NPB_CLEANING_CHEMICAL = 1, NPB_CLEANING_MECHANICAL = 2, NPB_CLEANING_HYDROBLAST = 3, NPB_CLEANING_REPLACEMENT = 4,
       NPB_CLEANING_OTHER = 5 };

/* TURBINE catalog (npb_perform_turbine_maintenance): the maintenance types a user can call directly on the turbine, one of its bearings,
 * its bearing-lubrication system and one of its stages -- X(KIND, id, "maintenance type string"); a catalog of its own beside the COMPONENT
 * catalog, with indices of its own.  Dispatchers: EnhancedTurbinePhysics.perform_maintenance turbine/enhanced_physics.py:1055-1267 (SYSTEM),
 * BearingModel.perform_maintenance turbine/rotor_dynamics.py:381-564 (BEARING, unit 0..3), TurbineBearingLubricationSystem.perform_maintenance
 * turbine/turbine_bearing_lubrication.py:481-668 (LUBE), TurbineStage.perform_maintenance turbine/stage_system.py:341-377 (STAGE, unit
 * 0..13); restated in nuclear_sim_amd/csrc/npd_turbine_maintenance.h.  A handler is in the catalog exactly when the live reference shows it
 * CLOSED over the carried state: what it writes outside include/npb_fields.h no step reads before rewriting it
 * (tools/make_turbine_maintenance_golden.py, op_closed in tests/golden/operator_turbine/).  Handlers that move no carried member are
 * catalogued all the same: success, nothing stored.  Not in the catalog: a stage's "cleaning", which leaves the stage's
 * blade_condition_factor and actual_efficiency stale for the next step's expansion to read (stage_system.py:353-359, 221-224).
 * LUBE_TURBINE_OIL_TOP_OFF is closed because the lubrication system's oil_level is 100 from construction (no step moves it, and
 * turbine_oil_change sets it to 100): nothing is added, the dilution is 0; were the level carried, the handler would read it. */
#define NPB_TURBINE_NACT 21
enum { NPB_TURBINE_SYSTEM = 0, NPB_TURBINE_BEARING = 1, NPB_TURBINE_LUBE = 2, NPB_TURBINE_STAGE = 3, NPB_TURBINE_NKIND = 4 };
#define NPB_TURBINE_ACTIONS(X) \
  X(SYSTEM, TURBINE_PERFORMANCE_TEST,    "turbine_performance_test") \
  X(SYSTEM, TURBINE_SYSTEM_OPTIMIZATION, "turbine_system_optimization") \
  X(SYSTEM, TURBINE_PROTECTION_TEST,     "turbine_protection_test") \
  X(SYSTEM, THERMAL_STRESS_ANALYSIS,     "thermal_stress_analysis") \
  X(SYSTEM, VIBRATION_ANALYSIS,          "vibration_analysis") \
  X(SYSTEM, ROUTINE_MAINTENANCE,         "routine_maintenance") \
  X(BEARING, TURBINE_BEARING_INSPECTION,  "turbine_bearing_inspection") \
  X(BEARING, TURBINE_BEARING_REPLACEMENT, "turbine_bearing_replacement") \
  X(BEARING, BEARING_CLEARANCE_CHECK,     "bearing_clearance_check") \
  X(BEARING, BEARING_ALIGNMENT,           "bearing_alignment") \
  X(BEARING, THRUST_BEARING_ADJUSTMENT,   "thrust_bearing_adjustment") \
  X(BEARING, TURBINE_OIL_CHANGE,          "turbine_oil_change") \
  X(BEARING, ROUTINE_MAINTENANCE,         "routine_maintenance") \
  X(LUBE, TURBINE_OIL_CHANGE,      "turbine_oil_change") \
  X(LUBE, TURBINE_OIL_TOP_OFF,     "turbine_oil_top_off") \
  X(LUBE, OIL_FILTER_REPLACEMENT,  "oil_filter_replacement") \
  X(LUBE, OIL_COOLER_CLEANING,     "oil_cooler_cleaning") \
  X(LUBE, LUBRICATION_SYSTEM_TEST, "lubrication_system_test") \
  X(LUBE, ROUTINE_MAINTENANCE,     "routine_maintenance") \
  X(STAGE, BLADE_REPLACEMENT, "blade_replacement") \
  X(STAGE, OVERHAUL,          "overhaul")
enum {
#define NPB__X(kind, id, name) NPB_TA_##kind##_##id,
  NPB_TURBINE_ACTIONS(NPB__X)
#undef NPB__X
  NPB_TA_COUNT_
};
/* units per kind: -, bearings, -, stages; the thrust bearing is the third (rotor_dynamics.py:829) */
#define NPB_TURBINE_UNITS(kind) ((kind) == NPB_TURBINE_BEARING ? 4 : (kind) == NPB_TURBINE_STAGE ? 14 : 1)
#define NPB_TURBINE_THRUST_BEARING 2

enum { NPB_CMP_GREATER_THAN = 0, NPB_CMP_LESS_THAN = 1, NPB_CMP_GREATER_EQUAL = 2, NPB_CMP_LESS_EQUAL = 3, NPB_CMP_EQUALS = 4, NPB_CMP_NOT_EQUALS = 5 };
enum { NPB_PRIO_LOW = 1, NPB_PRIO_MEDIUM = 2, NPB_PRIO_HIGH = 3, NPB_PRIO_CRITICAL = 4, NPB_PRIO_EMERGENCY = 5 };
enum { NPB_BEARING_ALL = 0, NPB_BEARING_MOTOR = 1, NPB_BEARING_PUMP = 2, NPB_BEARING_THRUST = 3 };

typedef struct npb_maint_table_t {
  double threshold[NPB_MAINT_NPARAM];
  double cooldown_hours[NPB_MAINT_NPARAM];
  int rank[NPB_MAINT_NPARAM];        /* position in the configuration's dict order; -1 = no such threshold */
  int comparison[NPB_MAINT_NPARAM];
  int action[NPB_MAINT_NPARAM];
  int priority[NPB_MAINT_NPARAM];
  int bearing[NPB_MAINT_NPARAM];     /* threshold's component_id for bearing_replacement (NPB_BEARING_*; 0 = none) */
} npb_maint_table_t;

static inline void npb_maint_table_default(npb_maint_table_t *t) {
#define NPB__T(rk, id, thr, cmp, act, cool, prio, brg) \
  t->rank[NPB_MP_##id] = (rk); t->threshold[NPB_MP_##id] = (thr); t->comparison[NPB_MP_##id] = NPB_CMP_##cmp; \
  t->action[NPB_MP_##id] = NPB_MA_##act; t->cooldown_hours[NPB_MP_##id] = (cool); t->priority[NPB_MP_##id] = NPB_PRIO_##prio; \
  t->bearing[NPB_MP_##id] = NPB_BEARING_##brg;
  NPB__T(0,  OIL_LEVEL,               58.0, LESS_THAN,    OIL_TOP_OFF,              168.0,  HIGH,     ALL)
  NPB__T(1,  OIL_CONTAMINATION_LEVEL, 15.2, GREATER_THAN, OIL_CHANGE,               720.0,  MEDIUM,   ALL)
  NPB__T(2,  LUBRICATION_EFFECTIVENESS, 0.35, LESS_THAN,  LUBRICATION_SYSTEM_CHECK, 720.0,  MEDIUM,   ALL)
  NPB__T(3,  IMPELLER_WEAR,           8.0,  GREATER_THAN, IMPELLER_INSPECTION,      2190.0, MEDIUM,   ALL)
  NPB__T(4,  CAVITATION_DAMAGE,       8.0,  GREATER_THAN, IMPELLER_REPLACEMENT,     4380.0, HIGH,     ALL)
  NPB__T(5,  CAVITATION_INTENSITY,    0.25, GREATER_THAN, CAVITATION_ANALYSIS,      168.0,  HIGH,     ALL)
  NPB__T(6,  NPSH_AVAILABLE,          18.0, LESS_THAN,    NPSH_ANALYSIS,            168.0,  HIGH,     ALL)
  NPB__T(7,  MOTOR_BEARING_WEAR,      8.5,  GREATER_THAN, BEARING_REPLACEMENT,      2190.0, HIGH,     MOTOR)
  NPB__T(8,  PUMP_BEARING_WEAR,       6.5,  GREATER_THAN, BEARING_REPLACEMENT,      2190.0, HIGH,     PUMP)
  NPB__T(9,  THRUST_BEARING_WEAR,     4.5,  GREATER_THAN, BEARING_REPLACEMENT,      2190.0, CRITICAL, THRUST)
  NPB__T(10, SEAL_WEAR,               16.0, GREATER_THAN, SEAL_REPLACEMENT,         2190.0, MEDIUM,   ALL)
  NPB__T(11, VIBRATION_LEVEL,         20.0, GREATER_THAN, VIBRATION_ANALYSIS,       168.0,  HIGH,     ALL)
  NPB__T(12, OIL_TEMPERATURE,         55.0, GREATER_THAN, LUBRICATION_INSPECTION,   168.0,  MEDIUM,   ALL)
  NPB__T(13, MOTOR_TEMPERATURE,       90.0, GREATER_THAN, MOTOR_INSPECTION,         168.0,  MEDIUM,   ALL)
  NPB__T(14, SEAL_LEAKAGE_RATE,       0.15, GREATER_THAN, SEAL_REPLACEMENT,         2190.0, MEDIUM,   ALL)
  NPB__T(15, SUM_WEAR_LEVEL,          75.0, GREATER_THAN, COMPONENT_OVERHAUL,       4380.0, HIGH,     ALL)
#undef NPB__T
}

/* ---- automatic maintenance of the steam generators and the condenser (npb_set_component_maintenance): the rows of the reference's
 * maintenance configuration for SG-0..2 and SECONDARY-COMP-001-COND whose parameter resolves in the component's state-log row
 * (StateManager._find_parameter_in_row_data; every other row of those components resolves to None and is never compared), one table for
 * the three generators.  X(KIND, id, "name in the state log").  Restated in nuclear_sim_amd/csrc/npd_component_auto.h.
 * tube_leak_rate is no carried member (TubeDegradationModel.update_tube_failures computes it from the tubes that failed in this step): the rule
 * recomputes it from the carried members the step leaves behind (npd_component_auto.h, npd_cond_tube_leak_rate).
 * Rows that resolve on the reference and are NOT scanned, by name: efficiency on the fourteen turbine stages and the turbine (0.88 as built
 * against a threshold of 0.30; its action, efficiency_analysis, is in no device catalog): npb_set_component_maintenance has no row for it. */
#define NPB_CMAINT_NPARAM 5
#define NPB_CMAINT_PARAMS(X) \
  X(SG,   TSP_FOULING_FRACTION,  "tsp_fouling_fraction") \
  X(SG,   TUBE_WALL_TEMPERATURE, "tube_wall_temperature") \
  X(SG,   STEAM_QUALITY,         "steam_quality") \
  X(COND, FOULING_RESISTANCE,    "fouling_resistance") \
  X(COND, TUBE_LEAK_RATE,        "tube_leak_rate")
/* the action of the composer's tube_leak_rate row, condenser_tube_plugging, is not in the COMPONENT catalog (an operator cannot order it: the
 * reference's handler raises AttributeError, condenser/physics.py:1245).  As a work order it is created, queued and counted like any other;
 * carried out, the handler has moved the tube counts (plugged + 10, active - 10, :1238-1240) when it raises, AutoMaintenanceSystem catches the
 * exception, and the order completes with success = false (auto_maintenance.py:655-664).  A table row of the condenser may name it by this
 * index behind the catalog. */
#define NPB_CA_AUTO_CONDENSER_TUBE_PLUGGING NPB_COMPONENT_NACT
enum {
#define NPB__X(kind, id, name) NPB_CP_##kind##_##id,
  NPB_CMAINT_PARAMS(NPB__X)
#undef NPB__X
  NPB_CP_COUNT_
};
/* the components in the reference's scan order behind FWP-1..4 (the order of StateManager.maintenance_thresholds): SG-0, SG-1, SG-2, the
 * condenser; rows per component: a generator's three, the condenser's two */
#define NPB_CMAINT_NCOMP 4
#define NPB_CMAINT_COND 3
#define NPB_CMAINT_NROW 3
typedef struct npb_component_maint_table_t {
  double threshold[NPB_CMAINT_NPARAM];
  double cooldown_hours[NPB_CMAINT_NPARAM];
  int rank[NPB_CMAINT_NPARAM];        /* position in the component's dict order; -1 = no such threshold */
  int comparison[NPB_CMAINT_NPARAM];  /* NPB_CMP_* */
  int action[NPB_CMAINT_NPARAM];      /* COMPONENT catalog index (NPB_CA_*) of the row's component kind, or NPB_CA_AUTO_CONDENSER_TUBE_PLUGGING */
  int priority[NPB_CMAINT_NPARAM];    /* NPB_PRIO_* */
} npb_component_maint_table_t;
/* the composer's action-test configuration as the live StateManager.maintenance_thresholds['SG-0'] / ['SECONDARY-COMP-001-COND'] holds it */
static inline void npb_component_maint_table_default(npb_component_maint_table_t *t) {
#define NPB__T(rk, id, thr, cmp, act, cool, prio) \
  t->rank[NPB_CP_##id] = (rk); t->threshold[NPB_CP_##id] = (thr); t->comparison[NPB_CP_##id] = NPB_CMP_##cmp; \
  t->action[NPB_CP_##id] = NPB_CA_##act; t->cooldown_hours[NPB_CP_##id] = (cool); t->priority[NPB_CP_##id] = NPB_PRIO_##prio;
  NPB__T(0, SG_TSP_FOULING_FRACTION,  0.3,   GREATER_THAN, SG_TSP_CHEMICAL_CLEANING,          1.0,    HIGH)
  NPB__T(1, SG_TUBE_WALL_TEMPERATURE, 305.0, GREATER_THAN, SG_SCALE_REMOVAL,                  24.0,   HIGH)
  NPB__T(2, SG_STEAM_QUALITY,         0.9,   LESS_THAN,    SG_MOISTURE_SEPARATOR_MAINTENANCE, 2190.0, HIGH)
  NPB__T(0, COND_FOULING_RESISTANCE,  0.001, GREATER_THAN, COND_CONDENSER_TUBE_CLEANING,      2190.0, MEDIUM)
  NPB__T(4, COND_TUBE_LEAK_RATE,      0.01,  GREATER_THAN, AUTO_CONDENSER_TUBE_PLUGGING,      168.0,  HIGH)
#undef NPB__T
}
/* a generator's primary_scale_cleaning and tube_eddy_current_testing are handlers of SteamGenerator.perform_maintenance but not values of the
 * reference's MaintenanceActionType (systems/maintenance/maintenance_actions.py): a row naming one fires, is stamped, and creates no work
 * order (auto_maintenance.py:338-343).  Every other generator and condenser entry of the COMPONENT catalog is a value. */
#define NPB_CMAINT_ACTION_IS_TYPE(a) ((a) != NPB_CA_SG_PRIMARY_SCALE_CLEANING && (a) != NPB_CA_SG_TUBE_EDDY_CURRENT_TESTING)
/* the side state of that rule, per plant (npb_get_component_maintenance_state / npb_set_...): NPB_CMAINT_SIDE_DOUBLES doubles, member-major
 * -- member m of plant p at [m * n_plants + p] -- with slot = component * NPB_CMAINT_NROW + row (row = the parameter's position among its
 * kind's parameters; the condenser uses rows 0 and 1):
 *   last_violation_time[slot]   StateManager.threshold_last_violation_times[component][parameter]; -1 = never
 *   wo_order[slot]              0 = the component has no open order for the action of row `row`, n = its open order is WO-n (an order is
 *                               filed under the FIRST row of the component that names its action: a (component, action) pair has one slot)
 *   wo_created[slot]            created_date of that order [min]
 *   wo_planned_start[slot]      planned_start_date of that order [min]
 *   wo_priority[slot]           NPB_PRIO_* of that order
 *   last_trigger_time[slot]     AutoMaintenanceSystem.recent_work_order_triggers[component:action]; -1 = never */
#define NPB_CMAINT_NSLOT (NPB_CMAINT_NCOMP * NPB_CMAINT_NROW)
enum { NPB_CMS_LAST_VIOLATION_TIME = 0, NPB_CMS_WO_ORDER = 1, NPB_CMS_WO_CREATED = 2, NPB_CMS_WO_PLANNED_START = 3, NPB_CMS_WO_PRIORITY = 4,
       NPB_CMS_LAST_TRIGGER_TIME = 5, NPB_CMS_NMEMBER = 6 };
#define NPB_CMAINT_SIDE_DOUBLES (NPB_CMS_NMEMBER * NPB_CMAINT_NSLOT)

/* one record of the maintenance event log (npb_set_maintenance_log): a work order created or completed on a feedwater pump.
 * The reference keeps these in WorkOrderManager.work_orders / completed_work_orders (work_orders.py) and the data-gen runner
 * writes them out as *_work_orders.csv / *_maintenance_actions.csv (maintenance_scenario_runner.py:1071-1231). */
/* NPB_MAINT_EVENT_OPERATOR: an action a caller ordered through npb_perform_maintenance and the dispatcher carried out at once (no work
 * order behind it): order = 0, created = planned_start = time = the plant's clock at the call, trigger = priority = 0 */
/* NPB_MAINT_EVENT_OPERATOR_COMPONENT: the same through npb_perform_component_maintenance: action = index of the COMPONENT catalog
 * (NPB_CA_*), the pump byte = the unit (generator 0..2, ejector 0..1; 0 for the system and the condenser), the rest as for OPERATOR */
/* NPB_MAINT_EVENT_OPERATOR_TURBINE: the same through npb_perform_turbine_maintenance: action = index of the TURBINE catalog (NPB_TA_*),
 * the pump byte = the unit (bearing 0..3, stage 0..13; 0 for the turbine and the lubrication system), the rest as for OPERATOR */
/* NPB_MAINT_EVENT_COMPONENT_CREATED / _COMPONENT_COMPLETED: a work order of the automatic maintenance of a steam generator or the
 * condenser (npb_set_component_maintenance): action = index of the COMPONENT catalog (NPB_CA_*), the pump byte = the unit (generator 0..2;
 * 0 for the condenser), the bearing byte = the component kind (NPB_COMPONENT_SG / NPB_COMPONENT_COND), priority = NPB_PRIO_* of the order
 * (kept in the side state: on the completion too), trigger: bit r = row r of the component stamped by the creating scan, the reserved
 * byte = the result's success (a completion; every catalogued handler succeeds), order = the reference's number in the counter the
 * components share with the pumps */
enum { NPB_MAINT_EVENT_CREATED = 0, NPB_MAINT_EVENT_COMPLETED = 1, NPB_MAINT_EVENT_OPERATOR = 2, NPB_MAINT_EVENT_OPERATOR_COMPONENT = 3,
       NPB_MAINT_EVENT_OPERATOR_TURBINE = 4, NPB_MAINT_EVENT_COMPONENT_CREATED = 5, NPB_MAINT_EVENT_COMPONENT_COMPLETED = 6 };
typedef struct npb_maint_event_t {
  double time;            /* the rule's clock: prim.sim_time of the step [min], fp64 under either storage type */
  double created;         /* the order's creation time [min]; for a completion mpump.last_trigger_time[action], which is the open
                           * order's creation time because a second open order for the same (pump, action) is never created */
  double planned_start;   /* mpump.wo_planned_start[action] as the arena holds it [min] */
  int32_t plant;          /* the plant's index within the handle */
  int32_t order;          /* the per-plant creation number n (mpump.wo_order): the reference's work-order id WO-%06d */
  uint16_t trigger;       /* creation: bit q = catalog parameter q whose last_violation_time this scan stamped; 0 for a completion */
  uint8_t pump;           /* 0..3 = FWP-1..4; OPERATOR_COMPONENT / OPERATOR_TURBINE: the unit */
  uint8_t action;         /* action catalog index (NPB_MA_*); OPERATOR_COMPONENT: component catalog index (NPB_CA_*); OPERATOR_TURBINE: NPB_TA_* */
  uint8_t kind;           /* NPB_MAINT_EVENT_CREATED | _COMPLETED | _OPERATOR | _OPERATOR_COMPONENT | _OPERATOR_TURBINE */
  uint8_t priority;       /* creation: NPB_PRIO_* of the order; 0 for a completion (the state does not keep an order's priority) */
  uint8_t bearing;        /* bearing_replacement: NPB_BEARING_* of the order (mpump.wo_bearing); else 0 */
  uint8_t reserved;
} npb_maint_event_t;
#define NPB_MAINT_EVENT_BYTES 40

/* ---- the per-plant work-order summary (npb_set_maintenance_summary): the event log folded, on the device, into four numbers per (key, plant)
 * -- what the data-gen runner returns of a finished scenario (whether the target action fired, work orders created and executed after
 * tracking_start_hours, and when: maintenance_scenario_runner.py:431-468) and what the timing optimiser reads of a probe run (the time the
 * target action first fired: optimization/timing_optimizer.py:273-320).
 * A key selects records: `catalog` NPB_MAINT_CATALOG_* (a record's catalog follows from its kind: NPB_MAINT_EVENT_CREATED, _COMPLETED and
 * _OPERATOR are feedwater, _OPERATOR_COMPONENT, _COMPONENT_CREATED and _COMPONENT_COMPLETED are component, _OPERATOR_TURBINE is turbine),
 * `action` the index into that catalog (NPB_MA_* / NPB_CA_*, NPB_CA_AUTO_CONDENSER_TUBE_PLUGGING included / NPB_TA_*) or -1 = any action of
 * it, `unit` the record's pump / unit byte or -1 = any, `kinds` a mask over NPB_MAINT_EVENT_*: bit k = records of kind k match.  One
 * record may match several keys.
 * For key j and plant p the caller owns four device tables, member-major, element [j * n_plants + p]:
 *   first_created    double, +inf = never     n_created    int32
 *   first_completed  double, +inf = never     n_completed  int32
 * A matching record of a creation kind (_CREATED, _COMPONENT_CREATED) feeds the created pair, one of any other kind the completed pair: an
 * operator action counts as a completion at the time of the call.  The time is the record's `time` [plant minutes, fp64 under either
 * storage type]; records with time < since_minutes are dropped (the runner's tracking_start_hours).
 * Several records of one fold may hit one cell (the four pumps of a plant can each create oil_top_off in one step): counts move by integer
 * atomic adds, times by a 64-bit UNSIGNED atomic minimum on the double's bit pattern.  PRECONDITION: every record's time is >= +0.0 -- a
 * plant's clock starts at 0 and only grows -- so that the order of the bit patterns is the order of the values; a negative time, -0.0 or a
 * NaN has a larger pattern than +inf and never wins.  The tables are therefore a function of the SET of records folded, bit for bit,
 * whatever order the device visits them in.  The caller initialises them with the bit pattern of +inf and 0 (npb_maint_summary_clear). */
#define NPB_MAINT_SUMMARY_MAX_KEYS 16
enum { NPB_MAINT_CATALOG_FEEDWATER = 0, NPB_MAINT_CATALOG_COMPONENT = 1, NPB_MAINT_CATALOG_TURBINE = 2, NPB_MAINT_NCATALOG = 3 };
/* the record kinds of each catalog, as masks over NPB_MAINT_EVENT_*, and the creation kinds among them */
#define NPB_MAINT_CATALOG_KINDS(c) ((c) == NPB_MAINT_CATALOG_FEEDWATER ? 0x07u : (c) == NPB_MAINT_CATALOG_COMPONENT ? 0x68u : (c) == NPB_MAINT_CATALOG_TURBINE ? 0x10u : 0u)
#define NPB_MAINT_CREATION_KINDS 0x21u
typedef struct npb_maint_summary_key_t {
  int32_t catalog;        /* NPB_MAINT_CATALOG_* */
  int32_t action;         /* index into the catalog, -1 = any */
  int32_t unit;           /* pump 0..3 / the component's or the turbine part's unit, -1 = any */
  uint32_t kinds;         /* bit k = NPB_MAINT_EVENT_* k matches; at least one kind of the key's catalog */
} npb_maint_summary_key_t;
typedef struct npb_maint_summary_desc_t {
  int32_t n_keys;         /* 1 .. NPB_MAINT_SUMMARY_MAX_KEYS */
  int32_t consume;        /* 0 = keep mode, 1 = consume mode (include/npb.h npb_set_maintenance_summary) */
  double since_minutes;
  npb_maint_summary_key_t keys[NPB_MAINT_SUMMARY_MAX_KEYS];
  double *first_created, *first_completed;      /* device, [n_keys][n_plants], 8-byte aligned */
  int32_t *n_created, *n_completed;             /* device, [n_keys][n_plants], 4-byte aligned */
  uint32_t *folded, *dropped;                   /* device, one word each, 4-byte aligned */
} npb_maint_summary_desc_t;
#ifdef __cplusplus
static_assert(sizeof(npb_maint_event_t) == NPB_MAINT_EVENT_BYTES, "npb_maint_event_t layout");
static_assert(NPB_MAINT_NPARAM <= 16 && NPB_MAINT_NACT <= 255 && NPB_COMPONENT_NACT <= 255, "npb_maint_event_t field widths");
static_assert(NPB_CA_COUNT_ == NPB_COMPONENT_NACT, "NPB_COMPONENT_NACT");
static_assert(NPB_TA_COUNT_ == NPB_TURBINE_NACT && NPB_TURBINE_NACT <= 255, "NPB_TURBINE_NACT");
#else
_Static_assert(sizeof(npb_maint_event_t) == NPB_MAINT_EVENT_BYTES, "npb_maint_event_t layout");
#endif

#endif /* NPB_MAINT_H */
