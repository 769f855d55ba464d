/*
 * npd_turbine_maintenance.h -- device physics: the perform_maintenance handlers of the turbine, one of its bearings, its
 * bearing-lubrication system and one of its stages, as a USER calls them between two steps (npb_perform_turbine_maintenance;
 * catalog NPB_TURBINE_ACTIONS, include/npb_maint.h).
 *
 * Follows EnhancedTurbinePhysics.perform_maintenance  turbine/enhanced_physics.py:1055-1267,
 *         TurbineProtectionSystem.reset_protection_system  turbine/enhanced_physics.py:473-479,
 *         BearingModel.perform_maintenance  turbine/rotor_dynamics.py:381-564,
 *         TurbineBearingLubricationSystem.perform_maintenance  turbine/turbine_bearing_lubrication.py:481-668,
 *         TurbineStage.perform_maintenance  turbine/stage_system.py:341-377.
 *
 * Only what a handler does to CARRIED state (include/npb_fields.h) is restated.  What the handlers also write and the schema does
 * not carry is either reassigned by every step before anything reads it -- a bearing's efficiency_factor (rotor_dynamics.py:303),
 * the turbine's performance_factor and availability_factor (enhanced_physics.py:828-829), overall_efficiency, the thermal tracker's
 * max_thermal_stress and thermal_shock_risk -- or read by no physics: a bearing's clearance_increase, vibration_displacement,
 * vibration_velocity and oil_contamination_level, the stage system's system_efficiency, the protection system's system_available,
 * trip_time and emergency_actions.  Established per call on the live reference by tools/make_turbine_maintenance_golden.py (the
 * closure check; op_closed in tests/golden/operator_turbine/).  Two attributes the lubrication system's handlers READ are
 * construction constants: oil_level is 100 (no step moves it; turbine_oil_change sets it to 100) and oil_cooling_effectiveness is 1
 * (update_turbine_lubrication_effects, the only other writer, is called by no step; the handler's min(1.0, 1 + 0.15) keeps it).
 * Inspections, tests and analyses that move no carried member: success, nothing changes.
 */
#ifndef NPD_TURBINE_MAINTENANCE_H
#define NPD_TURBINE_MAINTENANCE_H
#include "npd_turbine.h"

/* turbine kind of a catalog index (NPB_TURBINE_*), -1 outside the catalog */
NPD_FN int npd_turbine_kind(int action) {
  switch (action) {
#define NPD__X(kind, id, name) case NPB_TA_##kind##_##id: return NPB_TURBINE_##kind;
    NPB_TURBINE_ACTIONS(NPD__X)
#undef NPD__X
    default: return -1;
  }
}

/* EnhancedTurbinePhysics.perform_maintenance  enhanced_physics.py:1055-1267: action of kind NPB_TURBINE_SYSTEM */
NPD_FN void npd_turbine_system_maintenance(npb_turb_t *t, int action) {
  switch (action) {
    case NPB_TA_SYSTEM_TURBINE_SYSTEM_OPTIMIZATION:                                                 /* :1119-1122 */
      t->lub_effectiveness = npd_pymin(1.0, t->lub_effectiveness + 0.05);
      break;
    case NPB_TA_SYSTEM_TURBINE_PROTECTION_TEST:                                                     /* :1146-1147 */
      if (t->trip_active) {      /* reset_protection_system :473-479 */
        t->trip_active = 0;
        t->trip_latched_mask = 0;
        t->timer_overspeed = 0.0; t->timer_vibration = 0.0; t->timer_bearing_temp = 0.0;
      }
      break;
    case NPB_TA_SYSTEM_VIBRATION_ANALYSIS: t->thermal_bow *= 0.7; break;                            /* :1215-1216 */
    case NPB_TA_SYSTEM_ROUTINE_MAINTENANCE:                                                         /* :1245-1247 */
#pragma unroll
      for (int b = 0; b < 4; b++) t->bearing_metal_temp[b] = npd_pymax(80.0, t->bearing_metal_temp[b] - 0.5);
      break;
    /* turbine_performance_test (:1066-1101) and thermal_stress_analysis (:1169-1192) write overall_efficiency, performance_factor and
     * the thermal tracker's stress figures: every step reassigns them before anything reads them */
    default: break;
  }
}

/* BearingModel.perform_maintenance  rotor_dynamics.py:381-564: bearing b (a constant index at the call), action of kind
 * NPB_TURBINE_BEARING.  thrust_bearing_adjustment on a journal bearing is refused before this is called (npd_turbine_order_ok). */
NPD_FN void npd_turbine_bearing_maintenance(npb_turb_t *t, int b, int action) {
  switch (action) {
    case NPB_TA_BEARING_TURBINE_BEARING_REPLACEMENT:                                                /* :425-428 */
      t->bearing_wear_factor[b] = 1.0;
      t->bearing_metal_temp[b] = npd_pymin(t->bearing_metal_temp[b], 90.0);
      break;
    case NPB_TA_BEARING_THRUST_BEARING_ADJUSTMENT: t->bearing_metal_temp[b] = npd_pymax(80.0, t->bearing_metal_temp[b] - 5.0); break;   /* :492 */
    case NPB_TA_BEARING_TURBINE_OIL_CHANGE: t->bearing_metal_temp[b] = npd_pymax(80.0, t->bearing_metal_temp[b] - 2.0); break;          /* :524 */
    case NPB_TA_BEARING_ROUTINE_MAINTENANCE: t->bearing_metal_temp[b] = npd_pymax(80.0, t->bearing_metal_temp[b] - 1.0); break;         /* :544 */
    /* turbine_bearing_inspection reads state only; bearing_clearance_check (:445-453) and bearing_alignment (:469-474) move the
     * clearance, the efficiency factor and the bearing's own vibration figures, none of them carried or read by a step */
    default: break;
  }
}

/* TurbineBearingLubricationSystem.perform_maintenance  turbine_bearing_lubrication.py:481-668: action of kind NPB_TURBINE_LUBE */
NPD_FN void npd_turbine_lube_maintenance(npb_turb_t *t, int action) {
  const double oil_level = 100.0, oil_cooling_effectiveness = 1.0;      /* construction constants: see the head of this file */
  switch (action) {
    case NPB_TA_LUBE_TURBINE_OIL_CHANGE:                                                            /* :499-508 */
      t->lub_oil_contamination = 1.0;
      t->lub_oil_acidity = 0.05;
      t->lub_oil_moisture = 0.01;
      t->lub_effectiveness = npd_pymin(1.0, t->lub_effectiveness + 0.15);
      t->lub_oil_temperature = npd_pymax(45.0, t->lub_oil_temperature - 5.0);
      break;
    case NPB_TA_LUBE_TURBINE_OIL_TOP_OFF: {                                                         /* :528-535 */
      double oil_added = npd_pymin(100.0 - oil_level, 50.0);
      double dilution_factor = oil_added / 100.0;
      t->lub_oil_contamination = npd_pymax(1.0, t->lub_oil_contamination - dilution_factor * 2.0);
      t->lub_oil_acidity = npd_pymax(0.05, t->lub_oil_acidity - dilution_factor * 0.1);
      break;
    }
    case NPB_TA_LUBE_OIL_FILTER_REPLACEMENT: {                                                      /* :553-558 */
      double contamination_reduction = npd_pymin(5.0, t->lub_oil_contamination * 0.6);
      t->lub_oil_contamination -= contamination_reduction;
      t->lub_oil_contamination = npd_pymax(1.0, t->lub_oil_contamination);
      t->lub_effectiveness = npd_pymin(1.0, t->lub_effectiveness + 0.05);
      break;
    }
    case NPB_TA_LUBE_OIL_COOLER_CLEANING: {                                                         /* :574-585; 'oil_coolers' is the fifth component */
      double temp_reduction = (1.0 - oil_cooling_effectiveness) * 15.0;
      t->lub_oil_temperature = npd_pymax(45.0, t->lub_oil_temperature - temp_reduction);
      t->lub_wear[4] = npd_pymax(0.0, t->lub_wear[4] - 5.0);
      break;
    }
    case NPB_TA_LUBE_LUBRICATION_SYSTEM_TEST: t->lub_effectiveness = npd_pymin(1.0, t->lub_effectiveness + 0.1); break;   /* :605 */
    case NPB_TA_LUBE_ROUTINE_MAINTENANCE:                                                           /* :642-648 */
      t->lub_effectiveness = npd_pymin(1.0, t->lub_effectiveness + 0.02);
      t->lub_oil_contamination = npd_pymax(1.0, t->lub_oil_contamination - 0.5);
      t->lub_oil_temperature = npd_pymax(45.0, t->lub_oil_temperature - 1.0);
#pragma unroll
      for (int c = 0; c < 5; c++) t->lub_wear[c] = npd_pymax(0.0, t->lub_wear[c] - 0.5);
      break;
    default: break;
  }
}

/* TurbineStage.perform_maintenance  stage_system.py:341-377: one stage's three carried members, action of kind NPB_TURBINE_STAGE.
 * The fouling factor, blade condition factor and actual efficiency the handlers also set are what the step derives from these three
 * when it reads them (npd_turbine.h): after blade_replacement and overhaul the two agree ("cleaning", where they do not, is not
 * offered). */
NPD_FN void npd_turbine_stage_maintenance(double *efficiency_degradation, double *deposit_thickness, double *blade_wear_factor, int action) {
  switch (action) {
    case NPB_TA_STAGE_BLADE_REPLACEMENT: *blade_wear_factor = 1.0; break;                           /* :363 */
    case NPB_TA_STAGE_OVERHAUL:                                                                     /* :369-373 */
      *deposit_thickness = 0.0;
      *blade_wear_factor = 1.0;
      *efficiency_degradation = 0.0;
      break;
    default: break;
  }
}

/* what the reference's result says of an order: a catalogued type on a unit that exists; the thrust adjustment on the thrust bearing
 * only ("Bearing type journal is not a thrust bearing", rotor_dynamics.py:504-511) */
NPD_FN bool npd_turbine_order_ok(int kind, int action, int unit) {
  if (kind < 0 || unit < 0 || unit >= NPB_TURBINE_UNITS(kind)) return false;
  if (action == NPB_TA_BEARING_THRUST_BEARING_ADJUSTMENT && unit != NPB_TURBINE_THRUST_BEARING) return false;
  return true;
}

#endif
