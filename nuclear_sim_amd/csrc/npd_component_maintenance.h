/*
 * npd_component_maintenance.h -- device physics: the perform_maintenance handlers of a steam generator, the steam-generator
 * system, the condenser and a steam-jet ejector, as a USER calls them between two steps (npb_perform_component_maintenance;
 * catalog NPB_COMPONENT_ACTIONS, include/npb_maint.h).
 *
 * Follows SteamGenerator.perform_maintenance  steam_generator/steam_generator.py:1092-1326,
 *         TSPFoulingModel.perform_cleaning  tsp_fouling_model.py:447-487,
 *         TubeInteriorFouling._primary_scale_cleaning  tube_interior_fouling.py:361-394,
 *         EnhancedSteamGeneratorPhysics.perform_maintenance  steam_generator/enhanced_physics.py:1062-1191,
 *         EnhancedCondenserPhysics.perform_maintenance  condenser/physics.py:1188-1372 (the SECOND definition in the class body:
 *         it replaces the one at :912, and it is the one sim.secondary_physics.condenser.perform_maintenance resolves to),
 *         AdvancedFoulingModel.perform_cleaning  condenser/physics.py:386-441,
 *         WaterChemistry.perform_chemical_treatment  water_chemistry.py:472-523,
 *         SteamJetEjector.perform_maintenance / perform_cleaning  condenser/vacuum_pump.py:309-468.
 *
 * Only what a handler does to CARRIED state (include/npb_fields.h) is restated.  The attributes the handlers also write and
 * the schema does not carry -- total_cleaning_cycles, last_cleaning_time, last_treatment_time, thermal_performance_factor,
 * performance_factor, load_balance_factor, cleaning_effectiveness_history, overall_performance_factor, the tube-interior
 * model's own fouling_fraction -- are never read by a step before it rewrites them: established per action on the live reference
 * by tools/make_component_maintenance_golden.py (the closure check; op_closed in tests/golden/operator_components/).
 * Inspections and tests read state only: success, nothing changes.
 */
#ifndef NPD_COMPONENT_MAINTENANCE_H
#define NPD_COMPONENT_MAINTENANCE_H
#include "npd_sg.h"
#include "npd_chem.h"
#include "npd_condenser.h"

/* component kind of a catalog index (NPB_COMPONENT_*), -1 outside the catalog */
NPD_FN int npd_component_kind(int action) {
  switch (action) {
#define NPD__X(kind, id, name) case NPB_CA_##kind##_##id: return NPB_COMPONENT_##kind;
    NPB_COMPONENT_ACTIONS(NPD__X)
#undef NPD__X
    default: return -1;
  }
}

/* the handlers' default argument is cleaning_type="chemical" everywhere (tube_interior_fouling.py:368, condenser/physics.py:1206,
 * vacuum_pump.py:364) */
NPD_FN int npd_cleaning_type(int option) { return option == NPB_CLEANING_DEFAULT ? NPB_CLEANING_CHEMICAL : option; }

/* TSPFoulingModel.perform_cleaning  tsp_fouling_model.py:447-487 (effectiveness: TSPFoulingConfig.chemical_cleaning_effectiveness
 * 0.75, mechanical 0.85).  It recomputes the fouling fraction, pressure-drop ratio and heat-transfer degradation; the flow
 * maldistribution and fouling stage it also recomputes are not carried (every step derives them anew), and it does NOT evaluate the
 * shutdown conditions: tsp_shutdown_required keeps its value until the next step's update_fouling_state. */
NPD_FN void npd_tsp_perform_cleaning(npb_sg_t *g, double effectiveness) {
#pragma unroll
  for (int level = 0; level < NPB_NUM_TSP; level++) {
    g->tsp_magnetite[level] *= (1.0 - effectiveness);
    g->tsp_copper[level] *= (1.0 - effectiveness * 0.8);
    g->tsp_silica[level] *= (1.0 - effectiveness * 0.9);
    g->tsp_biological[level] *= (1.0 - effectiveness);
  }
  double levels[NPB_NUM_TSP];
  npd_tsp_flow_restriction(g, &g->tsp_fouling_fraction, &g->tsp_pressure_drop_ratio, levels);
  g->tsp_ht_degradation = npd_tsp_ht_degradation(g->tsp_fouling_fraction);
}

/* TubeInteriorFouling._primary_scale_cleaning  tube_interior_fouling.py:361-394 (chemical 0.9, mechanical 0.95 :90-91, else 0.85) */
NPD_FN void npd_scale_cleaning(npb_sg_t *g, int option) {
  const int type = npd_cleaning_type(option);
  const double effectiveness = type == NPB_CLEANING_CHEMICAL ? 0.9 : type == NPB_CLEANING_MECHANICAL ? 0.95 : 0.85;
  double scale_removed = g->scale_thickness * effectiveness;
  g->scale_thickness -= scale_removed;
  g->scale_thickness = npd_pymax(0.0, g->scale_thickness);
  g->scale_iron_oxide *= (1.0 - effectiveness);
  g->scale_crud *= (1.0 - effectiveness);
  g->scale_corrosion *= (1.0 - effectiveness);
  g->scale_thermal_resistance = npd_scale_thermal_resistance(g);
}

/* steam_generator.py:1168-1174 */
NPD_FN void npd_sg_moisture_separator_maintenance(npb_sg_t *g) {
  double current_quality = g->steam_quality;
  double quality_improvement = 0.999 - current_quality;
  g->steam_quality = npd_pymin(0.999, current_quality + quality_improvement * 0.8);
}
/* :1303-1306 */
NPD_FN void npd_sg_routine_maintenance(npb_sg_t *g) { g->steam_quality = npd_pymin(0.999, g->steam_quality + 0.001); }

/* SteamGenerator.perform_maintenance  steam_generator.py:1092-1326: one generator, action of kind NPB_COMPONENT_SG */
NPD_FN void npd_sg_maintenance(npb_sg_t *g, int action, int option) {
  switch (action) {
    case NPB_CA_SG_TSP_CHEMICAL_CLEANING: npd_tsp_perform_cleaning(g, 0.75); break;                 /* :1105-1107 */
    case NPB_CA_SG_TSP_MECHANICAL_CLEANING: npd_tsp_perform_cleaning(g, 0.85); break;               /* :1124-1126 */
    case NPB_CA_SG_MOISTURE_SEPARATOR_MAINTENANCE: npd_sg_moisture_separator_maintenance(g); break;
    case NPB_CA_SG_SCALE_REMOVAL:                                                                   /* :1187-1189 */
    case NPB_CA_SG_TUBE_INTERIOR_SCALE_CLEANING:                                                    /* :1278-1281 */
    case NPB_CA_SG_PRIMARY_SCALE_CLEANING: npd_scale_cleaning(g, option); break;                    /* :1293-1296 */
    case NPB_CA_SG_SECONDARY_SIDE_CLEANING: g->tsp_fouling_fraction *= (1.0 - 0.3); break;          /* :1243-1250 */
    case NPB_CA_SG_ROUTINE_MAINTENANCE: npd_sg_routine_maintenance(g); break;
    /* water_chemistry_adjustment (:1203-1206) resets SteamGenerator.water_chemistry, which is the steam-generator SYSTEM's own
     * WaterChemistry (enhanced_physics.py:130): never updated, at its reset values throughout, parameters here (npb_params.h
     * sgchem_*) -- no carried state moves.  primary_chemistry_optimization (tube_interior_fouling.py:476-500) with its default
     * targets writes the values the three concentrations have.  The rest are inspections and tests. */
    default: break;
  }
}

/* EnhancedSteamGeneratorPhysics.perform_maintenance  enhanced_physics.py:1062-1191: action of kind NPB_COMPONENT_SGSYS, one generator
 * at a time in the order the reference visits them (the caller keeps one generator in registers); *cleaned = how many generators
 * load_balancing_maintenance has cleaned so far, 0 before the first.  system_coordination_maintenance touches no generator. */
NPD_FN int npd_sgsys_touches_generators(int action) { return action != NPB_CA_SGSYS_SYSTEM_COORDINATION_MAINTENANCE; }
NPD_FN void npd_sgsys_maintenance_sg(npb_sg_t *g, int action, int *cleaned) {
  switch (action) {
    case NPB_CA_SGSYS_SYSTEM_STEAM_QUALITY_MAINTENANCE:                                             /* :1090-1099 */
      if (g->steam_quality < 0.99) npd_sg_moisture_separator_maintenance(g);
      break;
    case NPB_CA_SGSYS_LOAD_BALANCING_MAINTENANCE:                                                   /* :1118-1134 */
      /* performance_issues[:2]: chemical TSP cleaning of the first two generators above 5 % degradation */
      if (g->tsp_ht_degradation > 0.05 && *cleaned < 2) { npd_tsp_perform_cleaning(g, 0.75); (*cleaned)++; }
      break;
    case NPB_CA_SGSYS_ROUTINE_MAINTENANCE: npd_sg_routine_maintenance(g); break;                    /* :1156-1160 */
    default: break;
  }
}
/* ... and what the system's handlers do to the system's own carried state: system_coordination_maintenance :1073-1078 */
NPD_FN void npd_sgsys_maintenance_sec(npb_sec_t *sec, int action) {
  if (action == NPB_CA_SGSYS_SYSTEM_COORDINATION_MAINTENANCE) sec->sg_system_availability = 1;
}

/* AdvancedFoulingModel.perform_cleaning  condenser/physics.py:386-441 */
NPD_FN void npd_cond_perform_cleaning(npb_cond_t *cd, int option) {
  const int type = npd_cleaning_type(option);
  double bio_removal, scale_removal, corrosion_removal;
  if (type == NPB_CLEANING_CHEMICAL) { bio_removal = 0.8; scale_removal = 0.6; corrosion_removal = 0.3; }
  else if (type == NPB_CLEANING_MECHANICAL) { bio_removal = 0.5; scale_removal = 0.7; corrosion_removal = 0.8; }
  else if (type == NPB_CLEANING_HYDROBLAST) { bio_removal = 0.9; scale_removal = 0.4; corrosion_removal = 0.9; }
  else { bio_removal = 0.6; scale_removal = 0.5; corrosion_removal = 0.5; }
  double bio_removed = cd->biofouling_thickness * bio_removal;
  double scale_removed = cd->scale_thickness * scale_removal;
  double corrosion_removed = cd->corrosion_product_thickness * corrosion_removal;
  cd->biofouling_thickness -= bio_removed;
  cd->scale_thickness -= scale_removed;
  cd->corrosion_product_thickness -= corrosion_removed;
  cd->time_since_cleaning = 0.0;
  cd->fouling_distribution_factor = 1.0;
  cd->total_fouling_resistance = npd_cond_total_fouling_resistance(cd);
}

/* EnhancedCondenserPhysics.perform_maintenance  condenser/physics.py:1188-1372: action of kind NPB_COMPONENT_COND; chem = the
 * condenser-owned WaterChemistry (chem[1]), read and written by condenser_water_treatment only */
NPD_FN int npd_cond_touches_chemistry(int action) { return action == NPB_CA_COND_CONDENSER_WATER_TREATMENT; }
NPD_FN void npd_cond_maintenance(npb_cond_t *cd, npb_chem_t *chem, int action, int option) {
  switch (action) {
    case NPB_CA_COND_CONDENSER_TUBE_CLEANING: npd_cond_perform_cleaning(cd, option); break;                  /* :1204-1210 */
    case NPB_CA_COND_CONDENSER_CHEMICAL_CLEANING: npd_cond_perform_cleaning(cd, NPB_CLEANING_CHEMICAL); break; /* :1265-1271 */
    case NPB_CA_COND_CONDENSER_WATER_TREATMENT:                                                              /* :1291-1304 */
      /* perform_chemical_treatment("standard")  water_chemistry.py:508-521 (WaterChemistryConfig: ph_optimal 9.2, chlorine_dose_rate
       * 1.0, antiscalant_dose_rate 5.0, corrosion_inhibitor_dose 10.0, treatment_efficiency 0.95) */
      chem->ph += (9.2 - chem->ph) * 0.3;
      chem->chlorine_residual = 1.0;
      chem->antiscalant_concentration = 5.0;
      chem->corrosion_inhibitor_level = 10.0;
      chem->treatment_efficiency = 0.95;
      npd_chem_composites(chem);
      cd->biofouling_thickness *= 0.9;
      cd->scale_thickness *= 0.8;
      cd->corrosion_product_thickness *= 0.7;
      cd->total_fouling_resistance = npd_cond_total_fouling_resistance(cd);
      break;
    case NPB_CA_COND_VACUUM_LEAK_DETECTION: cd->current_air_leakage *= 0.5; break;                           /* :1345-1350 */
    default: break;      /* vacuum_system_test reads state only */
  }
}

/* SteamJetEjector.perform_cleaning  vacuum_pump.py:309-336 */
NPD_FN void npd_ejector_cleaning(npb_cond_t *cd, int e, int type) {
  if (type == NPB_CLEANING_CHEMICAL) {
    cd->ej_nozzle_fouling[e] = npd_pymin(1.0, cd->ej_nozzle_fouling[e] + 0.3);
    cd->ej_diffuser_fouling[e] = npd_pymin(1.0, cd->ej_diffuser_fouling[e] + 0.4);
  } else if (type == NPB_CLEANING_MECHANICAL) {
    cd->ej_nozzle_fouling[e] = npd_pymin(1.0, cd->ej_nozzle_fouling[e] + 0.4);
    cd->ej_diffuser_fouling[e] = npd_pymin(1.0, cd->ej_diffuser_fouling[e] + 0.5);
    cd->ej_nozzle_erosion[e] = npd_pymin(1.0, cd->ej_nozzle_erosion[e] + 0.1);
  } else if (type == NPB_CLEANING_REPLACEMENT) {
    cd->ej_nozzle_fouling[e] = 1.0;
    cd->ej_diffuser_fouling[e] = 1.0;
    cd->ej_nozzle_erosion[e] = 1.0;
  }
}

/* SteamJetEjector.perform_maintenance  vacuum_pump.py:338-468: ejector e, action of kind NPB_COMPONENT_EJECTOR */
NPD_FN void npd_ejector_maintenance(npb_cond_t *cd, int e, int action, int option) {
  switch (action) {
    case NPB_CA_EJECTOR_VACUUM_EJECTOR_CLEANING: npd_ejector_cleaning(cd, e, npd_cleaning_type(option)); break;      /* :364-367 */
    case NPB_CA_EJECTOR_VACUUM_EJECTOR_NOZZLE_REPLACEMENT: npd_ejector_cleaning(cd, e, NPB_CLEANING_REPLACEMENT); break; /* :381-384 */
    case NPB_CA_EJECTOR_VACUUM_EJECTOR_MECHANICAL_CLEANING: npd_ejector_cleaning(cd, e, NPB_CLEANING_MECHANICAL); break; /* :417-420 */
    case NPB_CA_EJECTOR_ROUTINE_MAINTENANCE:                                                                          /* :434-438 */
      cd->ej_nozzle_fouling[e] = npd_pymin(1.0, cd->ej_nozzle_fouling[e] + 0.05);
      cd->ej_diffuser_fouling[e] = npd_pymin(1.0, cd->ej_diffuser_fouling[e] + 0.05);
      break;
    case NPB_CA_EJECTOR_GENERAL:                                                                                      /* :454-460 */
      cd->ej_nozzle_fouling[e] = 1.0;
      cd->ej_diffuser_fouling[e] = 1.0;
      cd->ej_nozzle_erosion[e] = 1.0;
      break;
    default: break;      /* vacuum_ejector_inspection reads state only */
  }
}

#endif
