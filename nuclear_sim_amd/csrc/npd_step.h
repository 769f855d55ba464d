/*
 * npd_step.h -- device physics: the plant-level glue of NuclearPlantSimulator.step around the subsystems
 * (simulator/core/sim.py:130-258, 290-333, 429-542; SecondaryReactorPhysics.update_system, systems/secondary/__init__.py:371-932):
 * the per-step inputs, the secondary prelude, the electrical-power gates, the feedback into the primary state, the
 * observation row, the reward and the info row.
 *
 * One statement of each formula for every step kernel (npb_kernels.hip, npd_step1.h, npd_step2.h, npd_step4.h): the
 * arguments are scalars or section structs, so a multi-wave kernel passes what it has read back from its LDS slots.
 * Each function keeps the reference's expression order (the build does not contract, so the same order is the same bits).
 * Two pieces stay written out in each kernel because as functions they compiled to different compare / select code: the
 * power-setpoint clip before npd_primary_update, and the primary side's trip bits (NPB_TRIP_SCRAM, _SCRAM_FIRED, _NAN_RESET).
 */
#ifndef NPD_STEP_H
#define NPD_STEP_H
#include "npd_common.h"
#include "npd_condenser.h"

/* what step() receives for plant p (sim.py:130-133); a NULL array is the default of its argument */
NPD_FN npd_inputs_t npd_step_inputs(bool live, size_t p, const int32_t *action, const double *magnitude, const double *setpoint,
                                    const double *noise_z, const double *cw_temp) {
  npd_inputs_t in;
  in.action = (live && action) ? action[p] : 8;
  in.magnitude = (live && magnitude) ? magnitude[p] : 1.0;
  in.power_setpoint = (live && setpoint) ? setpoint[p] : NAN;
  in.noise_z = (live && noise_z) ? noise_z[p] : 0.0;
  in.cooling_water_temp = (live && cw_temp) ? cw_temp[p] : NAN;
  return in;
}

/* ---- secondary prelude (secondary/__init__.py:371-453) */
/* the feedwater temperature blend */
NPD_FN double npd_feedwater_temp(double prev_feedwater_temp) {
  const double estimated_feedwater_temp = 40.0 + 187.0;
  const double alpha = 0.1;
  return (alpha * estimated_feedwater_temp + (1 - alpha) * prev_feedwater_temp);
}
/* primary_thermal_power: the sum of the three loops' coupling powers */
NPD_FN double npd_load_demand_fraction(double primary_thermal_power) {
  double load_demand_fraction = npd_pymin(1.0, primary_thermal_power / 3000.0);
  return npd_pymax(load_demand_fraction, 0.2);
}
/* :447-453: a plant's first step (no previous SG conditions) takes hard-coded values, not the SG initial conditions */
NPD_FN void npd_first_step_sg_conditions(double load_demand_fraction, double *prev_levels, double *prev_flows, double *prev_quals) {
#pragma unroll
  for (int i = 0; i < NPB_NUM_SG; i++) { prev_levels[i] = 12.5; prev_flows[i] = 555.0 * load_demand_fraction; prev_quals[i] = 0.99; }
}

/* LP exhaust quality handed to the condenser (secondary/__init__.py:591-621), at the given condenser pressure */
NPD_FN double npd_lp_exhaust_quality(double condenser_pressure, double lp6_outlet_enthalpy) {
  double lp_exhaust_quality = 0.90;
  double h_f = npd_cond_hf(condenser_pressure), h_g = npd_cond_hg(condenser_pressure);
  double h_fg = h_g - h_f;
  if (h_fg > 0) {
    lp_exhaust_quality = (lp6_outlet_enthalpy - h_f) / h_fg;
    lp_exhaust_quality = npd_pymax(0.0, npd_pymin(1.0, lp_exhaust_quality));
  }
  return lp_exhaust_quality;
}

/* ---- electrical-power gates (secondary/__init__.py:750-932) */
typedef struct npd_power_t {
  double electrical_power, thermal_efficiency;
  double heat_rejection;                 /* total_system_heat_rejection, W */
} npd_power_t;
NPD_FN npd_power_t npd_power_gates(double turbine_electrical_power, double primary_thermal_power, double fw_total_flow,
                                   double sg_total_steam, double sg_avg_pressure) {
  npd_power_t r;
  r.heat_rejection = (primary_thermal_power - turbine_electrical_power) * 1e6;
  double power_reduction_factor = 1.0;
  if (fw_total_flow < 300.0) power_reduction_factor = 0.0;
  if (power_reduction_factor > 0.0) {
    if (sg_total_steam < (300.0 * 0.5)) power_reduction_factor *= 0.1;
    if (sg_avg_pressure < (1.0 * 0.5)) power_reduction_factor *= 0.1;
    if (primary_thermal_power > (primary_thermal_power * 1.1)) power_reduction_factor = 0.0;
  }
  r.electrical_power = turbine_electrical_power * power_reduction_factor;
  r.thermal_efficiency = (primary_thermal_power > 0) ? r.electrical_power / primary_thermal_power : 0.0;
  return r;
}

/* the secondary section's outputs and flags after the step (its narrow members; the caller stores them as whole columns) */
NPD_FN npb_sec_t npd_sec_outputs(double electrical_power, double thermal_efficiency, double total_steam_flow, double total_heat_transfer,
                                 double total_feedwater_flow, double load_demand, double sg_avg_pressure, double sg_avg_temperature,
                                 double sg_avg_quality, int sg_system_availability) {
  npb_sec_t so;
  so.electrical_power_output = electrical_power; so.thermal_efficiency = thermal_efficiency;
  so.total_steam_flow = total_steam_flow; so.total_heat_transfer = total_heat_transfer; so.total_feedwater_flow = total_feedwater_flow;
  so.load_demand = load_demand; so.sg_avg_pressure = sg_avg_pressure; so.sg_avg_temperature = sg_avg_temperature;
  so.sg_avg_quality = sg_avg_quality; so.has_previous_sg_conditions = 1; so.sg_system_availability = sg_system_availability;
  return so;
}

/* _apply_secondary_to_primary_feedback  sim.py:429-498: the heat-removal factor left in the primary state (beside
 * steam_flow_rate = the total steam flow) */
NPD_FN double npd_heat_removal_factor(double sg_total_steam, bool fw_available) {
  double heat_removal_factor = sg_total_steam / 1665.0;
  if (!fw_available) heat_removal_factor *= 0.5;
  return heat_removal_factor;
}

/* ---- get_observation  sim.py:290-333 */
/* the primary part (obs[7], the steam flow, is the primary state's: the step's feedback sets it afterwards) */
NPD_FN void npd_obs_primary(const npb_prim_t &s, double *obs) {
  obs[0] = s.neutron_flux / 1e12;
  obs[1] = s.fuel_temperature / 1000;
  obs[2] = s.coolant_temperature / 300;
  obs[3] = s.coolant_pressure / 20;
  obs[4] = s.coolant_flow_rate / 50000;
  obs[5] = s.steam_temperature / 300;
  obs[6] = s.steam_pressure / 10;
  obs[7] = s.steam_flow_rate / 3000;
  obs[8] = s.control_rod_position / 100;
  obs[9] = s.steam_valve_position / 100;
  obs[10] = s.power_level / 100;
  obs[11] = (double)(s.scram_status != 0);
}
/* obs[7] from the primary state's steam_flow_rate, obs[12..21] from the secondary side */
NPD_FN void npd_obs_secondary(double *obs, double steam_flow_rate, double electrical_power, double thermal_efficiency, double total_steam_flow,
                              double load_demand, double cooling_water_temperature, double fw_total_flow, double fw_total_power,
                              double fw_available) {
  obs[7] = steam_flow_rate / 3000;
  obs[12] = electrical_power / 1100;
  obs[13] = thermal_efficiency / 0.35;
  obs[14] = total_steam_flow / 1665;
  obs[15] = load_demand / 100;
  obs[16] = 227.0 / 250;
  obs[17] = cooling_water_temperature / 35;
  obs[18] = fw_total_flow / 1665;
  obs[19] = fw_total_power / 40;
  obs[20] = fw_available;
  obs[21] = fw_total_flow / 1665;
}

/* ---- calculate_reward */
/* calculate_reward(None)  sim.py:503-519: the primary-only reward, and the base of the full one */
NPD_FN double npd_base_reward(const npb_prim_t &s) {
  double power_reward = -fabs(s.power_level - 100) / 100;
  double temp_penalty = 0, pressure_penalty = 0;
  if (s.fuel_temperature > 800) temp_penalty = -(s.fuel_temperature - 800) / 100;
  if (s.coolant_pressure > 16) pressure_penalty = -(s.coolant_pressure - 16);
  double scram_penalty = s.scram_status ? -100 : 0;
  return power_reward + temp_penalty + pressure_penalty + scram_penalty;
}
/* calculate_reward(secondary_state)  sim.py:521-542 */
NPD_FN double npd_reward(double base_reward, double thermal_efficiency, double load_demand, double electrical_power, double sg_avg_pressure,
                         double condenser_pressure) {
  double efficiency_reward = (thermal_efficiency - 0.30) * 10;
  double target_electrical_power = load_demand / 100.0 * 1100.0;
  double electrical_reward = -fabs(electrical_power - target_electrical_power) / 100;
  double steam_pressure_penalty = 0;
  if (sg_avg_pressure < 5.0 || sg_avg_pressure > 8.0) steam_pressure_penalty = -fabs(sg_avg_pressure - 6.895) * 5;
  double condenser_penalty = 0;
  if (condenser_pressure > 0.01) condenser_penalty = -(condenser_pressure - 0.007) * 100;
  double secondary_reward = efficiency_reward + electrical_reward + steam_pressure_penalty + condenser_penalty;
  return base_reward + secondary_reward * 0.5;
}

/* ---- info  sim.py:199-250 */
NPD_FN void npd_info_primary(double *info, double thermal_power_mw, double total_reactivity_pcm, double sim_time) {
  info[NPB_INFO_THERMAL_POWER] = thermal_power_mw;
  info[NPB_INFO_REACTIVITY_PCM] = total_reactivity_pcm;
  info[NPB_INFO_TIME] = sim_time;
}
/* the secondary columns, with the non-finite substitutions of :231-240 */
NPD_FN void npd_info_secondary(double *info, double electrical_power, double thermal_efficiency, double steam_flow, double steam_pressure,
                               double condenser_pressure, double heat_rejection, double fw_total_flow, double sg_heat_transfer,
                               double turbine_power, double fw_total_power, double primary_thermal_power, double turbine_efficiency,
                               double turbine_hp_power, double turbine_lp_power) {
  info[NPB_INFO_ELECTRICAL_POWER] = isfinite(electrical_power) ? electrical_power : 0.0;
  info[NPB_INFO_THERMAL_EFFICIENCY] = npd_pymax(0.0, npd_pymin(isfinite(thermal_efficiency) ? thermal_efficiency : 0.0, 0.35));
  info[NPB_INFO_STEAM_FLOW] = isfinite(steam_flow) ? steam_flow : 1665.0;
  info[NPB_INFO_STEAM_PRESSURE] = isfinite(steam_pressure) ? steam_pressure : 6.895;
  info[NPB_INFO_CONDENSER_PRESSURE] = isfinite(condenser_pressure) ? condenser_pressure : 0.007;
  info[NPB_INFO_CONDENSER_HEAT_REJECTION] = isfinite(heat_rejection) ? heat_rejection : 0.0;
  info[NPB_INFO_FEEDWATER_FLOW] = fw_total_flow;
  info[NPB_INFO_SG_HEAT_TRANSFER] = sg_heat_transfer;
  info[NPB_INFO_TURBINE_POWER] = turbine_power;
  info[NPB_INFO_FEEDWATER_POWER] = fw_total_power;
  info[NPB_INFO_PRIMARY_THERMAL_POWER] = primary_thermal_power;
  info[NPB_INFO_TURBINE_EFFICIENCY] = turbine_efficiency;
  info[NPB_INFO_TURBINE_HP_POWER] = turbine_hp_power;
  info[NPB_INFO_TURBINE_LP_POWER] = turbine_lp_power;
}

#endif
