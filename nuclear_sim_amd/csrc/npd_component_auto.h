/*
 * npd_component_auto.h -- device side of the automatic maintenance of the steam generators and the condenser
 * (npb_set_component_maintenance; vocabulary and side state: include/npb_maint.h, NPB_CMAINT_*).
 *
 * The reference runs these components through the same control plane as the feedwater pumps (npd_maintenance.h): the state manager
 * scans StateManager.maintenance_thresholds in dict order -- FWP-1..4, SG-0..2, the turbine's stages, the condenser
 * (state_manager.py:1307-1369) -- with one last-violation stamp and cooldown per (component, row); the violations of one component go to
 * the orchestrator, and one event per component reaches AutoMaintenanceSystem._create_automatic_work_order (auto_maintenance.py:332-453),
 * which numbers every order from ONE counter and executes ONE due order per check, the earliest created of any component (:468-582).
 *
 * The orchestrator for these ids (maintenance_orchestrator.py:165-178, 239-357, 549-605):
 *   "SG-<i>" is a 'steam_generator'.  With at most three violations per generator only tube_bundle_overhaul can be reached (three
 *   violation actions among its `encompasses`; its *_threshold conditions and every promotion rule name parameters -- 'fouling',
 *   'heat_transfer_degradation', 'fouling_fraction', 'scale_thickness' ... -- that no scanned row carries), and tube_bundle_overhaul is not a
 *   MaintenanceActionType: the event creates no order (auto_maintenance.py:338-343).  A coordination keeps the requested action.
 *   "SECONDARY-COMP-001-COND" contains none of 'fwp', 'tb', 'turbine', 'sg', 'cd', 'condenser' in lower case: type 'unknown', no
 *   hierarchy, the requested action -- the first violation's -- as it is.
 * An order's handler is the component's own perform_maintenance(maintenance_type=action) with default arguments
 * (auto_maintenance.py:584-626): npd_component_maintenance.h.  A handler that raises is caught there, counted in
 * maintenance_actions_performed all the same and the order completed: "an order is open iff created > performed" holds for every order.
 *
 * The condenser's tube_leak_rate row orders condenser_tube_plugging, the one handler that does raise: plugged + 10, active - 10, then the
 * AttributeError; success = false (include/npb_maint.h, NPB_CA_AUTO_CONDENSER_TUBE_PLUGGING; tests/golden/auto_components/ac7_tube_leak).
 *
 * Values (end-of-step state, after the check's execution): tsp_fouling_fraction and steam_quality are carried fp64 members;
 * tube_wall_temperature (SteamGenerator.tube_wall_temp) and fouling_resistance (fouling_model.total_fouling_resistance) are OUTPUT
 * members the arena keeps as float: the scan compares the float (relative rounding 6e-8).  The condenser's resistance cannot be had
 * from carried members instead: the step computes it BEFORE it advances fouling_distribution_factor (npd_condenser.h), so the
 * end-of-step members give a value 1e-5 off.  tube_leak_rate is no member at all: npd_cond_tube_leak_rate below.  The fixtures keep every
 * scanned value 1e-5 away from its threshold.
 */
#ifndef NPD_COMPONENT_AUTO_H
#define NPD_COMPONENT_AUTO_H
#include "npd_maintenance.h"
#include "npd_component_maintenance.h"

struct npd_cmaint_consts_t { npb_component_maint_table_t T; };
/* the side state of one handle: [NPB_CMAINT_SIDE_DOUBLES][pitch] doubles behind the constants */
struct npd_cmaint_side_t { const npd_cmaint_consts_t *C; double *state; size_t pitch; };
#define NPD_CMS(side, member, slot, p) ((side).state[((size_t)(member) * NPB_CMAINT_NSLOT + (size_t)(slot)) * (side).pitch + (p)])

NPD_FN int npd_cmaint_rows(int c) { return c == NPB_CMAINT_COND ? 2 : 3; }
/* TubeDegradationModel.tube_leak_rate as the step left it (condenser/physics.py:114-131, npd_condenser.h), from the members the step leaves
 * behind: the failure rate from the damage accumulators and the chemistry's aggressiveness as they are after the step (the step uses them
 * after updating them), the tubes it failed from the active count BEFORE the step, which is active / (1 - f) while the counts add up to the
 * 84 000 tubes (f = the fraction failed, at most 1 %).  Not the reference's bits: the last ulps differ, the aggressiveness is a float-stored
 * output member, and a condenser handler carried out at this check has moved the counts by ten tubes (1e-4 of the value); the fixtures keep
 * the value 1e-5 away from its threshold. */
NPD_FN double npd_cond_tube_leak_rate(double vibration_damage, double corrosion_damage, double water_aggressiveness, double active_tube_count,
                                      double dt_hours) {
  double effective_failure_rate = (1e-06 * (1.0 + 10.0 * vibration_damage) * (1.0 + 5.0 * (corrosion_damage / 0.00159)) * (1.0 + water_aggressiveness));
  double f = npd_pymin(effective_failure_rate * dt_hours, 0.01);
  double tubes_failed = f * (active_tube_count / (1.0 - f));
  return npd_pymin(tubes_failed * 0.1, active_tube_count * 0.001) * 0.001;
}
NPD_FN int npd_cmaint_param0(int c) { return c == NPB_CMAINT_COND ? NPB_CP_COND_FOULING_RESISTANCE : NPB_CP_SG_TSP_FOULING_FRACTION; }

/* tube_bundle_overhaul's `encompasses`, as far as the generator's catalog has them (maintenance_orchestrator.py:552-555) */
static constexpr uint32_t NPD_CA_TUBE_BUNDLE_OVERHAUL_SET =
    (1u << NPB_CA_SG_TSP_CHEMICAL_CLEANING) | (1u << NPB_CA_SG_TSP_MECHANICAL_CLEANING) | (1u << NPB_CA_SG_SCALE_REMOVAL) |
    (1u << NPB_CA_SG_TUBE_INTERIOR_INSPECTION) | (1u << NPB_CA_SG_TUBE_INTERIOR_SCALE_CLEANING) |
    (1u << NPB_CA_SG_TUBE_INTERIOR_EDDY_CURRENT_TESTING) | (1u << NPB_CA_SG_TSP_INSPECTION);

/* which rows of component c are crossed outside their cooldown (bit r), from its values v[] and its stamps */
__device__ __forceinline__ uint32_t npd_cmaint_violations(const npd_cmaint_side_t &side, size_t p, int c, const double *v, double t) {
  const npb_component_maint_table_t &T = side.C->T;
  uint32_t viol = 0;
  for (int r = 0; r < npd_cmaint_rows(c); r++) {
    const int q = npd_cmaint_param0(c) + r;
    if (T.rank[q] < 0) continue;
    if (!npd_maint_violates(v[r], T.threshold[q], T.comparison[q])) continue;
    const double lv = NPD_CMS(side, NPB_CMS_LAST_VIOLATION_TIME, c * NPB_CMAINT_NROW + r, p);
    if (lv >= 0.0 && t - lv < T.cooldown_hours[q] * 60) continue;      /* _is_threshold_in_cooldown */
    viol |= 1u << r;
  }
  return viol;
}

/* one component's part of the scan and the work order it may create; returns the order's slot (its number is m->work_orders_created),
 * or -1.  *priority_out / *action_out describe the event */
__device__ __forceinline__ int npd_cmaint_scan(const npd_cmaint_side_t &side, size_t p, int c, uint32_t viol, npb_maint_t *m, const npb_params_t *P,
                                               double t, int *action_out, int *priority_out) {
  const npb_component_maint_table_t &T = side.C->T;
  const int q0 = npd_cmaint_param0(c), rows = npd_cmaint_rows(c);
  int first_rank = 1 << 30, requested = -1, priority = 0, in_overhaul = 0;
  for (int r = 0; r < rows; r++) {
    if (!((viol >> r) & 1u)) continue;
    const int q = q0 + r;
    NPD_CMS(side, NPB_CMS_LAST_VIOLATION_TIME, c * NPB_CMAINT_NROW + r, p) = t;
    if (T.rank[q] < first_rank) { first_rank = T.rank[q]; requested = T.action[q]; }
    if (T.priority[q] > priority) priority = T.priority[q];      /* the batched event's priority: the highest (state_manager.py:1602) */
    in_overhaul += (int)((NPD_CA_TUBE_BUNDLE_OVERHAUL_SET >> T.action[q]) & 1u);
  }
  if (c != NPB_CMAINT_COND && in_overhaul >= 3) return -1;      /* promoted to tube_bundle_overhaul, which is no action type: no order */
  if (!NPB_CMAINT_ACTION_IS_TYPE(requested)) return -1;
  int slot = -1;
  for (int r = rows - 1; r >= 0; r--)
    if (T.rank[q0 + r] >= 0 && T.action[q0 + r] == requested) slot = c * NPB_CMAINT_NROW + r;
  /* duplicate prevention (auto_maintenance.py:347-369): a number of hours compared with minutes, then an open order with this action */
  const double ltt = NPD_CMS(side, NPB_CMS_LAST_TRIGGER_TIME, slot, p);
  if (ltt >= 0.0 && t - ltt < P->maint_work_order_cooldown) return -1;
  if (NPD_CMS(side, NPB_CMS_WO_ORDER, slot, p) > 0.0) return -1;
  m->work_orders_created += 1;
  NPD_CMS(side, NPB_CMS_WO_ORDER, slot, p) = (double)m->work_orders_created;
  NPD_CMS(side, NPB_CMS_WO_CREATED, slot, p) = t;
  NPD_CMS(side, NPB_CMS_WO_PLANNED_START, slot, p) = npd_maint_start_time(P, t, priority);
  NPD_CMS(side, NPB_CMS_WO_PRIORITY, slot, p) = (double)priority;
  NPD_CMS(side, NPB_CMS_LAST_TRIGGER_TIME, slot, p) = t;
  *action_out = requested; *priority_out = priority;
  return slot;
}

/* the earliest-created due order among the components of plant p: its number (0 = none) and slot */
__device__ __forceinline__ double npd_cmaint_first_due(const npd_cmaint_side_t &side, size_t p, double t, int *slot_out) {
  double best = 0.0; int slot = -1;
  for (int s = 0; s < NPB_CMAINT_NSLOT; s++) {
    const double o = NPD_CMS(side, NPB_CMS_WO_ORDER, s, p), ps = NPD_CMS(side, NPB_CMS_WO_PLANNED_START, s, p);
    const bool due = o > 0.0 && ps != 0.0 && t >= ps;      /* `if work_order.planned_start_date and ...` (auto_maintenance.py:475) */
    if (due && (best == 0.0 || o < best)) { best = o; slot = s; }
  }
  *slot_out = slot;
  return best;
}

/* the side state of a freshly constructed plant */
__device__ __forceinline__ void npd_cmaint_init(double *state, size_t pitch, size_t p) {
  for (int k = 0; k < NPB_CMAINT_SIDE_DOUBLES; k++) {
    const int member = k / NPB_CMAINT_NSLOT;
    state[(size_t)k * pitch + p] = (member == NPB_CMS_LAST_VIOLATION_TIME || member == NPB_CMS_LAST_TRIGGER_TIME) ? -1.0 : 0.0;
  }
}

#endif
