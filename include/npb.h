/*
 * npb.h -- C ABI of the MI355X batched plant stepper (libnpb.so).
 *
 * This is the drop-in boundary for the per-timestep physics path of NuclearnAI/nuclear-sim:
 * the reference has no FFI (it is pure Python), so each entry point names the Python interface
 * it stands in for.  A maintainer of the reference binds these with ctypes;
 * this repo's own host mirror is nuclear_sim_amd/env.py.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative
 * NPB_E* code (text via npb_last_error); the caller owns every I/O buffer and passes raw DEVICE
 * pointers (e.g. torch.Tensor.data_ptr()); the library owns only the struct-of-arrays state arena
 * inside the handle; npb_step() allocates nothing and only enqueues work on `stream`
 * (a hipStream_t, NULL = default stream).  One handle per stream; distinct handles are independent.
 */
#ifndef NPB_H
#define NPB_H

#include <stddef.h>
#include <stdint.h>
#include "npb_fields.h"
#include "npb_params.h"
#include "npb_maint.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NPB_VERSION 154 /* 0.1.5.4: npb_set_maintenance_summary, npb_maint_summary_fold, npb_maint_summary_clear, npb_maint_summary_check (the maintenance event log folded into a per-plant work-order summary on the device); 0.1.5.3: npb_sampler_create, npb_sampler_sample, npb_sampler_destroy (a state log samples a watch list of plants, arena members and side buffers, in one launch); 0.1.5.2: npb_profile_seed, npb_profile_fill, npb_profile_ramp, npb_profile_get_state, npb_profile_set_state (the data-gen runner's power profile drawn on the device, per plant); 0.1.5.1: npb_carry_diagnostics, npb_diag_num_carried / npb_diag_carried_row / npb_diag_carried_fresh, npb_get / npb_set_diagnostics_state, npb_set_episode_index_buffer (the diagnostics rows the step carries travel with snapshots, start banks, the autoreset, resets and checkpoints; an episode index per plant); 0.1.5.0: npb_set_component_maintenance, npb_default_component_maintenance_table, npb_component_maint_* catalog queries, npb_get / npb_set_component_maintenance_state, NPB_MAINT_EVENT_COMPONENT_CREATED / _COMPLETED (automatic maintenance of steam generators and condenser in one work-order queue with the feedwater pumps); 0.1.4.9: npb_perform_turbine_maintenance, npb_turbine_* catalog queries, NPB_MAINT_EVENT_OPERATOR_TURBINE (maintenance of the turbine, its bearings, lubrication system and stages a caller orders); 0.1.4.8: npb_perform_component_maintenance, npb_component_* catalog queries, NPB_MAINT_EVENT_OPERATOR_COMPONENT (maintenance of steam generators, condenser and ejectors a caller orders); 0.1.4.7: npb_perform_maintenance, NPB_MAINT_EVENT_OPERATOR (maintenance a caller orders, carried out on the device between two steps); 0.1.4.6: npb_set_maintenance_log, npb_maint_event_bytes (work orders created and completed, logged on the device); 0.1.4.5: npb_noise_seed, npb_noise_fill, npb_noise_get_state, npb_noise_set_state (heat-source noise streams on the device); 0.1.4.4: npb_set_start_bank, npb_set_start_slots, npb_restore_bank, npb_set_episode_start_buffer (episodes restart from a bank of start states); 0.1.4.3: npb_snapshot, npb_restore, npb_set_autoreset, npb_set_episode_buffers (episodes: same-step autoreset, truncation); 0.1.4.2: NPB_DIAG_DIM 170 (state-log rows of round 4), npb_state_arena_layout, NPB_EINVAL for NPB_HEAT_EXTERNAL without its input column; 0.1.4.1: npb_state_arena_segment (segmented arenas), step-kernel variant 5, NPB_DIAG_DIM 136; 0.1.4: npb_debug_last_step_kernel, npb_info_dim / npb_obs_dim / npb_diag_dim, maintenance catalogs by index; 0.1.3.1: params.kinetics_rk4_substeps; 0.1.3: NPB_MODE_PRIMARY, reactivity components behind the info block (params.info_reactivity_components); 0.1.2: npb_reset_reference, maintenance table (npb_maint.h, mpump.* columns); 0.1.1: one arena of equally wide columns, npb_locate_field, npb_gather_fields, npb_create_storage */
#ifndef NPB_API
#define NPB_API __attribute__((visibility("default")))
#endif

enum { NPB_OK = 0, NPB_EINVAL = -1, NPB_EHIP = -2, NPB_ENOMEM = -3 };
enum { NPB_KIND_F64 = 0, NPB_KIND_I32 = 1 };
enum { NPB_OBS_DIM = 22, NPB_INFO_DIM = 17 };

/* info columns written by npb_step (the scalar keys of step()'s info dict, sim.py:199-250) */
enum {
  NPB_INFO_THERMAL_POWER = 0, NPB_INFO_REACTIVITY_PCM, NPB_INFO_ELECTRICAL_POWER, NPB_INFO_THERMAL_EFFICIENCY,
  NPB_INFO_STEAM_FLOW, NPB_INFO_STEAM_PRESSURE, NPB_INFO_CONDENSER_PRESSURE, NPB_INFO_CONDENSER_HEAT_REJECTION,
  NPB_INFO_TIME, NPB_INFO_FEEDWATER_FLOW,
  /* fp64 inputs of the reference's heat-flow bookkeeping and of the derived keys of its secondary result dict
   * (secondary/__init__.py:679-744, 922-1010; nuclear_sim_amd/env.py secondary_result): total steam-generator heat transfer
   * [W], turbine gross electrical power [MW], feedwater pump power [MW], primary thermal power over the three loops [MW] */
  NPB_INFO_SG_HEAT_TRANSFER, NPB_INFO_TURBINE_POWER, NPB_INFO_FEEDWATER_POWER, NPB_INFO_PRIMARY_THERMAL_POWER,
  /* the three keys of that dict that are left over from inside the turbine step (secondary/__init__.py:955-958): the stage
   * system's cycle efficiency (h_in - h_out) / h_in (stage_system.py:983-993) and the summed outputs of the HP-1..8 and
   * LP-1..6 stages [MW] (enhanced_physics.py:879-880); 0 where the turbine is not stepped (NPB_MODE_PRIMARY_SG) */
  NPB_INFO_TURBINE_EFFICIENCY, NPB_INFO_TURBINE_HP_POWER, NPB_INFO_TURBINE_LP_POWER
};
/* Step-internal diagnostics (optional: npb_set_diagnostics): what the reference's state log holds per turbine stage from inside
 * the expansion (TurbineStage.get_state_dict, stage_system.py:379-393) and nothing later in the step can recover -- fourteen
 * values each, HP-1..8 then LP-1..6, column (NPB_DIAG_* + stage) of a [NPB_DIAG_DIM][pitch] fp64 buffer -- and per steam generator. */
enum {
  NPB_DIAG_STAGE_INLET_PRESSURE = 0, NPB_DIAG_STAGE_INLET_TEMPERATURE = 14, NPB_DIAG_STAGE_OUTLET_PRESSURE = 28,
  NPB_DIAG_STAGE_OUTLET_TEMPERATURE = 42, NPB_DIAG_STAGE_POWER_OUTPUT = 56, NPB_DIAG_STAGE_LOADING_FACTOR = 70,
  /* per steam generator (SteamGenerator.get_state_dict, steam_generator.py:943-985), three values each, SG-0..2 */
  NPB_DIAG_SG_PRIMARY_INLET_TEMP = 84, NPB_DIAG_SG_PRIMARY_OUTLET_TEMP = 87, NPB_DIAG_SG_OVERALL_HTC = 90,
  NPB_DIAG_SG_FEEDWATER_FLOW_RATE = 93,
  /* per feedwater pump, FWP-1..4: the lubrication system's health factor as the step's wear update leaves it
   * (lubrication_base.py:398-399: mean component performance x lubrication effectiveness -- a maintenance action carried out
   * later in the same step does not refresh it), and the two maintenance flags of the pump's state dict
   * (pump_lubrication.py:1636-1641: an action / an oil top-off was carried out on this pump in this step) */
  NPB_DIAG_PUMP_HEALTH_FACTOR = 96, NPB_DIAG_PUMP_MAINTENANCE_OCCURRED = 100, NPB_DIAG_PUMP_OIL_TOP_OFF_OCCURRED = 104,
  /* the steam-generator conditions the feedwater system was given this step -- the copies of the step before, the hard-coded
   * ones at the first step (secondary/__init__.py:447-453) -- as its state dict averages them (feedwater/physics.py:1140-1145) */
  NPB_DIAG_FW_AVG_SG_LEVEL = 108, NPB_DIAG_FW_AVG_SG_PRESSURE = 109, NPB_DIAG_FW_TOTAL_STEAM_FLOW = 110, NPB_DIAG_FW_AVG_STEAM_QUALITY = 111,
  /* the rotor model's torque balance of this step (rotor_dynamics.py:855-911): bearing friction torque [N m] from the bearing loads
   * the step began with, net torque, acceleration [RPM/s] */
  NPB_DIAG_ROTOR_FRICTION_TORQUE = 112, NPB_DIAG_ROTOR_NET_TORQUE = 113, NPB_DIAG_ROTOR_ACCELERATION = 114,
  /* the condenser's step (condenser/physics.py:564-728, 73-145; vacuum_pump.py:96-190): overall heat-transfer coefficient, tube
   * leak rate, the first ejector's motive steam flow and steam consumption rate, the vacuum system's total motive steam */
  NPB_DIAG_COND_OVERALL_HTC = 115, NPB_DIAG_COND_TUBE_LEAK_RATE = 116, NPB_DIAG_COND_SJE1_STEAM_FLOW = 117,
  NPB_DIAG_COND_SJE1_STEAM_CONSUMPTION = 118, NPB_DIAG_COND_VACUUM_STEAM_CONSUMPTION = 119,
  /* per steam generator: the tube-scale formation rate of the step [mm / year] (tube_interior_fouling.py:117-188) */
  NPB_DIAG_SG_SCALE_FORMATION_RATE = 120,
  /* the feedwater system's performance factor (feedwater/physics.py:800-805: mean flow x efficiency factor of the running pumps x
   * water-quality factor, from the shared chemistry between its two updates of the step, x the diagnostics' health score) */
  NPB_DIAG_FW_PERFORMANCE_FACTOR = 123,
  /* accumulators of the rotor model that no physics reads, summed in the caller's buffer from the step the diagnostics were
   * switched on (zero the buffer at construction and they are the reference's): the four bearings' clearance increase [mm]
   * (rotor_dynamics.py:298-300) and the overspeed event count (:900-902) */
  NPB_DIAG_ROTOR_CLEARANCE_INCREASE = 124, NPB_DIAG_ROTOR_OVERSPEED_EVENTS = 128,
  /* the oil temperature the lubrication system hands each turbine bearing, TB-001..004 (turbine_bearing_lubrication.py:967-1072) */
  NPB_DIAG_BEARING_OIL_TEMP = 129,
  /* the stage system's efficiency factor -- a product carried from step to step in the caller's buffer like the accumulators above
   * (a row of zeros reads as 1.0) -- and the turbine's performance factor built on it (stage_system.py:981, enhanced_physics.py:823-828) */
  NPB_DIAG_STAGE_SYSTEM_EFFICIENCY = 133, NPB_DIAG_TURBINE_PERFORMANCE_FACTOR = 134,
  /* number of alarms the feedwater protection system holds after the step (protection_system.py:399-445) */
  NPB_DIAG_FW_ACTIVE_ALARMS = 135,
  /* round 4: what the state log's remaining columns need from inside the step.
   * per feedwater pump, FWP-1..4: the maintenance action carried out on the pump in this step as catalog index + 1 (0 = none;
   * include/npb_maint.h), from which the thirteen <action>_occurred flags of the pump's state dict follow
   * (pump_lubrication.py:642-643, 1636-1641); written by the maintenance rule like NPB_DIAG_PUMP_MAINTENANCE_OCCURRED */
  NPB_DIAG_PUMP_MAINTENANCE_ACTION = 136,
  /* the feedwater protection system's bookkeeping (protection_system.py:447-476, 680-716): trips standing after the step;
   * carried in the caller's buffer from the step diagnostics were switched on: steps on which a trip came up
   * (valid_trip_count), emergency feedwater / steam dump set by such a step's trips and never cleared by the step */
  NPB_DIAG_FW_ACTIVE_TRIPS = 140, NPB_DIAG_FW_VALID_TRIP_COUNT = 141, NPB_DIAG_FW_EMERGENCY_FEEDWATER = 142, NPB_DIAG_FW_STEAM_DUMP = 143,
  /* per turbine stage: the extraction flow the stage took [kg/s] (stage_system.py:186-203) */
  NPB_DIAG_STAGE_EXTRACTION_FLOW = 144,
  /* per steam-jet ejector, SJE-001..002 (vacuum_pump.py:470-536): air-removal capacity, motive steam flow, steam consumption
   * rate of the step; and carried in the caller's buffer: the compression ratio (kept from the ejector's last operating step;
   * the row starts at 1.0) and the hours it has operated; then the vacuum system's total air removal (vacuum_system.py:499) */
  NPB_DIAG_COND_SJE_CAPACITY = 158, NPB_DIAG_COND_SJE_STEAM_FLOW = 160, NPB_DIAG_COND_SJE_STEAM_CONSUMPTION = 162,
  NPB_DIAG_COND_SJE_COMPRESSION_RATIO = 164, NPB_DIAG_COND_SJE_OPERATING_HOURS = 166, NPB_DIAG_COND_AIR_REMOVAL = 168,
  /* the stage system's total power [MW] as its state dict holds it (stage_system.py:976): stability-adjusted, before the turbine's
   * protection and availability factors */
  NPB_DIAG_STAGE_SYSTEM_TOTAL_POWER = 169,
  NPB_DIAG_DIM = 170
};
/* The rows above that the step CARRIES in the caller's buffer from one step to the next -- accumulators, latches, values kept while
 * equipment rests: plant state that lives beside the arena -- stated once: X(row, value of a freshly constructed plant), in the order
 * npb_get_diagnostics_state / npb_set_diagnostics_state move them.  npb_diag_num_carried / _carried_row / _carried_fresh read it. */
#define NPB_DIAG_CARRIED(X) \
  X(NPB_DIAG_ROTOR_CLEARANCE_INCREASE + 0, 0.0) X(NPB_DIAG_ROTOR_CLEARANCE_INCREASE + 1, 0.0) X(NPB_DIAG_ROTOR_CLEARANCE_INCREASE + 2, 0.0) \
  X(NPB_DIAG_ROTOR_CLEARANCE_INCREASE + 3, 0.0) X(NPB_DIAG_ROTOR_OVERSPEED_EVENTS, 0.0) \
  X(NPB_DIAG_STAGE_SYSTEM_EFFICIENCY, 0.0)      /* a zero reads as 1.0 (above) */ \
  X(NPB_DIAG_FW_VALID_TRIP_COUNT, 0.0) X(NPB_DIAG_FW_EMERGENCY_FEEDWATER, 0.0) X(NPB_DIAG_FW_STEAM_DUMP, 0.0) \
  X(NPB_DIAG_COND_SJE_COMPRESSION_RATIO + 0, 1.0) X(NPB_DIAG_COND_SJE_COMPRESSION_RATIO + 1, 1.0) \
  X(NPB_DIAG_COND_SJE_OPERATING_HOURS + 0, 0.0) X(NPB_DIAG_COND_SJE_OPERATING_HOURS + 1, 0.0)
enum { NPB_DIAG_NUM_CARRIED = 13 };
/* info["reactivity_components"] (sim.py:205; reactivity_model.py:77-125, pcm, the dict's insertion order).  Only the
 * reactor heat source has them, and only a caller that sets params.info_reactivity_components gets them: the info
 * buffer handed to npb_step must then hold a second block behind the first, [n_plants][NPB_INFO_DIM] followed by
 * [n_plants][NPB_INFO_NRHO]. */
enum {
  NPB_RHO_CONTROL_RODS = 0, NPB_RHO_BORON, NPB_RHO_DOPPLER, NPB_RHO_MODERATOR_TEMP, NPB_RHO_MODERATOR_VOID, NPB_RHO_PRESSURE,
  NPB_RHO_XENON, NPB_RHO_SAMARIUM, NPB_RHO_FUEL_DEPLETION, NPB_RHO_BURNABLE_POISONS, NPB_INFO_NRHO
};
/* trip_flags bits */
enum {
  NPB_TRIP_SCRAM = 1u << 0,        /* ReactorState.scram_status latched (scram_logic.py:57) */
  NPB_TRIP_SCRAM_FIRED = 1u << 1,  /* scram fired on this step == step()['done'] (sim.py:256) */
  NPB_TRIP_NAN_RESET = 1u << 2,    /* NaN reset taken (thermal_hydraulics.py:247-270) */
  NPB_TRIP_TURBINE = 1u << 3,      /* TurbineProtectionSystem.trip_active */
  NPB_TRIP_FW_SYSTEM = 1u << 4,    /* FeedwaterProtectionSystem.system_trip_active */
  NPB_TRIP_FW_PUMP0 = 1u << 8      /* bits 8..11: feedwater pump i trip_active */
};

typedef struct NpbHandle NpbHandle;

NPB_API int npb_version(void);
/* schema sizes (must equal NPB_TOTAL_F64 / NPB_TOTAL_I32 the caller was compiled against) */
NPB_API int npb_num_f64(void);
NPB_API int npb_num_i32(void);
/* widths of the row-major output blocks of npb_step the library was built with (NPB_OBS_DIM / NPB_INFO_DIM / NPB_INFO_NRHO /
 * NPB_DIAG_DIM).  A binding that allocates those buffers checks them at load: a caller sized for fewer info columns than the
 * library writes would be overrun (the round-2 host crash). */
NPB_API int npb_obs_dim(void);
NPB_API int npb_info_dim(void);
NPB_API int npb_info_nrho(void);
NPB_API int npb_diag_dim(void);
/* the catalogs of include/npb_maint.h by index (NULL past the end): threshold parameter names as the state log spells them,
 * MaintenanceActionType values */
NPB_API int npb_maint_num_params(void);
NPB_API int npb_maint_num_actions(void);
NPB_API const char *npb_maint_param_name(int k);
NPB_API const char *npb_maint_action_name(int a);
NPB_API int npb_maint_action_has_handler(int a);
/* arena bytes per plant (fp64 storage): 8 * (carried fp64 members + ceil(narrow members / 2) per section instance) */
NPB_API size_t npb_state_bytes(void);
/* algorithmic HBM bytes of one plant-step: carried fp64 members read and written (16 B), int32 members read and
 * written (8 B), output members written as float (4 B) -- all but the maint.* section, which only the
 * maintenance kernel touches -- + per-step inputs (action 4 + magnitude/setpoint/noise/cooling 4*8) + outputs
 * (obs 22*8 + reward 8 + done 1 + trip_flags 4 + info 17*8) */
NPB_API size_t npb_step_bytes_per_plant(void);
/* the same for one handle: with fp32 storage every carried real moves 4 bytes instead of 8, and under
 * ConstantHeatSource the 12 point-kinetics columns of the primary section are not touched at all */
NPB_API size_t npb_handle_step_bytes_per_plant(const NpbHandle *h);

NPB_API void npb_default_params(npb_params_t *p);

/* NuclearPlantSimulator.__init__ (sim.py:30-87) for n_plants plants on HIP device `device`:
 * allocates the SoA arena and fills it with the construction-time state.  One handle carries at most
 * 4 GiB of fp64 state (about one million plants: the step kernel's column offsets are 32-bit);
 * larger batches use several handles (they are independent).  When the bytes a step touches are about the size of the
 * 256 MB Infinity Cache (200-340 MB: 65 536 fp64 plants), where the arena lands in physical memory decides between 0.097
 * and 0.110 ms per step; creation then times the step kernel on up to four candidate arenas and keeps the fastest
 * (~15 ms; the arena ends in the construction-time state all the same; environment NPB_PLACEMENT_PROBE=0 turns it off). */
NPB_API int npb_create(const npb_params_t *params, int n_plants, int device, NpbHandle **out);
/* The same with the element type of the real-valued state columns chosen (BASELINE config 5, "fp32-mixed"):
 * NPB_STORAGE_F32 keeps the carried state as float in HBM and in the LDS staging -- half the traffic of
 * the HBM-bound step kernel -- while every expression is still evaluated in fp64 exactly as in the fp64
 * build; values are rounded to float once per step, when they are stored.  Flags, counters and enums are
 * int32 columns either way and stay bit-exact as long as no rounded value sits within 1e-7 relative of a
 * trip threshold.  Inputs, observations, rewards and info stay fp64; npb_get_field / npb_set_field convert.
 * The reference has no counterpart (it is fp64 throughout); parity for this mode is 1e-4 relative on
 * observations (tests/test_gpu_parity.py). */
enum { NPB_STORAGE_F64 = 0, NPB_STORAGE_F32 = 1 };
NPB_API int npb_create_storage(const npb_params_t *params, int n_plants, int device, int storage, NpbHandle **out);
NPB_API int npb_storage(const NpbHandle *h);
NPB_API int npb_destroy(NpbHandle *h);
NPB_API const char *npb_last_error(const NpbHandle *h); /* h may be NULL: last create error */
NPB_API int npb_num_plants(const NpbHandle *h);
NPB_API int npb_set_params(NpbHandle *h, const npb_params_t *params);
/* thresholds of the automatic maintenance of the feedwater pumps (include/npb_maint.h): what the reference reads from
 * the maintenance_system section of its configuration into StateManager.maintenance_thresholds.  A new handle carries
 * npb_maint_table_default() (the data-gen action-test configuration), whose oil_level row follows the two parameters of ABI
 * version 1 (params.maint_oil_level_threshold / _cooldown_hours); a table set here is taken exactly as given. */
NPB_API int npb_set_maintenance_table(NpbHandle *h, const npb_maint_table_t *table);
NPB_API void npb_default_maintenance_table(npb_maint_table_t *table);
/* AutoMaintenanceSystem.maintenance_actions_performed of every plant as a column the caller owns (device, int32[n_plants]; NULL =
 * none): with params.maint_enabled every npb_step leaves it current -- filled whole after any call that may have changed state,
 * then kept by the maintenance rule kernel for the plants whose count it moves -- so a loop that wants the event counts after
 * each step (the data-gen runner does, maintenance_scenario_runner.py:392-411) needs no npb_get_field launch per step. */
NPB_API int npb_set_maintenance_count_buffer(NpbHandle *h, int32_t *counts);
/* The maintenance event log: every work order the automatic maintenance creates or completes, as an npb_maint_event_t record
 * (include/npb_maint.h: time, creation time, planned start, plant, order number n = the reference's WO-%06d, pump, action,
 * kind, priority, bearing, trigger mask) -- what the reference keeps in WorkOrderManager.work_orders / completed_work_orders and
 * the data-gen runner exports as *_work_orders.csv / *_maintenance_actions.csv.  records (device, capacity records, 8-byte aligned:
 * each record is stored whole and holds doubles) and cursor (device, one uint32, 4-byte aligned) are the caller's; records = NULL (capacity 0) turns the log off.  Every step with params.maint_enabled
 * appends: each event adds 1 to *cursor (atomically, so the records of one step arrive in no particular order) and is written to
 * records[slot] only while slot < capacity; a cursor past the capacity counts the events that were dropped.  The caller drains
 * the log on its stream: read the cursor, copy min(cursor, capacity) records, zero the cursor.  The log is output only: not plant
 * state, and npb_snapshot / npb_restore / the autoreset / the start bank neither read nor reset it.  NPB_EINVAL for a negative
 * capacity, records without a cursor, a capacity without records, or misaligned buffers. */
NPB_API int npb_set_maintenance_log(NpbHandle *h, void *records, int capacity, uint32_t *cursor);
NPB_API size_t npb_maint_event_bytes(void);   /* sizeof(npb_maint_event_t) */
/* The per-plant work-order summary: the maintenance event log folded into first-created / first-completed times and created / completed
 * counts per (key, plant) (include/npb_maint.h npb_maint_summary_desc_t: the keys, the caller's four tables, since_minutes).  A table of that
 * size never overflows and never needs draining; it stays on the device beside obs and info.  Needs a maintenance log
 * (npb_set_maintenance_log): a fold reads the records [*folded, min(*cursor, capacity)) and updates the tables, in one launch of a fixed
 * grid that takes its range from the device words; the host never learns the cursor and nothing synchronises.  With a summary set,
 * npb_step folds behind its rule kernel(s) and each of npb_perform_maintenance / _component_maintenance / _turbine_maintenance behind its
 * kernel, so the summary is current after every call that can append records; npb_maint_summary_fold folds explicitly.
 * The two device words `folded` and `dropped` (uint32, the caller's, zero to begin with) are the summary's bookkeeping:
 *   keep mode (consume = 0): the log stays the caller's to drain.  After a fold *folded = min(*cursor, capacity) and *dropped =
 *     max(*cursor - capacity, 0).  A caller that zeroes the cursor zeroes *folded with it.
 *   consume mode (consume = 1): the log is only a staging ring of the summary.  After a fold *dropped += max(*cursor - capacity, 0),
 *     *cursor = 0 and *folded = 0: the log never fills up over a long run.  It needs capacity >= n_plants -- a capacity the events of
 *     one call can exceed whenever every plant has one would lose events silently as a matter of course; what is lost beyond that is
 *     counted in *dropped, never hidden.
 * The cursor is rewritten by the last block to finish (one atomic ticket), after every record of the fold has been read; no block waits
 * for another.  The fold must run on the stream the appending calls run on.
 * The summary is output only, like the log: npb_snapshot / npb_restore, the autoreset and the start bank neither read nor reset it; a
 * caller who wants per-episode summaries clears the plants it restarted (npb_maint_summary_clear).  desc = NULL turns it off, and so does
 * turning the log off; a handle without a summary behaves exactly as before.
 * NPB_EINVAL, with the reason in npb_last_error, for: no maintenance log set; n_keys outside 1..NPB_MAINT_SUMMARY_MAX_KEYS; a catalog,
 * action or unit outside its catalog; a `kinds` without a kind of the key's catalog; a NULL or misaligned table or word; consume with a
 * log capacity below n_plants.  npb_maint_summary_check is that check alone, without a handle: NULL = accepted, else the reason
 * (log_capacity < 0 = no log set). */
NPB_API int npb_set_maintenance_summary(NpbHandle *h, const npb_maint_summary_desc_t *desc);
NPB_API const char *npb_maint_summary_check(const npb_maint_summary_desc_t *desc, int log_capacity, int n_plants);
NPB_API int npb_maint_summary_fold(NpbHandle *h, void *stream);
/* the rows of the plants of mask (device uint8[n_plants]; NULL = all) back to +inf and 0, for every key; asynchronous on `stream`.
 * NPB_EINVAL without a summary. */
NPB_API int npb_maint_summary_clear(NpbHandle *h, const uint8_t *mask, void *stream);
/* Operator-ordered maintenance: FeedwaterPump.perform_maintenance(maintenance_type, **kwargs) (feedwater/pump_system.py:750), i.e. the
 * lubrication system's dispatcher (feedwater/pump_lubrication.py:625-674), called by the USER between two steps: for every plant p
 * with action[p] >= 0, what that call does to pump pump[p] (0..3 = FWP-1..4) of the plant, at once -- no work order, no delay.  All
 * pointers are device pointers to n_plants elements; asynchronous on `stream`.
 *   action        NPB_MA_* index (npb_maint_action_name), -1 = nothing for this plant
 *   bearing       NULL = NPB_BEARING_ALL: the component_id kwarg of _perform_bearing_replacement (:755-808), NPB_BEARING_*
 *   target_level  NULL = 95.0, the default ARGUMENT of _perform_oil_top_off (:710) -- not params.maint_top_off_target, which is what the
 *                 automatic maintenance passes; the other handlers ignore both columns, as the reference's **kwargs do
 *   success       may be NULL; 1 where the reference's result dict has 'success': True -- the dispatcher has a handler for the action
 *                 (npb_maint_action_has_handler) and a bearing replacement names a valid bearing -- else 0, plants with action -1 included.
 *                 An action outside the catalog, a pump outside 0..3, a bearing_replacement with a bearing outside 0..3 are the reference's
 *                 "Unknown maintenance type" / "Invalid bearing component": success 0, state untouched, no error code (the columns are on
 *                 the device and the call does not synchronise).
 * Only the pump section of the ordered pump changes, and a plant without a successful order keeps its exact bits.  The work-order queue,
 * the maint.* / mpump.* columns, the count buffer (npb_set_maintenance_count_buffer) and the diagnostics rows do not move: a direct call
 * bypasses AutoMaintenanceSystem in the reference too.  Works with params.maint_enabled 0 or 1, in every mode and storage type.  With a
 * maintenance log set (npb_set_maintenance_log) every successful order appends one NPB_MAINT_EVENT_OPERATOR record.  Not offered: work
 * orders created by the operator (queued, delayed, counted).  Steam generators and condenser: npb_perform_component_maintenance; the
 * turbine: npb_perform_turbine_maintenance.
 * NPB_EINVAL for action = NULL or pump = NULL. */
NPB_API int npb_perform_maintenance(NpbHandle *h, const int32_t *action, const int32_t *pump, const int32_t *bearing,
                                    const double *target_level, uint8_t *success, void *stream);
/* The same for the other components whose direct-call handlers act on carried state: perform_maintenance(maintenance_type, **kwargs) of a
 * steam generator (steam_generator/steam_generator.py:1092-1326), the steam-generator system (steam_generator/enhanced_physics.py
 * :1062-1191), the condenser (condenser/physics.py:1188-1372, the definition the class ends up with) and a steam-jet ejector
 * (condenser/vacuum_pump.py:338-468), called by the USER between two steps.  Device pointers to n_plants elements; asynchronous.
 *   action   index of the COMPONENT catalog (NPB_CA_*, include/npb_maint.h; npb_component_action_name / _kind), -1 = nothing for this
 *            plant.  The index names the component kind, so one column may mix kinds.
 *   unit     NULL = 0: the generator 0..2 or the ejector 0..1 (SJE-001, SJE-002); ignored by system and condenser actions.  A call the
 *            reference's system delegates (kwarg sg_index) is the generator's action on unit sg_index.
 *   option   NULL = NPB_CLEANING_DEFAULT: the cleaning_type kwarg as NPB_CLEANING_*, read by the scale cleanings, condenser_tube_cleaning
 *            and vacuum_ejector_cleaning (each with its own set of named types; any other value is the handler's "else" branch)
 *   amount   NULL = 10: the tubes_to_plug kwarg.  Carried for condenser_tube_plugging, which is NOT in the catalog (the reference's
 *            handler raises); no catalogued handler reads it.
 *   success  may be NULL; 1 where the reference's result says success -- every catalogued action on a unit that exists -- else 0, plants
 *            with action -1 included.  An index outside the catalog or a unit that does not exist: success 0, state untouched, no error
 *            code.  In a mode that does not step a component (NPB_MODE_PRIMARY: none of them, the reference then has no secondary_physics
 *            to call; NPB_MODE_PRIMARY_SG: condenser and ejectors) its actions give success 0.
 * Only the sections the action touches change -- one sg instance; all three for the system's actions, or sec for its coordination; cond,
 * with chem[1] for condenser_water_treatment -- and a plant without a successful order keeps its exact bits.  water_chemistry_adjustment
 * resets the steam-generator system's own chemistry, which is not carried (npb_params.h sgchem_*): success 1, nothing moves.  The
 * work-order queue, maint.* / mpump.*, the count buffer and the diagnostics rows do not move; params.maint_enabled may be 0 or 1.  With
 * a maintenance log set every successful order appends one NPB_MAINT_EVENT_OPERATOR_COMPONENT record (action = catalog index, pump byte =
 * unit).  Not offered: work orders for these components.  The turbine: npb_perform_turbine_maintenance.
 * NPB_EINVAL for action = NULL. */
NPB_API int npb_perform_component_maintenance(NpbHandle *h, const int32_t *action, const int32_t *unit, const int32_t *option,
                                              const double *amount, uint8_t *success, void *stream);
/* the COMPONENT catalog by index: type string, component kind (NPB_COMPONENT_*; -1 outside the catalog), and per kind its name */
NPB_API int npb_component_num_actions(void);
NPB_API const char *npb_component_action_name(int a);
NPB_API int npb_component_action_kind(int a);
NPB_API const char *npb_component_kind_name(int kind);
/* The same for the turbine: perform_maintenance(maintenance_type) of the turbine (turbine/enhanced_physics.py:1055-1267), one of its four
 * bearings (turbine/rotor_dynamics.py:381-564), its bearing-lubrication system (turbine/turbine_bearing_lubrication.py:481-668) and one
 * of its fourteen stages (turbine/stage_system.py:341-377), called by the USER between two steps.  Device pointers to n_plants elements;
 * asynchronous.
 *   action   index of the TURBINE catalog (NPB_TA_*, include/npb_maint.h; npb_turbine_action_name / _kind), -1 = nothing for this plant.
 *            The index names the kind, so one column may mix kinds.  The catalog holds the handlers the live reference shows closed over
 *            the carried state; a stage's "cleaning" is not among them (include/npb_maint.h).
 *   unit     NULL = 0: the bearing 0..3 (TB-001..TB-004; the third is the thrust bearing) or the stage 0..13 (HP-1..HP-8, LP-1..LP-6);
 *            ignored by actions on the turbine and the lubrication system
 *   success  may be NULL; 1 where the reference's result says success -- a catalogued action on a unit that exists, and for
 *            thrust_bearing_adjustment the thrust bearing -- else 0, plants with action -1 included.  A stage's handler returns no
 *            success flag: 1 for its catalogued types.  An index outside the catalog or a unit that does not exist: success 0, state
 *            untouched, no error code.  In a mode that does not step the turbine (NPB_MODE_PRIMARY, NPB_MODE_PRIMARY_SG) every order
 *            gives success 0.
 * An order on the turbine, a bearing or the lubrication system changes members of turb only; an order on a stage changes that stage's
 * stage_deposit_thickness / stage_blade_wear_factor / stage_efficiency_degradation only; a plant without a successful order keeps its
 * exact bits.  Several catalogued handlers move no carried member (tests, inspections, analyses): success 1, nothing stored.  The
 * work-order queue, maint.* / mpump.*, the count buffer and the diagnostics rows do not move -- the accumulator rows of the diagnostics
 * buffer (the bearings' clearance increase, the stage system's efficiency) therefore do not follow an operator action.  With a
 * maintenance log set every successful order appends one NPB_MAINT_EVENT_OPERATOR_TURBINE record (action = catalog index, pump byte =
 * unit).  Not offered: work orders and automatic maintenance for the turbine.
 * NPB_EINVAL for action = NULL. */
NPB_API int npb_perform_turbine_maintenance(NpbHandle *h, const int32_t *action, const int32_t *unit, uint8_t *success, void *stream);
/* the TURBINE catalog by index: type string, turbine kind (NPB_TURBINE_*; -1 outside the catalog), and per kind its name */
NPB_API int npb_turbine_num_actions(void);
NPB_API const char *npb_turbine_action_name(int a);
NPB_API int npb_turbine_action_kind(int a);
NPB_API const char *npb_turbine_kind_name(int kind);
/* Automatic maintenance of the three steam generators and the condenser, in ONE work-order queue with the feedwater pumps, as the
 * reference's AutoMaintenanceSystem runs them (nuclear_sim_amd/csrc/npd_component_auto.h): after every step the scan goes over FWP-1..4,
 * SG-0..2 and the condenser in that order, every order created is numbered from the one counter maint.work_orders_created, and a due
 * check carries out ONE due order, the earliest created of any component -- so switching this on also changes WHEN a pump's order is
 * carried out.  table = the rows (include/npb_maint.h npb_component_maint_table_t; npb_default_component_maintenance_table = the
 * data-gen composer's), NULL switches the feature off; off is the default and leaves every result as it was.  Needs
 * params.maint_enabled and NPB_MODE_FULL (npb_step says so by name otherwise).  While it is on, npb_step launches the step kernel of a
 * handle WITHOUT automatic maintenance and then one rule kernel for pumps and components together (npb_maint_all_kernel).
 * The per-plant state of the rule -- a last-violation stamp per (component, row); per (component, action) the open order's number,
 * creation time, planned start, priority and the last trigger -- lives in a side buffer the handle owns, NOT in the arena:
 * NPB_CMAINT_SIDE_DOUBLES doubles per plant (include/npb_maint.h).  It is allocated, as a freshly built plant's, when the feature is
 * first switched on, and treated as the mpump section is: npb_reset clears it (masked: the masked plants'), npb_reset_reference leaves it
 * alone, npb_snapshot records it, npb_restore / the autoreset / npb_restore_bank put it back with the plant (a snapshot or bank recorded
 * without the feature is refused by name, and so is a bank handle that has not got it on).  A checkpoint that saves the arena must save it
 * too: npb_get_component_maintenance_state / npb_set_component_maintenance_state copy it to / from a buffer (host or device) of
 * npb_component_maintenance_state_bytes(h) bytes, member-major: member m of plant p at [m * n_plants + p]; both synchronise the stream.
 * The call synchronises the device before it uploads the table.  The side state is keyed by ROW (an open order and its trigger stamp
 * are filed under the first row of their component that names the action): a second call with another table while orders are open keeps
 * them attached to their rows, so an open order is then carried out with the action its row names in the NEW table, and a row that
 * changed its action inherits the old action's trigger stamp.  Change a table between episodes (after npb_reset), or with no order open
 * (wo_order all zero in the side state).
 * With a maintenance log set the rule appends NPB_MAINT_EVENT_COMPONENT_CREATED / _COMPONENT_COMPLETED records beside the pumps'.
 * NPB_EINVAL for a row whose comparison / priority is out of range or whose action is not a COMPONENT catalog entry of the row's kind. */
NPB_API int npb_set_component_maintenance(NpbHandle *h, const npb_component_maint_table_t *table);
NPB_API void npb_default_component_maintenance_table(npb_component_maint_table_t *table);
NPB_API int npb_component_maint_num_params(void);
NPB_API const char *npb_component_maint_param_name(int k);
NPB_API int npb_component_maint_param_kind(int k);      /* NPB_COMPONENT_SG | NPB_COMPONENT_COND */
NPB_API size_t npb_component_maintenance_state_bytes(const NpbHandle *h);
NPB_API int npb_get_component_maintenance_state(NpbHandle *h, double *buf, void *stream);
NPB_API int npb_set_component_maintenance_state(NpbHandle *h, const double *buf, void *stream);

/* re-initialise plants to the construction-time state; mask (device, uint8[n], NULL = all) selects plants.
 * Stands in for constructing a fresh simulator (the data-gen runner's episode start,
 * maintenance_scenario_runner.py:210-244). */
NPB_API int npb_reset(NpbHandle *h, const uint8_t *mask, void *stream);
/* NuclearPlantSimulator.reset(start_at_steady_state)  sim.py:546-581 with the reference's own semantics: each
 * subsystem's reset() puts part of its state back to literals, re-applies initial conditions for another part and
 * leaves the rest (lubrication systems, metal temperatures, pH controller, tube scale, the previous step's SG
 * conditions) as the history left it; start_at_steady_state != 0 additionally runs initialize_to_steady_state
 * (secondary/__init__.py:1074-1357: one steam-generator update as a side effect, every pump force-set).
 * mask as for npb_reset.  Follow with npb_observe for reset()'s return value. */
NPB_API int npb_reset_reference(NpbHandle *h, const uint8_t *mask, int start_at_steady_state, void *stream);

/* state columns: sim.state.<attr> / component attribute access.  `slot` is the global slot of
 * npb_fields.h; buf holds n_plants elements (double or int32_t) on the device or the host. */
NPB_API int npb_get_field(NpbHandle *h, int kind, int slot, void *buf, int buf_is_device, void *stream);
NPB_API int npb_set_field(NpbHandle *h, int kind, int slot, const void *buf, int buf_is_device, void *stream);
/* Many fields in one launch, every value widened to double: out (device) = [n_fields][n_plants].  This is the sampling
 * step of a columnar state log -- the batched counterpart of StateManager.collect_states (state_manager.py:152-213),
 * which walks every provider's get_state_dict() and appends one pandas row per step.  kinds / slots are host arrays;
 * the request is remembered, so repeating it costs one kernel launch. */
NPB_API int npb_gather_fields(NpbHandle *h, int n_fields, const int *kinds, const int *slots, double *out, void *stream);
/* A SAMPLER: the sampling step of a state log that follows a watch list of plants while the whole batch runs.  Created once from a
 * request, used once per sample: npb_sampler_sample is ONE kernel launch on `stream` that writes, widened to double, row r of watched
 * plant j to out[r * n_watched + j] (device, [rows][n_watched]) -- first the n_fields arena members (kinds / slots as npb_gather_fields
 * takes them), then the rows of every side source in request order.  A side source is a caller-owned DEVICE buffer that holds per-plant
 * values beside the arena (the diagnostics buffer, the step's info block, done, the episode columns): row q of plant p is element
 * base[q * row_stride + p * plant_stride] of the given type, strides in elements.  The caller keeps these buffers alive and in place
 * while the sampler exists.  The plant ids (host int32[n_watched]) keep the caller's order: consecutive ids make consecutive lanes,
 * which coalesce; every id of a scattered list costs a cache line per row.
 * npb_sampler_create validates the whole request before any device work and refuses by name (npb_last_error): n_watched <= 0, an id
 * outside [0, n_plants), a duplicate id, a bad kind or slot, a side source with a NULL base, an unknown type or rows <= 0, a request
 * without rows.  It uploads plan and ids once (synchronously); npb_sampler_sample uploads nothing and does not synchronise.  Samplers
 * share nothing with npb_gather_fields' remembered request or with one another.  *sampler = an id >= 0 of this handle.
 * npb_sampler_destroy frees one (a pending npb_sampler_sample on `stream`s the caller has not synchronised must have finished);
 * npb_destroy frees the rest.  An unknown or destroyed id is NPB_EINVAL. */
enum { NPB_SAMPLE_F64 = 0, NPB_SAMPLE_F32 = 1, NPB_SAMPLE_I32 = 2, NPB_SAMPLE_U8 = 3 };
typedef struct { const void *base; int type; int rows; int64_t row_stride, plant_stride; } npb_sample_source_t;
typedef struct {
  int n_watched; const int32_t *plants;                 /* host */
  int n_fields; const int *kinds; const int *slots;     /* host; n_fields may be 0 */
  int n_sources; const npb_sample_source_t *sources;    /* host array of descriptors of device buffers; n_sources may be 0 */
} npb_sampler_desc_t;
NPB_API int npb_sampler_create(NpbHandle *h, const npb_sampler_desc_t *desc, int *sampler);
NPB_API int npb_sampler_sample(NpbHandle *h, int sampler, double *out, void *stream);
NPB_API int npb_sampler_destroy(NpbHandle *h, int sampler);
/* raw arena (checkpointing, external kernels): one allocation of equally wide columns, column-major with `pitch`
 * plants per column; the members of the schema are mapped onto columns as include/npb_fields.h describes.  A handle of
 * more than 45 056 plants keeps its arena in SEGMENTS (npb_state_arena_segment(h) plants each -- 16 384 --, 0 = not
 * segmented): the allocation is then consecutive [columns][pitch] blocks, pitch = the segment size, block s holding
 * plants s * pitch .. (s + 1) * pitch - 1 -- plant p's element of column c is at (p / pitch) * pitch * columns +
 * c * pitch + p % pitch.  (Measured: the step of 65 536 plants is 5 % faster on such an arena than on one block, that
 * of 262 144 plants 10 %.) */
NPB_API int npb_state_arena(NpbHandle *h, void **arena, size_t *pitch, int *storage);
NPB_API size_t npb_state_arena_segment(const NpbHandle *h);
/* The same with the whole layout in one answer: *segment = plants per segment (0 = one block), *columns = arena columns of the
 * handle's storage type.  npb_state_arena itself REFUSES to hand out the pointer of a segmented arena (NPB_EINVAL, npb_last_error
 * says why): a caller written before segments existed would compute arena + (column * pitch + plant) * width and touch the wrong
 * plants without any error.  A raw-arena dump is a checkpoint only together with (pitch, segment, columns, storage): record them.
 * Asking for the layout alone (arena = NULL) does not invalidate the maintenance cooldown cache; asking for the pointer does. */
NPB_API int npb_state_arena_layout(NpbHandle *h, void **arena, size_t *pitch, size_t *segment, int *columns, int *storage);
/* (With params.maint_enabled the step kernels consult a cache of which maintenance thresholds are inside their cooldown; every
 * entry point that can change state, the table or the clock invalidates it, this one included.  A caller that keeps the pointer
 * and writes the arena between later steps calls npb_state_arena again after each such write.) */
/* where a field lives: arena column, position of a narrow member inside the column (0/1), and how it is stored
 * (0 = carried real of the column width, 1 = output real stored as float, 2 = int32); element address =
 * arena + (column * pitch + plant) * width + sub * 4, width = 8 (NPB_STORAGE_F64) or 4 (NPB_STORAGE_F32) */
NPB_API int npb_locate_field(const NpbHandle *h, int kind, int slot, int *column, int *sub, int *access);

/* NuclearPlantSimulator.step (sim.py:130-258) for every plant.  Input columns (device, n_plants each)
 * may be NULL: action -> NO_ACTION(8), magnitude -> 1.0, power_setpoint -> unchanged
 * (NaN entries also mean unchanged; replaces heat_source.set_power_setpoint), noise_z -> 0
 * (standard-normal sample that ConstantHeatSource would draw, constant_heat_source.py:178),
 * cooling_water_temp -> unchanged.  Output columns (device) may be NULL:
 * obs [n,22] row-major, reward [n], done [n] u8, trip_flags [n] u32, info [n,NPB_INFO_DIM] (+ [n,NPB_INFO_NRHO] behind it with
 * params.info_reactivity_components).  Under NPB_HEAT_EXTERNAL the noise_z / power_setpoint columns carry the caller's heat
 * source (include/npb_params.h).
 * With params.maint_enabled the automatic maintenance of the feedwater pumps -- the handle's threshold table (npb_maint.h), the
 * orchestrator's rule, the work-order queue, the thirteen handlers -- runs after the physics, in the reference's order
 * (sim.py:208-223: AutoMaintenanceSystem.update, then the state manager's threshold scan), inside the same launch (full mode);
 * its state and counters are the maint.* / mpump.* columns of npb_fields.h. */
NPB_API int npb_step(NpbHandle *h, const int32_t *action, const double *magnitude, const double *power_setpoint,
             const double *noise_z, const double *cooling_water_temp, double *obs, double *reward, uint8_t *done,
             uint32_t *trip_flags, double *info, void *stream);

/* Have npb_step write the NPB_DIAG_* columns of every following step into buf ([NPB_DIAG_DIM][pitch] doubles on the handle's
 * device, pitch >= n_plants rounded up to a multiple of 64; NULL = off, the default).  While it is set the step runs the diagnostics build of the one-wave
 * kernel at every batch size (same results, ~1.4x the time at small batches); full mode only. */
NPB_API int npb_set_diagnostics(NpbHandle *h, double *buf, size_t pitch);
/* The carried rows (NPB_DIAG_CARRIED): how many, row k's number, the value row k has in a freshly constructed plant. */
NPB_API int npb_diag_num_carried(void);
NPB_API int npb_diag_carried_row(int k);        /* -1 outside [0, npb_diag_num_carried()) */
NPB_API double npb_diag_carried_fresh(int k);   /* NaN outside */
/* on != 0: the handle treats the carried rows of the caller's diagnostics buffer as plant state.  The buffer stays the live copy -- the
 * step kernels read and write it as before -- and npb_snapshot records the rows beside the snapshot arena, npb_set_start_bank copies the
 * bank handle's beside the bank, npb_restore / npb_restore_bank / the autoreset put them back per plant with the arena, npb_reset puts a
 * freshly constructed plant's values and npb_reset_reference what NuclearPlantSimulator.reset() leaves (every row to its fresh value,
 * the stage system's efficiency as 1.0, except the ejectors' compression ratios, which are kept), for the plants they reset.  Needs a buffer set by
 * npb_set_diagnostics (so: full mode); NPB_EINVAL otherwise.  While it is on, npb_set_autoreset is accepted if the source it restores
 * from (the snapshot, or the bank with slots) was recorded with the rows, and while both are on npb_set_diagnostics (any buffer, or
 * NULL) and npb_carry_diagnostics(h, 0) are refused; without autoreset npb_set_diagnostics with another buffer is refused while carrying
 * is on (switch carrying off first) and NULL switches both off.  A handle that never calls this behaves as before in every entry point. */
NPB_API int npb_carry_diagnostics(NpbHandle *h, int on);
/* the carried rows of every plant as [npb_diag_num_carried()][n_plants] doubles (device or host), in table order: what a checkpoint
 * saves beside the arena.  Synchronous on `stream`.  NPB_EINVAL without carrying. */
NPB_API int npb_get_diagnostics_state(NpbHandle *h, double *buf, void *stream);
NPB_API int npb_set_diagnostics_state(NpbHandle *h, const double *buf, void *stream);

/* Which of the two step kernels npb_step launches (same device functions in the same per-plant order: identical int32
 * columns and flags, reals equal to the last bit or two; this is a measurement / A-B aid):
 * 0 = by batch size (default; also the environment variable NPB_STEP_KERNEL at handle creation), 1 = one wavefront per
 * 64 plants with an LDS-DMA staging pipeline, 2 = two wavefronts per 64 plants that own different subsystems (two builds of
 * it: the whole register file up to 32 768 plants, where a SIMD holds one wave anyway, 256 registers above), 3 = the
 * 256-register build at any size, 4 = the one-wavefront kernel with streaming (non-temporal) state stores, which 0 takes
 * above ~90 000 plants of fp64 storage, where nothing a step writes is still cached when the next step reads it, 5 = four
 * wavefronts per 64 plants handing values to each other through progress words in LDS (what 0 takes up to 32 768 plants,
 * where all of its 2 048 wavefronts are resident at once, and again between 45 057 and 114 688 plants, on the segmented
 * arena handles of that size have, npb_state_arena). */
NPB_API int npb_set_step_kernel(NpbHandle *h, int variant);
/* Which kernel the handle's last npb_step actually launched (NPB_KERNEL_NONE before the first step): the selection above is by
 * batch size, mode, storage and override, and a test or a benchmark that means to exercise one kernel asserts it here instead
 * of trusting the selection rule.  npb_step_kernel_name(id) = the kernel's symbol as rocprofv3 lists it. */
enum {
  NPB_KERNEL_NONE = 0,
  NPB_KERNEL_STEP = 1,         /* npb_step_kernel: one wavefront per 64 plants */
  NPB_KERNEL_STEP2_WIDE = 2,   /* npb_step2_wide_kernel: two wavefronts, the whole register file (<= 32 768 plants) */
  NPB_KERNEL_STEP2 = 3,        /* npb_step2_kernel: two wavefronts, 256 registers (two waves per SIMD) */
  NPB_KERNEL_STEP_NT = 4,      /* npb_step_nt_kernel: one wavefront, streaming state stores */
  NPB_KERNEL_STEP_DIAG = 5,    /* npb_step_diag_kernel: one wavefront, step-internal diagnostics written (npb_set_diagnostics) */
  NPB_KERNEL_STEP_PRIMARY = 6, /* npb_step_primary_kernel: NPB_MODE_PRIMARY */
  /* the builds of 1-4 with the automatic maintenance compiled in (params.maint_enabled, full mode): same step, same results */
  NPB_KERNEL_STEP_MAINT = 7, NPB_KERNEL_STEP2_WIDE_MAINT = 8, NPB_KERNEL_STEP2_MAINT = 9, NPB_KERNEL_STEP_NT_MAINT = 10,
  NPB_KERNEL_STEP4 = 11,       /* npb_step4_kernel: four wavefronts per 64 plants, 256 registers (two waves per SIMD at 32 768 plants) */
  NPB_KERNEL_STEP4_MAINT = 12,
  NPB_KERNEL_COUNT_
};
NPB_API int npb_debug_last_step_kernel(const NpbHandle *h);
NPB_API const char *npb_step_kernel_name(int kernel_id);

/* NuclearPlantSimulator.get_observation (sim.py:290-333) */
NPB_API int npb_observe(NpbHandle *h, double *obs, void *stream);

/* Episodes (no reference counterpart: the reference steps one simulator until the caller builds a new one).  The semantics are
 * gymnasium's vector-env "same-step" autoreset with truncation.
 * npb_snapshot: copy the whole arena into a snapshot arena the handle owns -- the same layout (segments, pitch, storage type), one
 * device-to-device copy on `stream` -- allocated on first use (NPB_EHIP if that fails), freed by npb_destroy.  Take it after the
 * initial conditions have been put in (npb_set_field ...): it is each plant's episode-start state.  Episode counters are not touched. */
NPB_API int npb_snapshot(NpbHandle *h, void *stream);
/* the plants of mask (device, uint8[n], NULL = all) back to the snapshot, their episode counters (if any) to zero; with
 * params.maint_enabled their maintenance cooldown cache and their entries in the event-count column follow.  NPB_EINVAL without a
 * snapshot.  Follow with npb_observe for the restored observation. */
NPB_API int npb_restore(NpbHandle *h, const uint8_t *mask, void *stream);
/* enabled != 0: every npb_step is followed, on the same stream, by the episode kernel (no host synchronisation, nothing read back):
 * per plant len += 1, ret += reward; truncated = max_episode_steps > 0 && len >= max_episode_steps && !done (termination wins);
 * a plant with done | truncated goes back to the snapshot as npb_restore would, its obs row is first copied to final_obs and
 * then replaced by the restored state's observation; reward, info and trip_flags keep describing the terminal transition.  The
 * episode buffers (npb_set_episode_buffers) receive len / ret as of this step (a reset plant's: its finished episode's) and the
 * truncation flag.  With a start bank and slots (npb_set_start_bank, npb_set_start_slots) the reset plants are restored from their
 * bank entries instead.  Needs a snapshot, or a bank and slots; allocates the handle's carried counters (int32 length[pitch], double return[pitch]) and
 * zeroes them; npb_step then needs a non-NULL done column.  Refused (NPB_EINVAL) while npb_set_diagnostics is set, as that is
 * refused while autoreset is on: the diagnostics buffer carries plant state outside the arena -- unless npb_carry_diagnostics is on
 * and the snapshot (or the bank) was recorded with the carried rows, which the restores then take along.  enabled = 0 turns it off.
 * npb_reset, npb_reset_reference and npb_restore zero the counters of the plants they reset. */
NPB_API int npb_set_autoreset(NpbHandle *h, int enabled, int max_episode_steps /* 0 = no limit */);
/* the caller's output columns of the episode kernel (device; each may be NULL): length int32[n], ret double[n], truncated
 * uint8[n], final_obs double[n][NPB_OBS_DIM] (rows of plants reset on the step; other rows are left as they were) */
NPB_API int npb_set_episode_buffers(NpbHandle *h, int32_t *length, double *ret, uint8_t *truncated, double *final_obs /* [n,22] */);
/* Start bank: restarts from a bank of M start states instead of each plant's own snapshot lane (M independent of n).
 * npb_set_start_bank: copy src's whole arena into a bank arena h owns -- one device-to-device copy on `stream`; M =
 * npb_num_plants(src); the bank keeps src's layout (pitch, segment size), src may be h itself.  NPB_EINVAL if the storage type or
 * the device differs.  Called again it replaces the bank (reallocating only if the new one needs more room).  src = NULL frees the
 * bank, refused while autoreset is on and the handle has no snapshot to fall back on.  npb_destroy frees it.  Setting a bank
 * (first, or after freeing it) puts every plant's carried start entry (npb_set_episode_start_buffer) to -1. */
NPB_API int npb_set_start_bank(NpbHandle *h, const NpbHandle *src, void *stream);
/* which bank entry each restore takes (device int32[n] columns the caller owns; episode_start may be NULL): plant p restored from the
 * bank takes entry s = ((next_slot[p] % M) + M) % M, defined for any value the caller wrote, and the library then stores
 * next_slot[p] = (s + advance) % M and episode_start[p] = s.  advance = 0 leaves every restart to the caller (e.g. random slots written
 * on the same stream).  NPB_EINVAL for next_slot = NULL or advance < 0.  With a bank and slots, npb_step's autoreset restores from
 * the bank instead of the snapshot. */
NPB_API int npb_set_start_slots(NpbHandle *h, int32_t *next_slot, int32_t *episode_start, int advance);
/* npb_restore's counterpart: the plants of mask (device, uint8[n], NULL = all) from their bank entries, episode counters (if any) to
 * zero; with params.maint_enabled their cooldown cache and event counts follow, as npb_restore's do.  NPB_EINVAL without a bank and
 * slots.  Follow with npb_observe for the restored observation. */
NPB_API int npb_restore_bank(NpbHandle *h, const uint8_t *mask, void *stream);
/* a caller column (device int32[n], NULL = none) the autoreset from the bank fills on every step with the bank entry of the episode this
 * step's transition belonged to (a plant reset on the step: its finished episode's, as length / ret of npb_set_episode_buffers).
 * -1 for an episode that did not start from the bank: construction, npb_reset, npb_reset_reference and npb_restore put the carried
 * entry to -1. */
NPB_API int npb_set_episode_start_buffer(NpbHandle *h, int32_t *out_start);
/* Episode index: with autoreset the handle counts each plant's episodes -- one int32 per plant, zeroed by npb_set_autoreset and bumped
 * wherever the plant's episode length is zeroed (the autoreset, npb_restore, npb_restore_bank, npb_reset, npb_reset_reference).  A
 * caller column (device int32[n], NULL = none) receives on every step the index of the episode this step's transition belonged to (a
 * plant reset on the step: its finished episode's, as length / ret of npb_set_episode_buffers). */
NPB_API int npb_set_episode_index_buffer(NpbHandle *h, int32_t *index);

/* Heat-source noise streams on the device (constant_heat_source.py:58-62,178: each ConstantHeatSource owns a
 * np.random.RandomState(seed) and draws rng.normal(0, sigma) per step, i.e. sigma * standard_normal()).  One MT19937 per plant,
 * owned by the handle (about 2.5 KB a plant), that follows numpy.random.RandomState(seed).standard_normal() -- legacy_gauss: the polar
 * method with its one-value cache: the integer state (key, pos, has_gauss) is numpy's exactly and every draw is within a few ulp of
 * numpy's (only the fp64 log is the device library's).  The step kernels do not change: npb_noise_fill writes a [k][n] block whose
 * row t npb_step takes as its noise_z column.
 * npb_noise_seed: plant p's generator becomes RandomState(seeds[p]) (seeds: host int64[n]); allocated on first use, freed by
 * npb_destroy, or by seeds = NULL.  NPB_EINVAL for a seed outside [0, 2^32), as numpy refuses it.  Returns once the seeding is done. */
NPB_API int npb_noise_seed(NpbHandle *h, const int64_t *seeds, void *stream);
/* the next k standard_normal() draws of every plant into out (device, double[k][n]: out[t * n + p]), enqueued on `stream`.
 * Allocates nothing.  NPB_EINVAL if the handle has no generators or k < 1. */
NPB_API int npb_noise_fill(NpbHandle *h, int k, double *out, void *stream);
/* the generators' state in numpy's RandomState.get_state() layout (host buffers): key uint32[n][624], pos int32[n] (0-624),
 * has_gauss int32[n] (0 | 1), cached double[n] (0.0 when has_gauss is 0).  Synchronous on `stream`.  NPB_EINVAL without generators.
 * npb_noise_set_state loads such a state (allocating the generators if there are none): checkpoints, and a host stream continued on
 * the device.  It refuses pos outside [0, 624] and has_gauss outside {0, 1}. */
NPB_API int npb_noise_get_state(NpbHandle *h, uint32_t *key, int32_t *pos, int32_t *has_gauss, double *cached, void *stream);
NPB_API int npb_noise_set_state(NpbHandle *h, const uint32_t *key, const int32_t *pos, const int32_t *has_gauss, const double *cached, void *stream);

/* The data-gen runner's power profile on the device, per plant (maintenance_scenario_runner.py:586-671; nuclear_sim_amd/scenarios.py
 * power_profile_rows is the readable statement).  Per run of `steps` rows the runner draws z = np.random.normal(0, 1, steps) from numpy's
 * global legacy stream and makes, in this order,
 *   raw = clip(base + min(0.2, std) * z, 20, 105)
 *   sm[i] = (raw[i-1] + raw[i] + raw[i+1]) / 3.0 for 0 < i < steps - 1, sm = raw at both ends (and everywhere if steps < 3)
 *   target[0] = sm[0];     target[i] = sm[i] if |sm[i] - target[i-1]| <= 0.05, else target[i-1] -/+ 0.05         (logged as target_power)
 *   setpoint[0] = target[0]; setpoint[i] = target[i] if |target[i] - setpoint[i-1]| <= 0.02, else setpoint[i-1] -/+ 0.02 (given to the heat source)
 * Here every plant has a stream of its own: a SECOND set of MT19937 generators in the handle (the layout of the heat-source noise's,
 * about 2.5 KB a plant again, allocated on first use, freed by npb_destroy; independent of npb_noise_*, so both can be on) drawn by the
 * same fill kernel into a block the handle owns, and a filter kernel that turns the block into rows.  Given the draws, the filter's rows
 * are exactly numpy's (no contraction, IEEE division); the draws are within a few ulp of numpy's, as npb_noise_fill's are.
 * All plants advance together: the handle keeps ONE position, the rows made of the current profile -- unless episode streams are on
 * (npb_set_episode_streams below), where every plant has a position of its own and restarts its profile with its episode.  A block may
 * cross a profile's end:
 * the profile's last row takes no draw, and the next row starts the next profile of the same horizon from the next draw, its ramp
 * afresh (first setpoint = first target) -- a second runner on the same stream.
 * Generator state: after R rows in all (q whole profiles and r = R mod steps rows of the next) every generator is numpy's
 * RandomState(seed) after R standard_normal() calls -- plus ONE, the moving average's look-ahead, when steps >= 3 and r >= 1.  At a
 * profile's end (r = 0) it is exactly numpy's after q * steps draws.
 * npb_profile_seed: plant p's stream becomes RandomState(seeds[p]) (host int64[n]; NPB_EINVAL outside [0, 2^32)), position 0, profiles of
 * `steps` >= 1 rows.  base / std: the load profile's base_power_percent / noise_std_percent, host doubles -- NULL (90.0 / 2.0, the
 * runner's defaults), n_base / n_std = 1 (one value for all) or n (one per plant).  seeds = NULL frees the profile.  Returns once done. */
NPB_API int npb_profile_seed(NpbHandle *h, const int64_t *seeds, int steps, const double *base, int n_base, const double *std, int n_std, void *stream);
/* the next k rows of every plant, enqueued on `stream`: setpoint_out, target_out, z_out device double[k][n] (row t of plant p at
 * [t * n + p]); target_out and z_out may be NULL.  z_out[t] is the draw behind row t's raw value: power_profile_rows(z_out) must equal
 * the other two bit for bit.  Allocates only when k exceeds every earlier k (the draw block grows; that call waits for the stream).
 * NPB_EINVAL before npb_profile_seed, for k < 1 and for a NULL setpoint_out. */
NPB_API int npb_profile_fill(NpbHandle *h, int k, double *setpoint_out, double *target_out, double *z_out, void *stream);
/* The ramp stage alone, on the caller's targets (_set_target_power for any block): setpoint_out[t] from target_in[t] (device
 * double[k][n] each; they may be the same block) and the previous setpoint the handle carries per plant from call to call -- NaN at
 * first, which means "first call": that setpoint is its target.  No profile needed.  k = 0 with both blocks NULL forgets the carried
 * setpoints.  NPB_EINVAL for k < 1 or a NULL block otherwise. */
NPB_API int npb_profile_ramp(NpbHandle *h, int k, const double *target_in, double *setpoint_out, void *stream);
/* Checkpoints (host buffers, synchronous on `stream`): the generators as npb_noise_get_state gives them (numpy's get_state() layout),
 * the filter's carried values, double[5][n]: the clipped raw value of the row before the next and of the next row (the look-ahead), the
 * draw behind the latter, the previous target, the previous setpoint (meaningful from position 1 on), and the position.  The horizon
 * and the load profiles are configuration: npb_profile_set_state needs npb_profile_seed (same steps, base, std) first and refuses,
 * beside what npb_noise_set_state refuses, a position outside [0, steps). */
NPB_API int npb_profile_get_state(NpbHandle *h, uint32_t *key, int32_t *pos, int32_t *has_gauss, double *cached, double *carried, int32_t *position, void *stream);
NPB_API int npb_profile_set_state(NpbHandle *h, const uint32_t *key, const int32_t *pos, const int32_t *has_gauss, const double *cached, const double *carried,
                                  int32_t position, void *stream);

/* Episode streams: each plant's heat-source noise and power profile restart with its episode.  Off (the default) the two streams run
 * on across restarts as described above; on, every (plant, episode) takes the rows a freshly built runner of its scenario would: the
 * reference's runner builds a new ConstantHeatSource(seed 42) and draws a new load profile for every run
 * (maintenance_scenario_runner.py:210-244, :586-671).  nuclear_sim_amd/scenarios.py episode_stream_rows is the readable statement.
 * While the mode is on the HANDLE owns the streams' consumption: [block][n] blocks of noise, setpoint and target rows of its own, one
 * cursor per stream, and per plant the row of its current profile (int32) in place of the single position.  npb_step given a NULL noise_z
 * (with noise generators) or a NULL power_setpoint (with a profile) takes the handle's current row of that stream and moves that cursor;
 * an explicit column is used as before and consumes no row of that stream.  A block that has run out is made again, for every plant from
 * where its streams are, before the step that needs it.  Nothing is read back and nothing synchronises.
 * A plant RESTARTS wherever its episode index is bumped: the autoreset behind npb_step, npb_restore, npb_restore_bank, and npb_reset /
 * npb_reset_reference for the plants of their mask.  On the same stream, behind that call's own kernels, a restart kernel then gives the
 * plant both streams of its new episode from their beginning: both generators seeded anew, the profile's position, rows made and carried
 * values zeroed -- the ramp starts afresh, first setpoint = first target --, and the rows drawn ahead for it in the handle's blocks made
 * again from the new streams, so that no row of the old episode reaches a step.  (On a block's last row nothing is pending: the next
 * refill begins the new episode.)  The j-th step after a restart that takes a stream's row takes draw j of the new noise stream, and row
 * j mod steps of consecutive profiles of the new profile stream.  Seeds: a restart that took bank entry s (what episode_start reports)
 * uses bank_noise_seeds[s] / bank_profile_seeds[s] where that table was given; every other restart -- from the snapshot, a reset, no
 * table -- uses the plant's own seed again, as given to npb_noise_seed / npb_profile_seed (the handle keeps them), so a restart from the
 * snapshot repeats the plant's first episode exactly.  base / std stay with the plant position.
 * Generator state, per plant: after m rows made since its restart (rows taken plus rows drawn ahead and not yet taken) its noise
 * generator is numpy's after m calls and its profile generator after m calls plus the one look-ahead when steps >= 3 and m % steps >= 1:
 * the rule stated above for the whole batch.  A lane draws exactly what its rows use.
 * npb_set_episode_streams(h, desc, stream): desc = NULL switches the mode off.  It works on whichever of the two generator sets the
 * handle has (npb_noise_seed, npb_profile_seed); switching on -- and switching off -- is itself a restart of every plant from its own
 * seeds, with nothing drawn ahead (off: the profile's single position is 0 again).  It needs the autoreset on (npb_set_autoreset: the
 * restarts are read off the episode index it keeps).  The three output columns (device double[n], the caller's, each may be NULL) receive
 * the rows each step takes from the handle's streams: noise_out the noise_z, setpoint_out the setpoint, target_out the row before the
 * ramp (the runner's target_power); a step given that column explicitly leaves them as they were.  They are written on the step's stream
 * in the restart kernel's launch behind the step, not in a launch of their own.
 * Everything is validated before any device work and refused by name (npb_last_error; npb_episode_streams_check is that check alone,
 * without a handle: NULL = accepted): no generators; block < 1; a table without a bank; n_bank_seeds that is not the bank's entry count;
 * a table seed outside [0, 2^32); generators that were only ever loaded (npb_noise_set_state) and have no seed; no autoreset.  While
 * tables are set, npb_set_start_bank with another entry count, or with NULL, is REFUSED: switch the mode off first.
 * While the mode is on npb_noise_fill, npb_profile_fill, npb_noise_set_state, npb_profile_set_state, npb_noise_seed and npb_profile_seed
 * are refused (NPB_EINVAL, naming the mode); npb_noise_get_state and npb_profile_get_state keep working, the latter reporting position
 * -1, and npb_profile_get_positions gives the per-plant values (host int32[n] each, either may be NULL; synchronous on `stream`;
 * NPB_EINVAL without the mode or without a profile).
 * NOT part of this: checkpointing a handle in this mode in the middle of a block -- the rows drawn ahead and the cursors are not
 * exported, and the get_state calls give the generators as they are after the rows made.  The arena's own state is unaffected. */
typedef struct {
  int block;                                   /* rows per refill, >= 1 */
  const int64_t *bank_noise_seeds;             /* host int64[n_bank_seeds] or NULL */
  const int64_t *bank_profile_seeds;           /* host int64[n_bank_seeds] or NULL */
  int n_bank_seeds;                            /* the bank's entry count when a table is given */
  double *noise_out, *setpoint_out, *target_out;   /* device double[n] each, or NULL */
} npb_episode_streams_desc_t;
NPB_API int npb_set_episode_streams(NpbHandle *h, const npb_episode_streams_desc_t *desc, void *stream);
/* has_generators: the handle has noise generators or a profile; bank_entries: 0 = no bank */
NPB_API const char *npb_episode_streams_check(const npb_episode_streams_desc_t *desc, int has_generators, int bank_entries);
NPB_API int npb_profile_get_positions(NpbHandle *h, int32_t *position /* host [n] */, int32_t *rows_made /* host [n], since the last restart */, void *stream);

/* Episode records: a device-side log of FINISHED episodes, each record complete -- who, which episode, from which bank entry, how long, the
 * return, how it ended, when on the plant's clock, optionally the terminal observation and that episode's work-order summary -- so that a run
 * of any length yields the table of its episodes with one read-back whenever the caller chooses, instead of one per step (the episode
 * columns of npb_set_episode_buffers are overwritten by every step).
 * The record is a struct of arrays the caller owns (device), `capacity` entries per column:
 *   plant int32        handle-local plant number
 *   episode int32      the plant's episode index (npb_set_episode_index_buffer)
 *   start int32        the bank entry the episode started from; -1 if there is no bank or the episode did not begin from it
 *   length int32       steps of the episode, the terminal one included
 *   flags int32        bit 0 terminated (done), bit 1 truncated (max_episode_steps); termination wins, as in npb_set_autoreset
 *   trip_flags uint32  the terminal step's trip_flags column; 0 if npb_step was given NULL
 *   step int32         number of npb_step calls since the records were switched on, the terminal one = 0 for the first
 *   ret double         summed reward of the episode (the carried sum; unchanged by a step given reward = NULL)
 *   end_time double    prim.sim_time after the terminal step, as npb_get_field returns it under the handle's storage type: the clock the
 *                      maintenance records' `time` comes from
 *   final_obs double [capacity][NPB_OBS_DIM] row-major, NULL = not recorded: the step's obs row before the autoreset replaces it.  While it
 *                      is set npb_step refuses obs = NULL.
 *   first_created, first_completed double [n_keys][capacity], n_created, n_completed int32 [n_keys][capacity]: the plant's cells of the
 *                      handle's work-order summary (npb_set_maintenance_summary) as of the terminal step, element [key * capacity + slot];
 *                      all four or none (NULL)
 *   cursor uint32      one word: slots handed out
 * While records are on npb_step launches one more kernel on its stream, behind the summary fold and before the episode kernel -- so the
 * arena, the step's output columns and the carried episode counters still describe the episode that ended and the summary holds the step's
 * events.  It decides "ended" by the episode kernel's own rule; a wave without an ended plant writes nothing.  The ended plants of one wave
 * take consecutive slots in plant order with ONE atomic add to *cursor; waves arrive in no particular order.  A record is stored only
 * while slot < capacity: a cursor past the capacity counts the episodes that were dropped, as the maintenance log's does.  The caller
 * drains on its stream: read the cursor, copy min(cursor, capacity) entries of each column, zero the cursor.
 * clear_summary != 0: the summary cells of every ended plant go back to +inf / 0 for every key -- whether or not its record fitted -- so
 * the summary restarts with the episode and each record holds the work orders of its own episode only.  Off, the summary goes on counting
 * across restarts as before.
 * The records are output only: npb_snapshot / npb_restore, the start bank and checkpoints neither read nor reset them.  An episode the
 * caller ABANDONS -- npb_restore, npb_restore_bank, npb_reset, npb_reset_reference of a running plant -- bumps the plant's episode index
 * and writes NO record (and clears no summary row): records are of episodes that ended by done or truncation.
 * npb_set_episode_records(h, desc): desc = NULL turns the records off; the descriptor is copied and the step counter starts at 0.
 * NPB_EINVAL, with the reason in npb_last_error, for: no autoreset (npb_set_autoreset first); capacity < 1; a NULL or misaligned mandatory
 * column or cursor (doubles 8-byte, the others 4-byte); summary columns, or clear_summary, without a summary set; only part of the four
 * summary tables.  npb_episode_records_check is that check alone, without a handle (summary_keys = the summary's n_keys, 0 = none set):
 * NULL = accepted, else the reason.
 * While records that copy or clear the summary are on, npb_set_maintenance_summary (another descriptor, or NULL) and
 * npb_set_maintenance_log(NULL) are refused; while any records are on npb_set_autoreset(h, 0) is refused: switch the records off first.
 * A handle that never calls this behaves as before in every entry point. */
typedef struct npb_episode_records_desc_t {
  int32_t capacity;                             /* entries per column, >= 1 */
  int32_t clear_summary;                        /* != 0: an ended plant's summary cells back to +inf / 0 */
  int32_t *plant, *episode, *start, *length, *flags;
  uint32_t *trip_flags;
  int32_t *step;
  double *ret, *end_time;
  double *final_obs;                            /* [capacity][NPB_OBS_DIM] or NULL */
  double *first_created, *first_completed;      /* [n_keys][capacity], all four or none */
  int32_t *n_created, *n_completed;
  uint32_t *cursor;                             /* one word */
} npb_episode_records_desc_t;
NPB_API int npb_set_episode_records(NpbHandle *h, const npb_episode_records_desc_t *desc);
NPB_API const char *npb_episode_records_check(const npb_episode_records_desc_t *desc, int has_autoreset, int summary_keys);

/* Column statistics: what a plant's STATE did, folded on the device into a handful of numbers per (column, plant) -- the lowest oil level,
 * the peak tube-wall temperature, the mean electrical power, how long a level sat beyond a limit and when it first got there -- instead
 * of a time series that somebody has to drain.  A column is an arena member (kinds / slots, as npb_gather_fields and npb_sampler_create
 * take them) or a side row: a caller-owned DEVICE buffer of one value per plant (npb_sample_source_t with rows == 1: an info column, an
 * obs column, the reward, a diagnostics row).  Members come first, then the side rows, n_cols = n_fields + n_sources <=
 * NPB_COLUMN_STATS_MAX.  Every sample is widened to double as npb_sample_kernel widens it, and folded into the caller's device tables:
 *   n_samples int32 [n_plants]             samples folded (mandatory)
 *   min, max  double [n_cols][n_plants]    v < min ? v : min, v > max ? v : max: a NaN sample replaces neither; empty +inf / -inf
 *   sum, sumsq double [n_cols][n_plants]   sum + v, sumsq + v * v (the product rounded before the add: the library is built with
 *                                          -ffp-contract=off), sequential in step order; empty 0
 *   last double [n_cols][n_plants]         the latest sample; empty NaN
 *   first_beyond double [n_cols][n_plants] for a column with a limit (direction[c] = +1: v > limit[c], -1: v < limit[c], 0: no limit): the
 *                                          plant clock prim.sim_time (as npb_get_field returns it) after the first step whose sample was
 *                                          beyond the limit; empty +inf = never
 *   n_beyond int32 [n_cols][n_plants]      samples that were beyond the limit; empty 0
 * element [column * n_plants + plant].  Any table but n_samples may be NULL: not kept, not touched.  The caller initialises the tables
 * with the empty values, or calls npb_column_stats_clear.  nuclear_sim_amd/colstats.py states the fold in numpy; the device produces its
 * bits.
 * With stats set npb_step launches ONE more kernel on its stream (grid (ceil(n / 256), n_cols), a thread per cell, no atomics): behind the
 * step kernel, the rule and the work-order summary fold, BEFORE the episode-records kernel and the episode kernel -- the sample is the
 * end-of-step state of the episode the step belonged to, before any restore.  npb_column_stats_fold is the same launch on request;
 * npb_column_stats_clear puts the plants of mask (device uint8 [n_plants], NULL = all) back to the empty values in every table kept.  Both
 * are NPB_EINVAL without stats.  The npb_perform_*_maintenance calls do not fold.
 * Output only, like the work-order summary: npb_snapshot / npb_restore, the resets, the start bank, the autoreset and checkpoints neither
 * read nor reset the tables.
 * npb_set_column_stats(h, desc): desc = NULL turns the stats off.  The descriptor is copied (its host arrays too).  NPB_EINVAL with the reason
 * in npb_last_error, before any device work, for what npb_column_stats_check refuses -- that check alone, without a handle, NULL =
 * accepted, else the reason: a column count outside 1..NPB_COLUMN_STATS_MAX; a bad kind or slot; a source with a NULL base, an unknown
 * type or rows != 1; a direction outside {-1, 0, +1}; a NaN limit; a NULL n_samples; a misaligned table (doubles 8-byte, int32 4-byte);
 * first_beyond or n_beyond with no limit set.  NPB_VERSION stays 154: a binding detects the entry points by name.
 * A handle that never calls this behaves as before in every entry point. */
#define NPB_COLUMN_STATS_MAX 32
typedef struct npb_column_stats_desc_t {
  int n_fields; const int *kinds; const int *slots;      /* host; arena members, n_fields may be 0 */
  int n_sources; const npb_sample_source_t *sources;     /* host descriptors of one-row device buffers; n_sources may be 0 */
  const int *direction;                                  /* host [n_cols]: +1, -1, 0 = no limit; NULL = no limits */
  const double *limit;                                   /* host [n_cols]; read where direction != 0 */
  double *min, *max, *sum, *sumsq, *last, *first_beyond; /* device [n_cols][n_plants], each or NULL */
  int32_t *n_beyond;                                     /* device [n_cols][n_plants] or NULL */
  int32_t *n_samples;                                    /* device [n_plants] */
} npb_column_stats_desc_t;
NPB_API int npb_set_column_stats(NpbHandle *h, const npb_column_stats_desc_t *desc);
NPB_API const char *npb_column_stats_check(const npb_column_stats_desc_t *desc, int n_plants);
NPB_API int npb_column_stats_fold(NpbHandle *h, void *stream);
NPB_API int npb_column_stats_clear(NpbHandle *h, const uint8_t *mask, void *stream);
/* The statistics of each EPISODE in its record (npb_set_episode_records): a descriptor of its own, so that npb_episode_records_desc_t
 * keeps its layout.  Record-side columns double / int32 [n_cols][capacity], element [column * capacity + slot], and n_samples int32
 * [capacity], each NULL or set -- set only where the handle keeps that statistic.  npb_episode_records_kernel then copies an ended plant's
 * cells into its slot as it copies the work-order summary's, and with clear != 0 puts them back to the empty values, whether or not the
 * record fitted: each record then holds the statistics of its own episode and n_samples == length.  Needs records and stats both on
 * (NPB_EINVAL otherwise, and for a misaligned column).  While it is set npb_set_column_stats (another descriptor, or NULL) is refused;
 * desc = NULL drops it, and so does EVERY successful npb_set_episode_records, with a descriptor or with NULL: the record-side columns
 * belong to one set of record columns and their capacity, so a caller who sets the records again calls this again behind it.  The
 * handle keeps what the kernel reads of both descriptors in device memory of its own and hands the kernel one pointer; the call
 * uploads it synchronously.  Off, the records kernel stores exactly what it stored before. */
typedef struct npb_episode_record_stats_desc_t {
  double *min, *max, *sum, *sumsq, *last, *first_beyond; /* device [n_cols][capacity], each or NULL */
  int32_t *n_beyond;                                     /* device [n_cols][capacity] or NULL */
  int32_t *n_samples;                                    /* device [capacity] or NULL */
  int clear;                                             /* != 0: an ended plant's cells back to the empty values */
} npb_episode_record_stats_desc_t;
NPB_API int npb_set_episode_record_stats(NpbHandle *h, const npb_episode_record_stats_desc_t *desc);

/* Event windows: what a plant looked like AROUND a trip, a work order or a limit being crossed, without logging every plant and without
 * choosing the plants beforehand -- a trigger, as an oscilloscope has one.  Every plant keeps the last H = pre + 1 + post samples of up to
 * NPB_EVENT_WINDOW_COLS_MAX columns (and its clock, prim.sim_time) in a ring the handle owns; a trigger arms a capture, and `post` steps
 * later the window -- `pre` samples before the trigger, the trigger sample, `post` after -- goes into a record of the caller's, drained
 * whenever the caller chooses.  The volume of output follows the events, not plants x steps.
 * Recorded columns: n_fields / kinds / slots and n_sources / sources exactly as npb_column_stats_desc_t takes them (members first, then the
 * one-row side sources), widened to double as npb_sample_kernel widens them; n_cols = n_fields + n_sources.
 * Triggers: 1 .. NPB_EVENT_WINDOW_TRIGGERS_MAX, each a column of its own (an arena member, or a side source; it need not be recorded) and
 * a mode, comparing the sample v with the previous sample prev of the same plant:
 *   NPB_TRIGGER_BITS_RISE(mask)             integer column (an int32 member, an I32 or U8 source): (v & mask) & ~(prev & mask) != 0
 *   NPB_TRIGGER_INCREASE                    v > prev; a NaN on either side does not fire
 *   NPB_TRIGGER_BEYOND(direction, limit)    the edge only: beyond now (+1: v > limit, -1: v < limit, the statistics' rule) and not beyond at
 *                                           the previous sample
 * With windows set npb_step launches ONE more kernel on its stream, one wave per 64 plants: behind the column-statistics fold and BEFORE
 * the episode-records kernel and the episode kernel -- the sample is the end-of-step state of the episode the step belonged to, and the
 * work-order summary already holds this step's events.  For plant p at sample s (0 = the first npb_step after the set):
 *   1. where the handle carries an episode index (npb_set_autoreset) and it differs from the one last seen, the plant was restarted since
 *      the last sample (autoreset, npb_restore*, npb_reset*): its ring is empty, it is unprimed, and an armed capture is dropped without a
 *      record.  Without an episode index npb_event_windows_clear(mask) does the same on request (mask: device uint8 [n_plants], NULL = all).
 *   2. ring row s % H takes the recorded columns and the clock; valid = min(valid + 1, H).
 *   3. every trigger is evaluated against prev, then prev = v.  The first sample of an unprimed plant only primes: it never fires.
 *   4. idle and a trigger fired: armed, due = s + post, n_pre = min(pre, valid - 1), and the lowest trigger that fired, the fired set, s
 *      and the clock are kept.  Armed already and a trigger fires: retriggers += 1, nothing else.
 *   5. the capture is taken when s == due; and, with flags bit 0 set and n_post = s - trigger step, when the plant is armed and its episode
 *      ends on this step by the episode kernel's rule (done, or carried length + 1 >= max_episode_steps; autoreset on).  The plant is idle again.
 * Record r (slots are handed out like the episode records': cursor counts every capture, those at or past `capacity` are dropped and
 * counted): plant, episode (the carried index, 0 without one), trigger, step (the trigger's sample number), n_pre, n_post, flags,
 * retriggers int32; fired uint32; time double (prim.sim_time as npb_get_field returns it, at the trigger sample); times double [H] and
 * values double [H][n_cols]: row k is sample step + k - pre, so the trigger sample is row `pre`; rows outside [pre - n_pre, pre + n_post]
 * are NaN in both.  nuclear_sim_amd/eventwin.py states all of this in numpy; the device produces its bits.
 * npb_set_event_windows(h, desc): desc = NULL turns the windows off and frees what the handle allocated (npb_event_windows_bytes: the ring
 * double [H][n_cols + 1][n_plants], prev double [n_triggers][n_plants], and nine 4- or 8-byte words per plant -- the primed flag is
 * valid > 0).  A failed allocation is NPB_EHIP with the byte count in the message, and what was set before stays.  NPB_EINVAL with the
 * reason in npb_last_error, before any device work, for what npb_event_windows_check refuses -- that check alone, without a handle, NULL =
 * accepted, else the reason: counts outside their ranges (columns, triggers, pre, post, H <= NPB_EVENT_WINDOW_ROWS_MAX, capacity >= 1); a
 * bad kind or slot; a side source with a NULL base, an unknown type or rows != 1; BITS_RISE on a real-valued column or with mask 0; an
 * unknown mode; a NaN limit or a direction outside {-1, +1} for BEYOND; a NULL or misaligned record column or cursor (doubles 8-byte, the
 * others 4-byte).  has_autoreset is taken for symmetry with npb_episode_records_check and refuses nothing.
 * Output only: npb_snapshot / npb_restore, the start bank and checkpoints neither read nor write it.  NPB_VERSION stays 154: a binding
 * detects the entry points by name.  A handle that never calls this behaves as before in every entry point. */
#define NPB_EVENT_WINDOW_COLS_MAX 16
#define NPB_EVENT_WINDOW_TRIGGERS_MAX 8
#define NPB_EVENT_WINDOW_ROWS_MAX 1024
enum { NPB_TRIGGER_MODE_BITS_RISE = 0, NPB_TRIGGER_MODE_INCREASE = 1, NPB_TRIGGER_MODE_BEYOND = 2 };
/* the last four members of an npb_event_trigger_t initialiser */
#define NPB_TRIGGER_BITS_RISE(mask) NPB_TRIGGER_MODE_BITS_RISE, (uint32_t)(mask), 0, 0.0
#define NPB_TRIGGER_INCREASE NPB_TRIGGER_MODE_INCREASE, 0u, 0, 0.0
#define NPB_TRIGGER_BEYOND(direction, limit) NPB_TRIGGER_MODE_BEYOND, 0u, (direction), (limit)
typedef struct npb_event_trigger_t {
  int from_source;               /* 0: the arena member (kind, slot); != 0: `source`, one value per plant */
  int kind, slot;
  npb_sample_source_t source;
  int mode; uint32_t mask; int direction; double limit;
} npb_event_trigger_t;
typedef struct npb_event_windows_desc_t {
  int n_fields; const int *kinds; const int *slots;      /* host; arena members, n_fields may be 0 */
  int n_sources; const npb_sample_source_t *sources;     /* host descriptors of one-row device buffers; n_sources may be 0 */
  int n_triggers; const npb_event_trigger_t *triggers;   /* host */
  int pre, post, capacity;
  int32_t *plant, *episode, *trigger, *step, *n_pre, *n_post, *flags, *retriggers;      /* device [capacity] */
  uint32_t *fired;                                       /* device [capacity] */
  double *time;                                          /* device [capacity] */
  double *times;                                         /* device [capacity][H] */
  double *values;                                        /* device [capacity][H][n_cols] */
  uint32_t *cursor;                                      /* device, one word: captures so far */
} npb_event_windows_desc_t;
NPB_API int npb_set_event_windows(NpbHandle *h, const npb_event_windows_desc_t *desc);
NPB_API const char *npb_event_windows_check(const npb_event_windows_desc_t *desc, int n_plants, int has_autoreset);
NPB_API int npb_event_windows_clear(NpbHandle *h, const uint8_t *mask, void *stream);
NPB_API size_t npb_event_windows_bytes(const npb_event_windows_desc_t *desc, int n_plants);

/* Tasks: the caller's own reward and termination rule, formed on the device behind every step -- the one part of an RL or data-generation
 * job that every user defines themselves.  Without a task the episode machinery (npb_set_autoreset, the episode records, the event
 * windows' early captures) ends an episode on the reference's scram pulse or on max_episode_steps and sums the reference's reward; with a
 * task it uses the task's `done` and `reward` columns in place of the step's: an episode can end because the turbine tripped, because a
 * pump's oil level fell through a limit or because a value went non-finite, and a work order can cost something.
 * Columns (npb_task_column_t) are named as npb_event_trigger_t names its column: an arena member (kind, slot), or with from_source != 0 a
 * one-row npb_sample_source_t (an info or obs column, the step's reward / done / trip_flags buffers, a row of the work-order summary, the
 * event-count column), every value widened to double as npb_sample_kernel widens it.
 * Reward terms, 0 .. NPB_TASK_TERMS_MAX, each a column v, a weight w and a kind (ref = the constant `ref`, or with ref_from_column != 0 the
 * sample of ref_column; prev = the same plant's previous sample of the column):
 *   NPB_TASK_VALUE     f = v
 *   NPB_TASK_ABS_ERR   f = fabs(v - ref)
 *   NPB_TASK_SQ_ERR    f = (v - ref) * (v - ref)
 *   NPB_TASK_BEYOND    f = 1.0 if beyond the limit by the statistics' rule (direction +1: v > limit, -1: v < limit), else 0.0
 *   NPB_TASK_EXCESS    f = +1: v > limit ? v - limit : 0.0;  -1: v < limit ? limit - v : 0.0
 *   NPB_TASK_BITS      integer column: f = ((v & mask) != 0) ? 1.0 : 0.0
 *   NPB_TASK_DELTA     f = v - prev; 0.0 on the first sample of an UNPRIMED plant.  A plant is unprimed when the task is set, when the
 *                      handle carries an episode index (npb_set_autoreset) and it differs from the one last seen (the event windows' rule:
 *                      autoreset, npb_restore*, npb_reset*), and after npb_task_clear(mask).  This is how an event count, a work-order
 *                      count of the summary or a maintenance counter gets a price.
 *   reward = bias + w_0 * f_0 + w_1 * f_1 + ... accumulated sequentially in term order, each product rounded before its add (the library
 *   is built with -ffp-contract=off).  A NaN sample gives a NaN reward through VALUE, ABS_ERR, SQ_ERR and DELTA (whatever the weight, 0
 *   included); BEYOND and EXCESS compare, so a NaN sample gives 0.0 there.  The step's own reward is a term like any other -- a source on
 *   the reward buffer given to npb_step -- so "the reference's reward plus extras" is one VALUE term of weight 1.
 * Termination rules, 0 .. NPB_TASK_RULES_MAX, each a column, a mode and a terminal_reward:
 *   NPB_TASK_RULE_BITS_ANY(mask)             integer column: (v & mask) != 0
 *   NPB_TASK_RULE_BEYOND(direction, limit)   beyond the limit, as above
 *   NPB_TASK_RULE_NONFINITE                  !(fabs(v) <= DBL_MAX): a NaN or an infinity
 *   cause = one bit per rule that fired (bit r = rule r), done = cause != 0, and the terminal rewards of the fired rules are added to the
 *   reward behind the terms, in rule order.  Rules are LEVELS, not edges: with the autoreset on the plant restarts on that very step and
 *   the level is gone at the next sample; without it a level keeps reporting done on every step for as long as it holds.  The reference's
 *   scram pulse is the rule BITS_ANY(0xff) on the done buffer given to npb_step; a task without that rule no longer ends episodes on a
 *   scram -- the caller's choice.
 * Outputs, device buffers of the caller's: reward double [n_plants] and done uint8 [n_plants], mandatory; cause uint32 [n_plants] or NULL;
 * terms double [n_terms][n_plants] or NULL: each term's w * f, element [term * n_plants + plant], for reward decomposition.  The handle
 * owns the previous samples of the DELTA terms ([n_delta][n_plants], in term order), a primed flag and the episode index last seen per
 * plant; npb_task_get_state / npb_task_set_state move them to and from host arrays for checkpoints (prev double [n_delta][n_plants] --
 * may be NULL when the task has no DELTA term --, primed int32 [n_plants], seen int32 [n_plants]; synchronous on `stream`; NPB_EINVAL
 * without a task).
 * With a task set npb_step launches ONE more kernel on its stream (npd_task.h; one thread per plant, one wave per 64, no LDS, no atomics):
 * behind the step kernel, the maintenance rule and the work-order summary fold -- a term may read this step's event count and summary
 * rows -- and BEFORE the column-statistics fold, the event-windows kernel, the episode-records kernel and the episode kernel, which are
 * then handed the task's done and reward columns in place of the caller's.  The reward / done buffers given to npb_step still receive
 * exactly what the step kernel writes.  No step, restore or episode kernel changes.
 * npb_set_task(h, desc): desc = NULL turns the task off; the descriptor is copied (its host arrays too), every plant unprimed.  NPB_EINVAL
 * with the reason in npb_last_error, before any device work, for what npb_task_check refuses -- that check alone, without a handle, NULL
 * = accepted, else the reason: n_plants < 1; a term or rule count out of range (or a count without its array); a task with neither terms
 * nor rules; a bad kind or slot; a source with a NULL base, an unknown type or rows != 1; an unknown term kind or rule mode; BITS or
 * BITS_ANY on a real-valued column, or with mask 0; a direction outside {-1, +1} where one is needed; a NaN weight, limit, ref, bias or
 * terminal reward; a NULL reward or done output; a misaligned output (doubles 8-byte, cause 4-byte).  While npb_set_episode_record_task
 * is set npb_set_task (another descriptor, or NULL) is refused.
 * npb_set_episode_record_task(h, cause): why an episode ended, in its record (npb_set_episode_records) -- cause int32 [capacity] on the
 * device takes the ended plant's cause word (its bits) beside the record's other columns.  A descriptor of its own, so that
 * npb_episode_records_desc_t keeps its layout, under the rules of npb_set_episode_record_stats: it needs records and a task both on
 * (NPB_EINVAL otherwise, for a misaligned column, and for a task that keeps no cause column); NULL drops it, and so does EVERY successful
 * npb_set_episode_records.  Off, the records kernel stores exactly what it stored before.
 * NPB_VERSION stays 154: a binding detects the entry points by name.  A handle that never calls this behaves as before in every entry
 * point. */
#define NPB_TASK_TERMS_MAX 16
#define NPB_TASK_RULES_MAX 8
enum { NPB_TASK_VALUE = 0, NPB_TASK_ABS_ERR = 1, NPB_TASK_SQ_ERR = 2, NPB_TASK_BEYOND = 3, NPB_TASK_EXCESS = 4, NPB_TASK_BITS = 5, NPB_TASK_DELTA = 6 };
enum { NPB_TASK_RULE_MODE_BITS_ANY = 0, NPB_TASK_RULE_MODE_BEYOND = 1, NPB_TASK_RULE_MODE_NONFINITE = 2 };
/* the members mode, mask, direction, limit of an npb_task_rule_t initialiser */
#define NPB_TASK_RULE_BITS_ANY(mask) NPB_TASK_RULE_MODE_BITS_ANY, (uint32_t)(mask), 0, 0.0
#define NPB_TASK_RULE_BEYOND(direction, limit) NPB_TASK_RULE_MODE_BEYOND, 0u, (direction), (limit)
#define NPB_TASK_RULE_NONFINITE NPB_TASK_RULE_MODE_NONFINITE, 0u, 0, 0.0
typedef struct npb_task_column_t {
  int from_source;               /* 0: the arena member (kind, slot); != 0: `source`, one value per plant */
  int kind, slot;
  npb_sample_source_t source;
} npb_task_column_t;
typedef struct npb_task_term_t {
  npb_task_column_t column;
  double weight;
  int kind;                      /* NPB_TASK_* */
  int ref_from_column;           /* ABS_ERR, SQ_ERR: 0 = the constant `ref`, != 0 = ref_column */
  double ref;
  npb_task_column_t ref_column;
  int direction; double limit;   /* BEYOND, EXCESS */
  uint32_t mask;                 /* BITS */
} npb_task_term_t;
typedef struct npb_task_rule_t {
  npb_task_column_t column;
  int mode; uint32_t mask; int direction; double limit;
  double terminal_reward;
} npb_task_rule_t;
typedef struct npb_task_desc_t {
  int n_terms; const npb_task_term_t *terms;      /* host */
  int n_rules; const npb_task_rule_t *rules;      /* host */
  double bias;
  double *reward;                /* device [n_plants] */
  uint8_t *done;                 /* device [n_plants] */
  uint32_t *cause;               /* device [n_plants] or NULL */
  double *terms_out;             /* device [n_terms][n_plants] or NULL */
} npb_task_desc_t;
NPB_API int npb_set_task(NpbHandle *h, const npb_task_desc_t *desc);
NPB_API const char *npb_task_check(const npb_task_desc_t *desc, int n_plants);
NPB_API int npb_task_clear(NpbHandle *h, const uint8_t *mask, void *stream);
NPB_API int npb_task_get_state(NpbHandle *h, double *prev, int32_t *primed, int32_t *seen, void *stream);
NPB_API int npb_task_set_state(NpbHandle *h, const double *prev, const int32_t *primed, const int32_t *seen, void *stream);
NPB_API int npb_set_episode_record_task(NpbHandle *h, int32_t *cause /* device [capacity] */);

/* Features: the caller's policy inputs, formed on the device behind every step -- the observation side of the task.  The caller names 1 ..
 * NPB_FEATURES_COLS_MAX columns, each with a transform, and a stack depth K (1 .. NPB_FEATURES_STACK_MAX, K * C <= NPB_FEATURES_CELLS_MAX);
 * the handle keeps `out`, a contiguous row-major [n_plants][K][C] tensor of float (NPB_FEATURES_F32) or double (NPB_FEATURES_F64) of the
 * caller's, holding every plant's last K frames: out[p][K - 1] is the newest frame, out[p][0] the oldest.  No half types.
 * Columns are named as the task names them (npb_task_column_t), every sample v widened to double as npb_sample_kernel widens it.  Kinds:
 *   NPB_FEATURE_AFFINE       y = (v - ref) * scale, ref the constant `ref` or with ref_from_column != 0 the sample of ref_column (a setpoint
 *                            error); the subtraction is rounded before the product (the library is built with -ffp-contract=off)
 *   NPB_FEATURE_BITS(mask)   integer column: y = ((v & mask) != 0) ? 1.0 : 0.0
 * and behind the kind, in this order: if y is a NaN and nan_to is not, y = nan_to (with a NaN nan_to a NaN stays, as THE quiet NaN, sign
 * clear and no payload: 0x7ff8000000000000, as float 0x7fc00000); y = y < lo ? lo : y, then y = y > hi ? hi : y (lo = -inf, hi = +inf: no
 * clip; a NaN passes both comparisons); for float output the narrowing rounds to nearest even, overflows to an infinity and keeps
 * subnormals.
 * A FRESH frame is the frame of a plant whose step outputs do not describe its current state: after a restore or a reset, before any step
 * of the new episode.  In a fresh frame an arena member is read live, and so is a source with fresh_live != 0 (the obs buffer given to
 * npb_step, which the episode kernel rewrites for a restarted plant); every other source takes its raw value `fresh` (for a ref_column
 * without ref_fresh_live: the constant `ref`), which then goes through the same transform.  That makes the restart frame well defined
 * although reward, info and trip_flags keep describing the terminal transition (npb_set_autoreset).
 * The handle keeps per plant a primed flag and the episode index last seen (the task's rule).  With features set npb_step launches one
 * kernel more, or with the autoreset on two (npd_features.h; one wave per 64 plants, the frame transposed through LDS, no atomics):
 *   pass A, behind the event-windows kernel and before the episode-records and episode kernels: a primed plant whose episode index is the
 *     one seen shifts its stack by one frame and appends this step's frame, all columns live; an unprimed plant, or one whose index
 *     differs (restored by the caller between steps), has all K slots filled with this step's frame.  Both: primed = 1, seen = index.
 *   pass B, behind the episode kernel, only with the autoreset on: a plant whose carried episode index now differs from `seen` was
 *     restarted on this step.  With a `final` buffer ([n_plants][K][C], the type of out) its whole stack -- the terminal frame pass A just
 *     appended included -- is first copied to final[p]; the rows of the other plants stay as they were (as final_obs).  Then all K slots
 *     take the fresh frame of the restored state, and seen = index.
 * npb_features_prime: the unprimed plants get all K slots filled with the fresh frame of their current state and become primed; primed
 * plants are untouched -- the initial observation before the first step, and the observation after a reset.  npb_features_clear: the
 * plants of mask (device uint8 [n_plants], NULL = all) become unprimed.  npb_features_get_state / npb_features_set_state move primed and
 * seen (int32 [n_plants] each) to and from host arrays for checkpoints, synchronous on `stream`; the stack itself is the caller's buffer.
 * These four return NPB_EINVAL when no features are set.
 * npb_set_features(h, desc): desc = NULL turns the features off; the descriptor is copied (its host array too), every plant unprimed.
 * NPB_EINVAL with the reason in npb_last_error, before any device work, for what npb_features_check refuses -- that check alone, without a
 * handle, NULL = accepted, else the reason: n_plants < 1; a column count or stack depth out of range (or a count without its array), or K
 * * C > NPB_FEATURES_CELLS_MAX; a bad kind or slot; a source with a NULL base, an unknown type or rows != 1; an unknown feature kind;
 * BITS on a real-valued column, or with mask 0; a NaN scale, ref, lo, hi or fresh; lo > hi; an unknown out type; a NULL or misaligned
 * out, or a misaligned final (4-byte for float, 8-byte for double).
 * No step, restore or episode kernel changes.  Not here: the terminal stack in the episode records, half-precision output, a delta or rate
 * kind (the stack carries it).  Running statistics updated on the device have the normaliser's section below (npb_set_normalizer), which
 * rewrites `ref` and `scale` of the columns it is given in front of pass A.
 * NPB_VERSION stays 154: a binding detects the entry points by name.  A handle that never calls this behaves as before in every entry
 * point. */
#define NPB_FEATURES_COLS_MAX 64
#define NPB_FEATURES_STACK_MAX 16
#define NPB_FEATURES_CELLS_MAX 256
enum { NPB_FEATURE_KIND_AFFINE = 0, NPB_FEATURE_KIND_BITS = 1 };
enum { NPB_FEATURES_F32 = 0, NPB_FEATURES_F64 = 1 };
/* the members kind, mask of an npb_feature_column_t initialiser */
#define NPB_FEATURE_AFFINE NPB_FEATURE_KIND_AFFINE, 0u
#define NPB_FEATURE_BITS(mask) NPB_FEATURE_KIND_BITS, (uint32_t)(mask)
typedef struct npb_feature_column_t {
  npb_task_column_t column;
  int kind; uint32_t mask;       /* NPB_FEATURE_AFFINE, or NPB_FEATURE_BITS(mask) */
  double scale;                  /* AFFINE */
  int ref_from_column;           /* AFFINE: 0 = the constant `ref`, != 0 = ref_column */
  double ref;
  npb_task_column_t ref_column;
  double lo, hi;                 /* the clip; -inf / +inf = none */
  double nan_to;                 /* what a NaN becomes; a NaN = it stays */
  double fresh;                  /* a source's raw value in a fresh frame */
  int fresh_live, ref_fresh_live; /* != 0: the source is current after a restore and is read in a fresh frame too */
} npb_feature_column_t;
typedef struct npb_features_desc_t {
  int n_columns; const npb_feature_column_t *columns;      /* host */
  int stack;                     /* K */
  int out_type;                  /* NPB_FEATURES_F32 | NPB_FEATURES_F64 */
  void *out;                     /* device [n_plants][stack][n_columns] */
  void *final;                   /* device, the same shape, or NULL */
} npb_features_desc_t;
NPB_API int npb_set_features(NpbHandle *h, const npb_features_desc_t *desc);
NPB_API const char *npb_features_check(const npb_features_desc_t *desc, int n_plants);
NPB_API int npb_features_prime(NpbHandle *h, void *stream);
NPB_API int npb_features_clear(NpbHandle *h, const uint8_t *mask, void *stream);
NPB_API int npb_features_get_state(NpbHandle *h, int32_t *primed, int32_t *seen, void *stream);
NPB_API int npb_features_set_state(NpbHandle *h, const int32_t *primed, const int32_t *seen, void *stream);

/* Controls: the caller's policy outputs, decoded on the device in front of every step -- the action side of the task and the features.
 * The caller names 1 .. NPB_CONTROLS_AXES_MAX axes; axis a reads element [p][a] of `in`, a contiguous row-major [n_plants][n_axes] tensor
 * of float (NPB_CONTROLS_F32) or double (NPB_CONTROLS_F64) of the caller's, bound once.  No half types.  With controls set npb_step launches
 * one kernel more (npd_controls.h; one wave per 64 plants, the wave's rows loaded with unit stride and transposed through LDS, no atomics),
 * after the episode streams have taken their rows and in front of the step kernel.
 * The transform of an element x, widened to double, every step rounded on its own (the library is built with -ffp-contract=off):
 *   1. a NaN x becomes nan_to (finite);  2. y = x * scale + offset;  3. y = y < lo ? lo : y, then y = y > hi ? hi : y;
 *   4. NPB_CONTROL_RATE only: fabs(y) < deadband gives y = 0.0 (fabs(y) == deadband stays).
 * The kinds:
 *   NPB_CONTROL_RATE(actuator)   actuator one of NPB_ACTUATOR_ROD, _FLOW, _VALVE, _BORON.  y is a signed magnitude: y > 0 is the
 *       reference's move with the actuator's increasing ControlAction code (1, 2, 4, 10) at magnitude y, y < 0 the decreasing code (0, 3,
 *       5, 9) at -y, y == 0 nothing.  The usual clip is [-1, 1].
 *   NPB_CONTROL_TARGET(actuator) y is a position in the member's own units; the move is the reference's move at magnitude max_magnitude,
 *       stopped at the target: with pos the member now, y > pos gives new = min(up, y), up what the increasing code at max_magnitude
 *       makes of pos; y < pos gives new = max(down, y); y == pos nothing.  The actuator's range limit comes with up and down.
 *   NPB_CONTROL_COLUMN(input)    input NPB_CONTROL_INPUT_POWER_SETPOINT or NPB_CONTROL_INPUT_COOLING_WATER_TEMP: y goes into a column
 *       [n_plants] of the handle's, which npb_step hands to the step kernel as that input (the step's own setpoint clip still applies).
 *   NPB_CONTROL_VALUE            y moves nothing and fills nothing: it is held like every axis, for the task, the features, the
 *       statistics and the windows to read (a policy output the plant does not take but the reward prices).  With four actuators and two
 *       inputs, each named at most once, these are what brings an input tensor to more than six columns.
 * Both actuator kinds call the step's own npd_apply_control_actions: the rate expressions and the range limits are stated once.  Each
 * actuator and each input may be named by at most one axis.
 * Moving the actuators in front of the step is the same physics as the step's own action: control_rod_position, coolant_flow_rate,
 * steam_valve_position and boron_concentration are read only inside the primary update, behind its call of npd_apply_control_actions,
 * and in the observation at the end of the step; "move here, then step with NO_ACTION" is bit for bit "step with that action" (fp64
 * storage; under fp32 storage the moved member is rounded to float at the store here, as npb_set_field rounds it).  The maintenance
 * screen's cooldown cache watches the feedwater pumps' parameters, none of these four, and stays valid.  The caller may still pass
 * action and magnitude to npb_step: the step kernel applies them behind the controls, as it always did.
 * A lane stores only the members an axis changed, where the new bits differ from the old: a plant whose actuators do not move keeps its
 * exact bits under either storage type.
 * The hold: interval = K, 1 .. NPB_CONTROLS_INTERVAL_MAX.  Per plant the handle keeps age, primed and seen (int32 [n_plants]) and works on
 * `held` and `prev` (double [n_axes][n_plants], device memory of the caller's like `in`, so that a task, features, statistics or windows
 * can name a row of them as a side source).  A plant is unprimed when the controls are set, after npb_controls_clear(mask) and when the
 * handle carries an episode index that differs from `seen` (the task's rule; this kernel runs before the step, so it sees the index the
 * previous step's episode kernel left: the first step of a new episode starts a new hold).  Each step and plant: unprimed gives age = 0;
 * if age % K == 0 the row is read and transformed, prev = held (for an unprimed plant prev = the new y), held = y; otherwise the row is
 * not read and held is applied again (a held TARGET keeps moving towards its target, a held RATE repeats its move); then age += 1,
 * primed = 1, seen = index.
 * npb_controls_clear: the plants of mask (device uint8 [n_plants], NULL = all) become unprimed.  npb_controls_get_state /
 * npb_controls_set_state move held, prev ([n_axes][n_plants]), age, primed and seen to and from host arrays, synchronous on `stream`.
 * These return NPB_EINVAL when no controls are set.
 * npb_set_controls(h, desc): desc = NULL turns the controls off; the descriptor is copied, every plant unprimed.  NPB_EINVAL with the
 * reason in npb_last_error, before any device work, for what npb_controls_check refuses -- that check alone, without a handle, NULL =
 * accepted, else the reason: n_plants < 1; an axis count or interval out of range, or a count without its array; an unknown kind,
 * actuator or input; two axes on one target; a NaN or infinite scale, offset, nan_to, deadband or max_magnitude; deadband < 0 or
 * max_magnitude < 0; a NaN lo or hi, or lo > hi; an unknown input type; a NULL or misaligned in (4-byte for float, 8-byte for double),
 * held or prev; a POWER_SETPOINT axis under NPB_HEAT_EXTERNAL, where the column carries the plugin's power -- and on the handle a
 * POWER_SETPOINT axis while episode streams drive the profile (likewise npb_set_episode_streams with a profile while such an axis is set).
 * npb_step refuses a non-NULL caller column for an input an axis fills, naming the axis.
 * No step, restore, episode, task or features kernel changes.  Not here: a discrete action table, a rate limit on the COLUMN kind
 * (npb_profile_ramp), half-precision input, the feedwater action codes (the reference accepts them and they do nothing), K steps in
 * one call.
 * (A maintenance order needs no action table: it is a thresholded VALUE axis, npb_set_control_orders below.)
 * (The policy's section below, npb_set_policy, writes `in` on the device, and its npb_collect runs K steps in one call.)
 * NPB_VERSION stays 154: a binding detects the entry points by name.  A handle that never calls this behaves as before in every entry
 * point. */
#define NPB_CONTROLS_AXES_MAX 8
#define NPB_CONTROLS_INTERVAL_MAX 64
enum { NPB_CONTROL_KIND_RATE = 0, NPB_CONTROL_KIND_TARGET = 1, NPB_CONTROL_KIND_COLUMN = 2, NPB_CONTROL_KIND_VALUE = 3 };
enum { NPB_ACTUATOR_ROD = 0, NPB_ACTUATOR_FLOW = 1, NPB_ACTUATOR_VALVE = 2, NPB_ACTUATOR_BORON = 3, NPB_ACTUATOR_COUNT = 4 };
enum { NPB_CONTROL_INPUT_POWER_SETPOINT = 0, NPB_CONTROL_INPUT_COOLING_WATER_TEMP = 1, NPB_CONTROL_INPUT_COUNT = 2 };
enum { NPB_CONTROLS_F32 = 0, NPB_CONTROLS_F64 = 1 };
/* the members kind, target of an npb_control_axis_t initialiser */
#define NPB_CONTROL_RATE(actuator) NPB_CONTROL_KIND_RATE, (actuator)
#define NPB_CONTROL_TARGET(actuator) NPB_CONTROL_KIND_TARGET, (actuator)
#define NPB_CONTROL_COLUMN(input) NPB_CONTROL_KIND_COLUMN, (input)
#define NPB_CONTROL_VALUE NPB_CONTROL_KIND_VALUE, 0
typedef struct npb_control_axis_t {
  int kind, target;              /* NPB_CONTROL_RATE(actuator), NPB_CONTROL_TARGET(actuator), NPB_CONTROL_COLUMN(input) or NPB_CONTROL_VALUE */
  double scale, offset;          /* y = x * scale + offset */
  double lo, hi;                 /* the clip; -inf / +inf = none */
  double nan_to;                 /* what a NaN x becomes; finite */
  double deadband;               /* RATE: fabs(y) < deadband gives 0; >= 0 */
  double max_magnitude;          /* TARGET: the magnitude of one step's move; >= 0 */
} npb_control_axis_t;
typedef struct npb_controls_desc_t {
  int n_axes; const npb_control_axis_t *axes;      /* host */
  int interval;                  /* K */
  int in_type;                   /* NPB_CONTROLS_F32 | NPB_CONTROLS_F64 */
  const void *in;                /* device [n_plants][n_axes] */
  double *held, *prev;           /* device [n_axes][n_plants] each */
} npb_controls_desc_t;
NPB_API int npb_set_controls(NpbHandle *h, const npb_controls_desc_t *desc);
NPB_API const char *npb_controls_check(const npb_controls_desc_t *desc, int n_plants, int heat_source);
NPB_API int npb_controls_clear(NpbHandle *h, const uint8_t *mask, void *stream);
NPB_API int npb_controls_get_state(NpbHandle *h, double *held, double *prev, int32_t *age, int32_t *primed, int32_t *seen, void *stream);
NPB_API int npb_controls_set_state(NpbHandle *h, const double *held, const double *prev, const int32_t *age, const int32_t *primed,
                                   const int32_t *seen, void *stream);

/* Order rules on the controls' axes: how a policy orders maintenance.  A policy output on an NPB_CONTROL_VALUE axis is decoded and held
 * and moves nothing; an order rule says what service happens when that held value is positive enough.  npb_set_control_orders(h, desc)
 * attaches 1 .. NPB_CONTROL_ORDERS_MAX rules to a handle whose controls are set.  Rule r:
 *   axis          an axis of kind NPB_CONTROL_VALUE; several rules may share one
 *   family        NPB_ORDER_PUMP (npb_perform_maintenance), NPB_ORDER_COMPONENT (npb_perform_component_maintenance) or NPB_ORDER_TURBINE
 *                 (npb_perform_turbine_maintenance)
 *   action        the catalog index of that family (NPB_MA_*, NPB_CA_*, NPB_TA_*; include/npb_maint.h)
 *   unit          pump 0..3; generator 0..2 or ejector 0..1; bearing 0..3 or stage 0..13; ignored where the family's call ignores it
 *   option        NPB_BEARING_* for a pump's bearing replacement, NPB_CLEANING_* for the component family, else 0
 *   amount        the pump family's target_level (95.0 is the call's default) or the component family's tubes_to_plug
 *   threshold     a finite double
 *   min_interval  >= 1: the steps from one firing of the rule on a plant to the next at the earliest
 * With rules set npb_step (and so npb_collect) launches one kernel more (npd_control_orders.h; one wave per 64 plants, no LDS, no atomics
 * beyond the maintenance log's slot hand-out), behind the controls kernel and in front of the step kernel.  For plant p let latch be
 * "the controls read p's row on this step" and restart "the controls found p unprimed on this step" (above: a new episode index,
 * npb_controls_clear, a fresh npb_set_controls; the Python layer's reset / restore / restore_from_bank clear the controls of the plants
 * they restart): the orders follow exactly the plants the hold follows, and keep no restart words of their own.  With NEVER = INT32_MAX,
 * for r ascending:
 *   c = restart ? NEVER : since[r][p];   y = held[axis_r][p];
 *   fire = latch && y > threshold_r && (c == NEVER || c >= min_interval_r);
 *   since[r][p] = fire ? 1 : (c == NEVER ? NEVER : c + 1), saturating below NEVER;   fired[r][p] = fire ? 1.0 : 0.0
 * A held row orders once, on the step it was read, not K times; a NaN output never fires, because nan_to is finite.  Where fire holds
 * the plant gets what the family's npb_perform_* call does for (action, unit, option, amount), rule r + 1 seeing what rule r left: by
 * bits the kernel is "for r: npb_perform_<family>(action_r, unit_r, ..., masked by fire[r])", under either storage type; with a
 * maintenance log set it appends the NPB_MAINT_EVENT_OPERATOR* records those calls append, and the summary is folded behind it.  A plant
 * on which nothing fires has nothing stored to it.  The work-order queue, the maint.* / mpump.* sections, the counters and the cooldown
 * cache are untouched, for the reason npb_perform_maintenance gives.
 * fired: the caller's device double [n_orders][n_plants], like held: a side buffer a task, features, statistics or windows can name a
 * row of -- how an order gets a price, becomes a policy input and triggers a window.
 * A rule that cannot succeed on this handle is refused at set time, so at run time fire means success.  npb_control_orders_check(desc,
 * controls_desc, n_plants, mode) -- without a handle, NULL = accepted, else the reason: n_plants < 1; no controls descriptor; a rule
 * count out of range or without its array; an axis that is none or not VALUE; an unknown family; an action outside the catalog; a pump
 * action without a handler; a unit that does not exist; a thrust adjustment on a journal bearing; a bearing (option of a pump's bearing
 * replacement) outside NPB_BEARING_ALL .. _THRUST; a component or a turbine the mode does not step; a NaN or infinite threshold or
 * amount; min_interval < 1; a NULL or misaligned fired.
 * npb_set_control_orders: desc = NULL drops the rules; NPB_EINVAL without controls and for what the check refuses, and while a policy is
 * set (the message of npb_set_controls).  npb_set_controls, with NULL or a new descriptor, drops the rules.  Every since starts at NEVER.
 * npb_control_orders_get_state / _set_state move since (int32 [n_orders][n_plants]) to and from a host array, synchronous on `stream`;
 * NPB_EINVAL when no rules are set.
 * Not here: a categorical or Bernoulli head, queued (delayed, counted) work orders, per-plant rule parameters, rules on RATE, TARGET or
 * COLUMN axes, durations or outages of a service, the turbine's automatic maintenance.
 * NPB_VERSION stays 154: a binding detects the entry points by name.  A handle that never calls this behaves as before in every entry
 * point. */
#define NPB_CONTROL_ORDERS_MAX 8
#define NPB_CONTROL_ORDER_NEVER 0x7fffffff
enum { NPB_ORDER_PUMP = 0, NPB_ORDER_COMPONENT = 1, NPB_ORDER_TURBINE = 2, NPB_ORDER_NFAMILY = 3 };
typedef struct npb_control_order_t {
  int axis, family, action, unit, option;
  int min_interval;
  double amount, threshold;
} npb_control_order_t;
typedef struct npb_control_orders_desc_t {
  int n_orders; const npb_control_order_t *orders;      /* host */
  double *fired;                 /* device [n_orders][n_plants] */
} npb_control_orders_desc_t;
NPB_API int npb_set_control_orders(NpbHandle *h, const npb_control_orders_desc_t *desc);
NPB_API const char *npb_control_orders_check(const npb_control_orders_desc_t *desc, const npb_controls_desc_t *controls, int n_plants, int mode);
NPB_API int npb_control_orders_get_state(NpbHandle *h, int32_t *since, void *stream);
NPB_API int npb_control_orders_set_state(NpbHandle *h, const int32_t *since, void *stream);

/* The rollout: the learner's half of the loop, written down on the device -- what the policy saw (the features), what it did (the
 * controls' input and up to NPB_ROLLOUT_EXTRAS_MAX floats of its own per plant: value, log-probability, ...), what came of it (reward, how
 * the episode went on) for a horizon of T steps, and from that the GAE advantages and returns in one launch.  The rollout needs features
 * to be set; controls are optional.  Opt-in: a handle that never sets a rollout behaves as before in every entry point.
 * npb_set_rollout(h, desc) binds caller-owned device buffers, contiguous and time-major, slot t first, for 1 <= T <= NPB_ROLLOUT_HORIZON_MAX:
 *   obs        [T][n][K][C]   the features' out type   the features tensor as the policy saw it in front of step t
 *   act        [T][n][A]      the controls' in type    the bound controls input as the policy wrote it; NULL (and A = 0) without controls
 *   extra      [T][n][E]      float                    a copy of extras_in, a bound [n][E] input the caller writes before each step, E = 0 ..
 *                                                      NPB_ROLLOUT_EXTRAS_MAX (E = 0: both NULL)
 *   reward     [T][n]         double                   the reward the episode kernel sums: the task's while a task is set, else the step's
 *   ended      [T][n]         uint8                    bit 0 (NPB_ROLLOUT_TERMINATED), bit 1 (NPB_ROLLOUT_TRUNCATED), bit 2 (NPB_ROLLOUT_CUT)
 *   episode    [T][n]         int32                    the carried index of the episode the transition belonged to; -1 without autoreset
 *   final_row  [T][n]         int32                    a row of final_obs, or -1
 *   final_obs  [n * R][K][C]  the features' out type   the terminal stack of each truncated transition; NULL with R = 0
 * The handle keeps a host cursor t, the number of slots recorded (npb_rollout_steps), and a device int32 n_final[n], the rows of final_obs
 * each plant has taken.  npb_rollout_begin(h, stream): t = 0, n_final zeroed, final_row filled with -1.  npb_set_rollout begins too.
 * With a rollout set npb_step launches two kernels more (npd_rollout.h); neither touches the arena:
 *   pre, in front of the controls kernel: three contiguous copies into slot t in one launch, the features' out -> obs[t], the controls' in
 *     -> act[t], extras_in -> extra[t]; 16 bytes per lane where source and slot are 16-byte aligned.
 *   post, behind features pass A and in front of the episode-records and episode kernels, one lane per plant: there the features' out[p]
 *     IS the stack with the terminal frame appended, and the carried length is still the old one.  The outcome is decided as the episode
 *     kernel decides it behind this kernel on the same columns: terminated = done[p] != 0; truncated = max_episode_steps > 0 && len[p] + 1
 *     >= max_episode_steps && !terminated (termination wins); without autoreset only bit 0 can be set.  reward[t][p], ended[t][p] and
 *     episode[t][p] are written.  A truncated plant takes row p * R + n_final[p] of final_obs, n_final[p] += 1, final_row[t][p] = that row,
 *     and the wave copies the plant's K * C cells of out[p] to the row, all lanes on one row, 16 bytes per lane where K * C allows.
 *     No atomics: the row assignment is deterministic.  The terminal stacks of TERMINATED transitions are not stored: their bootstrap is 0.
 *   The host then bumps t.  npb_step at t == T is refused (NPB_EINVAL, before any launch; the rollout does not wrap silently:
 *   npb_rollout_begin rewinds it), and so is a NULL reward or done column while a rollout is set.
 * R is derived, not tuned: truncations of one plant are at least max_episode_steps steps apart and the first can fall on slot 0, so R >=
 * ceil(T / max_episode_steps) suffices; npb_step refuses (NPB_EINVAL) a smaller R while the autoreset has max_episode_steps > 0; R = 0
 * with final_obs NULL is valid when no truncation can happen.  (A plant that still runs out of rows -- the limit was lowered while the
 * rollout was recording -- takes none: final_row stays -1 and its bootstrap is 0.  npb_rollout_begin after such a change.)
 * npb_rollout_cut(h, mask, stream): a restart the caller makes between two recorded steps (npb_reset, npb_restore, npb_restore_bank).  With
 * t > 0 the plants of mask (device uint8 [n_plants], NULL = all) get bit 2 set in ended[t - 1]; with t == 0 nothing happens.
 * npb_rollout_advantages(h, desc, stream): one launch over the slots [0, t), one lane per plant, backwards over the slots, every access
 * consecutive along n.  In double, every operation rounded on its own (the library is built with -ffp-contract=off):
 *   gl    = gamma * lam                                   (once, on the host)
 *   v     = value ? (double)value[t][p] : 0.0
 *   nv    = (ended & 5) ? 0.0                             terminated or cut: no bootstrap
 *         : (ended & 2) ? (final_row[t][p] >= 0 ? (double)final_value[final_row[t][p]] : 0.0)      truncated: the value of the TERMINAL state
 *         : t == t_end - 1 ? (last_value ? (double)last_value[p] : 0.0)
 *         : value ? (double)value[t + 1][p] : 0.0
 *   delta = (reward[t][p] + gamma * nv) - v
 *   carry = (ended & 7) ? 0.0 : A[t + 1][p]               (0.0 behind the last slot)
 *   A     = delta + gl * carry
 *   ret   = A + v
 * carry is a select, not a product with 1 - done: a NaN in one episode never reaches the episode in front of it.  value is float, given as
 * base + time stride + plant stride in elements, so a column of `extra` serves in place; last_value is float [n], final_value float [n * R]:
 * the caller's value of final_obs.  adv and ret are [T][n], float (NPB_ROLLOUT_F32) or double (NPB_ROLLOUT_F64); either may be NULL; the
 * narrowing rounds to nearest even, as the features' does.  With lam = 1 and no values ret is the discounted return-to-go.
 * nuclear_sim_amd/rollout.py states all of it in numpy, and that statement is the contract: the recurrence is not restated as a scan.
 * NPB_EINVAL: no rollout set; t == 0; final_value NULL while R > 0; gamma or lam a NaN or outside [0, 1]; adv and ret both NULL; an
 * unknown out type.
 * npb_set_rollout(h, NULL) turns the rollout off; npb_destroy drops it.  While a rollout is set npb_set_features and npb_set_controls are
 * refused, set and NULL alike, naming the rollout: they would free or reshape what the pre kernel copies.  NPB_EINVAL with the reason in
 * npb_last_error, before any device work: no features set, and what npb_rollout_check refuses -- that check alone, without a handle
 * (features_cells = K * C, n_axes = the controls' axis count or 0), NULL = accepted, else the reason: n_plants < 1 or features_cells < 1;
 * T or E out of range; an act buffer without axes, or axes without an act buffer; R < 0, or n_plants * R beyond int32; final_obs NULL with R > 0; a NULL obs, reward,
 * ended, episode or final_row; E > 0 without extras_in or extra; a misaligned buffer (16 bytes for obs, act, extras_in, extra and
 * final_obs, 8 for reward, 4 for episode and final_row).
 * No step, restore, episode, task, features or controls kernel changes.  Not here: advantage normalisation and minibatch shuffling (they
 * have the section below, where the reduction order is pinned: npb_rollout_moments, npb_rollout_minibatch),
 * a checkpoint of a half-filled rollout, half types, V-trace or other off-policy corrections, rollouts without features.
 * (The values the advantages wait for, and the extras a policy writes by itself, have the policy's section below: npb_set_policy.)
 * NPB_VERSION stays 154: a binding detects the entry points by name. */
#define NPB_ROLLOUT_HORIZON_MAX 4096
#define NPB_ROLLOUT_EXTRAS_MAX 8
enum { NPB_ROLLOUT_TERMINATED = 1, NPB_ROLLOUT_TRUNCATED = 2, NPB_ROLLOUT_CUT = 4 };
enum { NPB_ROLLOUT_F32 = 0, NPB_ROLLOUT_F64 = 1 };
typedef struct npb_rollout_desc_t {
  int horizon;                   /* T */
  int n_extras;                  /* E */
  int final_rows;                /* R */
  const float *extras_in;        /* device [n_plants][E], or NULL with E = 0 */
  void *obs;                     /* device [T][n_plants][K][C] */
  void *act;                     /* device [T][n_plants][A], or NULL without controls */
  float *extra;                  /* device [T][n_plants][E], or NULL with E = 0 */
  double *reward;                /* device [T][n_plants] */
  uint8_t *ended;                /* device [T][n_plants] */
  int32_t *episode, *final_row;  /* device [T][n_plants] each */
  void *final_obs;               /* device [n_plants * R][K][C], or NULL with R = 0 */
} npb_rollout_desc_t;
typedef struct npb_rollout_advantages_desc_t {
  double gamma, lam;
  const float *value;            /* device, or NULL: value[t][p] = value[t * value_time_stride + p * value_plant_stride] */
  int64_t value_time_stride, value_plant_stride;      /* in elements */
  const float *last_value;       /* device [n_plants], or NULL */
  const float *final_value;      /* device [n_plants * R]; NULL only with R = 0 */
  int out_type;                  /* NPB_ROLLOUT_F32 | NPB_ROLLOUT_F64 */
  void *adv, *ret;               /* device [T][n_plants] each; one of them may be NULL */
} npb_rollout_advantages_desc_t;
NPB_API int npb_set_rollout(NpbHandle *h, const npb_rollout_desc_t *desc);
NPB_API const char *npb_rollout_check(const npb_rollout_desc_t *desc, int n_plants, int features_cells, int n_axes);
NPB_API int npb_rollout_begin(NpbHandle *h, void *stream);
NPB_API int npb_rollout_steps(const NpbHandle *h);      /* t, or -1 without a rollout */
NPB_API int npb_rollout_cut(NpbHandle *h, const uint8_t *mask, void *stream);
NPB_API int npb_rollout_advantages(NpbHandle *h, const npb_rollout_advantages_desc_t *desc, void *stream);

/* Between the advantages and the optimiser: what a PPO-style learner does with a finished rollout -- the advantages' mean and standard
 * deviation, a shuffled order, and the gather of one minibatch after the other -- on the device, with nothing read back.
 * nuclear_sim_amd/rollout.py (moments, permutation_keys, permutation, minibatch) states all of it in numpy, and that statement is the
 * contract; the device produces its bits whatever the launch geometry.  No kernel here touches the arena, uses atomics or depends on the
 * launch order; they are built without -freciprocal-math / -fapprox-func (npb_minibatch.hip): division and root are IEEE.
 * npb_rollout_moments(h, desc, stream): out = {count, mean, var, std} of src, a contiguous device [rows][cols] float or double tensor --
 *   any such tensor, no rollout need be set.  The order of every addition is pinned:
 *     col[p]  = 0.0, then col[p] += (double)src[s][p] for s = 0 .. rows - 1 in that order
 *     tree(c) : while c has more than one value: pad it with +0.0 to a multiple of 256, and in each group of 256 add the upper half onto
 *               the lower for half = 128, 64, ... 1; the groups' first values are the next c.  Its one value is the result.
 *     count   = rows * cols;  mean = tree(col) / count
 *     col2[p] += d * d with d = (double)src[s][p] - mean, the product rounded before the sum;  var = tree(col2) / (count - ddof)
 *     std     = sqrt(var)
 *   the sum is not restated as a scan or a different tree.  A NaN or an infinity propagates.  Four launches: a column pass with one lane
 *   per column whose workgroup of 256 evaluates one group of the tree in LDS and writes one partial, and one workgroup that finishes the
 *   tree over the partials, divides and (second pass) takes the root -- twice.  The partials live in a workspace of the handle's, grown
 *   on demand and dropped by npb_destroy.  NPB_EINVAL: a NULL descriptor, src or out; an unknown type; rows or cols < 1, cols beyond
 *   2^31 - 1, rows * cols beyond 2^53; ddof < 0 or rows * cols <= ddof; src misaligned for its type or out not 8-byte aligned.
 * npb_rollout_permutation(h, N, keys, first, count, out, stream): out[j] = entry first + j of a permutation of [0, N), 1 <= N <= 2^31 - 1,
 *   each entry a function of its position and the NPB_MINIBATCH_ROUNDS round keys alone -- no table, no sort, no memory:
 *     b = max(bit_length(N - 1), 2);  w = (b + 1) / 2;  x = position: L = x >> w, R = x & (2^w - 1)
 *     for r = 0 .. 5: (L, R) = (R, L ^ (mix(R ^ keys[r]) & (2^w - 1)))      mix: murmur3's 32-bit finaliser, in uint32 arithmetic
 *     x = L << w | R;  while x >= N the network is applied to x again (cycle walking)
 *   The network is a bijection on [0, 2^(2w)), so the walk is one on [0, N), and it ends: the walk from a position below N stays on that
 *   position's cycle.  2^(2w) < 4 N: under 4 applications in the mean.  One lane per entry.  The caller derives the keys from its seed
 *   and epoch (rollout.permutation_keys: a splitmix64 chain).  NPB_EINVAL: N out of range, count < 1, first < 0 or first + count > N, NULL
 *   keys or out, out not 4-byte aligned.
 * npb_rollout_minibatch(h, desc, stream): entries [first, first + count) of the epoch `keys` belong to, gathered from the handle's rollout
 *   -- sources and shapes (the recorded slots t, n, K * C, A, E, the types) are the rollout's -- in ONE launch:
 *   unit NPB_MINIBATCH_TRANSITION: N = t * n; index[j] = permutation(N)[first + j], the flat cell s * n + p; obs [count][K][C], act
 *     [count][A], extra [count][E], adv_out, ret_out [count] are that cell's rows of obs, act, extra, adv, ret.
 *   unit NPB_MINIBATCH_PLANT (recurrent policies: sequences kept whole): N = n; index[j] is a plant; every output is time-major,
 *     [t][count]... = src[s][index[j]] for every s < t.
 *   adv, ret: device [>= t][n] of `type`, as npb_rollout_advantages wrote them.  With moments (device, what npb_rollout_moments wrote)
 *     adv_out = narrow(((double)adv - moments[1]) / (moments[3] + eps)): one subtraction, one addition, one IEEE division in double, then
 *     one narrowing to `type`, round-to-nearest-even.  Without, adv is copied.  Any output but index may be NULL.
 *   A wave takes 32 output rows: one lane per row computes its source index and writes index, adv_out and ret_out, consecutive lanes on
 *   consecutive outputs; then the wave walks its rows, L lanes on each -- L the smallest power of two with L * 16 bytes >= the row, at
 *   most 64 --, 16 bytes per lane where the row is a whole number of 16-byte pieces, else one element per lane.  max_blocks: the most
 *   workgroups the launch may have (0: the launcher's own bound); the result does not depend on it.
 *   NPB_EINVAL with the reason in npb_last_error, before any device work: no rollout set, and what npb_minibatch_check refuses -- that
 *   check alone, without a handle (t = the recorded slots, features_cells = K * C), NULL = accepted, else the reason: a NULL descriptor;
 *   n_plants < 1 or features_cells < 1; t == 0 (nothing recorded); an unknown unit or type; N beyond 2^31 - 1; count < 1; first < 0 or
 *   first + count > N; index NULL; an act / extra output without axes / extras; adv_out without adv, ret_out without ret; moments set
 *   with adv_out NULL; eps negative or a NaN; max_blocks < 0; a misaligned buffer (16 bytes for the obs, act and extra outputs, 8 for
 *   moments, the element size for adv, ret and their outputs, 4 for index).
 * A handle that never calls these behaves as before in every entry point.  Not here: half or bfloat16 outputs, weighted or prioritised
 * sampling, sampling with replacement, masks over transitions, a checkpoint of a half-drained epoch (the epoch IS (seed, epoch, first):
 * three numbers the caller has), V-trace, gathering final_obs (its use ended in npb_rollout_advantages).  Running normalisation across
 * rollouts has the normaliser's section below (npb_set_normalizer), which shares this section's tree.  NPB_VERSION stays 154: a binding
 * detects the entry points by name. */
#define NPB_MINIBATCH_ROUNDS 6
enum { NPB_MINIBATCH_TRANSITION = 0, NPB_MINIBATCH_PLANT = 1, NPB_MINIBATCH_SEGMENT = 2 /* npb_rollout_minibatch_segments alone */ };
typedef struct npb_moments_desc_t {
  const void *src;               /* device [rows][cols], contiguous */
  int type;                      /* NPB_ROLLOUT_F32 | NPB_ROLLOUT_F64 */
  int ddof;
  int64_t rows, cols;
  double *out;                   /* device [4]: count, mean, var, std */
} npb_moments_desc_t;
typedef struct npb_minibatch_desc_t {
  int unit;                      /* NPB_MINIBATCH_TRANSITION | NPB_MINIBATCH_PLANT */
  uint32_t keys[NPB_MINIBATCH_ROUNDS];
  int type;                      /* of adv, ret, adv_out and ret_out: NPB_ROLLOUT_F32 | NPB_ROLLOUT_F64 */
  int64_t first, count;          /* entries [first, first + count) of the permutation */
  const void *adv, *ret;         /* device [>= t][n_plants]; NULL only where its output is */
  const double *moments;         /* device [4] as npb_rollout_moments writes it, or NULL: adv is copied */
  double eps;
  int32_t *index;                /* device [count] */
  void *obs, *act;               /* device [count][K][C], [count][A] (PLANT: [t][count]...), or NULL */
  float *extra;                  /* device [count][E] (PLANT: [t][count][E]), or NULL */
  void *adv_out, *ret_out;       /* device [count] (PLANT: [t][count]), or NULL */
  int max_blocks;                /* 0 = the launcher's bound */
} npb_minibatch_desc_t;
NPB_API int npb_rollout_moments(NpbHandle *h, const npb_moments_desc_t *desc, void *stream);
NPB_API int npb_rollout_permutation(NpbHandle *h, int64_t N, const uint32_t *keys, int64_t first, int64_t count, int32_t *out, void *stream);
NPB_API int npb_rollout_minibatch(NpbHandle *h, const npb_minibatch_desc_t *desc, void *stream);
NPB_API const char *npb_minibatch_check(const npb_minibatch_desc_t *desc, int n_plants, int t, int features_cells, int n_axes, int n_extras);

/* The normaliser: running observation and reward normalisation on the device -- what VecNormalize gives a PPO user, with the order of every
 * addition pinned.  An optional per-handle attachment.  While it is on and training, every npb_step folds this step's raw samples into
 * running statistics (count, mean, M2 per stream) and writes ref = mean and scale = 1 / sqrt(var + eps) into the features' device column
 * table BEFORE the features' pass A runs: the frame the policy sees is normalised with statistics that include it.  Optionally it keeps a
 * per-plant discounted return, folds that as one more stream, and writes a normalised reward.  nuclear_sim_amd/normalizer.py states all
 * of it in numpy, and that statement is the contract; the device produces its bits for every n_plants, storage type and launch geometry.
 * Streams, S of them: the chosen columns of the features (indices into npb_features_desc_t.columns, at most NPB_FEATURES_COLS_MAX, each
 * NPB_FEATURE_AFFINE with a constant ref), then, with reward != 0, the return stream.  Per stream three doubles, count, mean, M2, all 0 at
 * the start.
 * One fold over the n plants, stream c with raw sample x[p] (the column's value before any transform, widened to double as the features
 * widen it; for the return stream ret[p], below):
 *     shift = count[c] > 0 ? mean[c] : the column's own ref (the return stream: 0.0)
 *     d = x[p] - shift;  q = d * d                          each rounded (-ffp-contract=off)
 *     a sample counts iff q - q == 0.0                      not a NaN, an infinity or a square that overflows; one that does not count
 *                                                           contributes +0.0, +0.0 and count 0: a bad value never poisons a statistic
 *     s1 = tree(d), s2 = tree(q)                            the tree of npb_rollout_moments over the plants in order: groups of 256
 *                                                           padded with +0.0, the halves 128 .. 1, then the further levels
 *     cnt = the samples that count;  N = count + cnt
 *     if cnt > 0: mean = shift + s1 / N;  M2 = (M2 + s2) - (s1 * s1) / N, 0.0 where that is negative      IEEE division
 *     count = N
 *   Chan's merge with the batch taken around the running mean (normalizer.py derives it); from count == 0 it is the plain shifted-data
 *   formula around the column's ref.  The features' table then holds ref = mean, scale = 1.0 / sqrt(M2 / count + eps) (IEEE root and
 *   division) where count > 0, else the column's own ref and scale; lo, hi, nan_to stay the column's: the clip of the normalised
 *   observation is the column's clip.
 * The return stream (gamma, clip): per plant ret (double) and primed / seen as the features use them, and ended, this step's done[p] != 0.
 *     carry = primed && episode_index == seen && !ended (of the step before);  ret = (carry ? ret * gamma : 0.0) + r
 *   with ret * gamma rounded before the sum; r and done are the task's while a task is set, else the step's.  Behind fold and merge
 *     norm_reward[p] = r * rscale, then y = y < -clip ? -clip : y, y = y > clip ? clip : y (a NaN passes both)
 *   rscale = 1.0 / sqrt(M2 / count + eps) of the return stream (1.0 while its count is 0); the mean is not subtracted.  A truncation, an
 *   autoreset or a caller's reset / restore shows as a changed episode index.  A handle WITHOUT autoreset (npb_set_autoreset) carries no
 *   episode index: the index then always counts as the one seen and the carry is kept, so a caller that restarts plants itself
 *   (npb_reset, npb_restore) calls npb_normalizer_clear for them.
 * Fresh frames (the features' pass B and the priming) are not folded: they are normalised with the table as it stands.
 * npb_normalizer_training(h, 0) freezes: no fold and no table write, the two fold launches are skipped; norm_reward is still written, with
 * the frozen scale, and ret is still carried.
 * With the normaliser training npb_step launches two kernels more, three with the return stream, behind the task kernel and in front of
 * the features' pass A: the partials kernel (npd_normalizer.h; a workgroup of 256 per 256 plants = one group of the tree, the differences
 * and squares through LDS, eight streams a pass, counts by ballot; no division, no atomics, no scratch), the finish kernel
 * (npb_minibatch.hip, built with IEEE division and root: one workgroup ends the tree over the partials, merges, writes the state and,
 * one lane per stream, ref and scale into the features' table) and the reward kernel (one lane per plant).  With the return stream
 * npb_launch_rollout_post records norm_reward in place of the reward; the episode kernel, episode_return, the episode records, the
 * statistics and the windows keep the raw reward.  Nothing else in the sequence moves.
 * npb_set_normalizer(h, desc): desc = NULL turns it off, and the features' table gets the columns' own ref and scale back.  The state
 * starts at zero.  NPB_EINVAL with the reason in npb_last_error, before any device work, for what npb_normalizer_check refuses -- that
 * check alone, without a handle (features_desc: the features it would sit on, or NULL), NULL = accepted, else the reason: n_plants < 1;
 * columns chosen while no features are set; a column count out of range or without its array; a column index out of range or named
 * twice; a NPB_FEATURE_BITS column or one whose ref is a second column; a NaN or negative eps; gamma a NaN or outside [0, 1]; clip a NaN
 * or not positive; a NULL or misaligned norm_reward; neither columns nor reward.  On the handle: npb_set_normalizer while a rollout is set
 * (set the normaliser first); npb_set_features, set and NULL alike, while a normaliser with columns is on; npb_set_task, set and NULL
 * alike, while the return stream reads the task's reward; npb_step without a reward or done column while the return stream is on.
 * npb_normalizer_get_state / npb_normalizer_set_state move count, mean, M2 (double [S] each) and, with the return stream, ret (double
 * [n_plants]), primed, seen, ended (int32 [n_plants] each; NULL without it) to and from host arrays, synchronous on `stream`; set_state
 * is followed by one finish launch without a batch, so that the table follows a loaded state (a dry run's statistics warm-start a run).
 * npb_normalizer_clear(h, mask, stream): the plants of mask (device uint8 [n_plants], NULL = all) start a new return on their next step.
 * These return NPB_EINVAL when no normaliser is set.  npb_destroy drops it.
 * Not here: statistics over fresh frames; per-plant statistics (npb_set_column_stats has them); an exponential-moving-average variant;
 * half types; synchronising shards on the device (normalizer.merge is the host answer); normalising BITS or setpoint-error columns.
 * NPB_VERSION stays 154: a binding detects the entry points by name.  A handle that never calls this behaves as before in every entry
 * point.  Synchronising shards on the device has the section ONE NORMALISER AND ONE SET OF ADVANTAGE MOMENTS ACROSS SHARDS below. */
typedef struct npb_normalizer_desc_t {
  int n_columns; const int *columns;      /* host: indices into the features' columns; 0 / NULL = the return stream alone */
  double eps;
  int reward;                    /* != 0: the return stream */
  double gamma, clip;
  double *norm_reward;           /* device [n_plants]; with reward */
} npb_normalizer_desc_t;
NPB_API int npb_set_normalizer(NpbHandle *h, const npb_normalizer_desc_t *desc);
NPB_API const char *npb_normalizer_check(const npb_normalizer_desc_t *desc, int n_plants, const npb_features_desc_t *features_desc);
NPB_API int npb_normalizer_training(NpbHandle *h, int on);
NPB_API int npb_normalizer_get_state(NpbHandle *h, double *count, double *mean, double *M2, double *ret, int32_t *primed, int32_t *seen,
                                     int32_t *ended, void *stream);
NPB_API int npb_normalizer_set_state(NpbHandle *h, const double *count, const double *mean, const double *M2, const double *ret,
                                     const int32_t *primed, const int32_t *seen, const int32_t *ended, void *stream);
NPB_API int npb_normalizer_clear(NpbHandle *h, const uint8_t *mask, void *stream);

/* The policy: the one link of the per-step chain that used to leave the library -- between the features and the controls' input an MLP
 * actor-critic, the Gaussian draw, the log-probability and the value -- run on the device, in ONE launch in front of the rollout's pre
 * kernel.  An optional per-handle attachment; it needs features and controls to be set.  nuclear_sim_amd/policy.py states all of it in
 * numpy, and that statement is the contract; the device produces its bits for every n_plants and launch geometry, with one licensed
 * difference: the float tanh.
 * The nets: a diagonal-Gaussian actor and a critic, two separate MLPs of 1 .. NPB_POLICY_HIDDEN_MAX hidden layers each, widths 1 ..
 * NPB_POLICY_WIDTH_MAX chosen per net, activation NPB_POLICY_RELU or NPB_POLICY_TANH.  Input: the features' out[p] flattened, K * C
 * cells, a double tensor narrowed to float first (round to nearest even).  The actor's head has A outputs, A the controls' axis count;
 * the critic's one.
 * The parameters: one flat float vector theta -- the actor's layers, then the critic's, then log_std[A], then std[A]; a layer is
 * W[out][in] row-major, then b[out].  std is the caller's exp(log_std): the device takes no exponential.
 * One layer, for output j: acc = b[j], then for k ascending acc = fmaf(x[k], W[j][k], acc) in float, a single rounding per step; k is
 * extended with +0.0 cells and +0.0 weights to a multiple of 4.  A subnormal result or accumulator is outside the contract.  relu: acc >
 * 0 ? acc : +0.0; tanh: the device's float tanh (the statement: the double tanh narrowed).
 * The noise: Philox4x32-10, key = the two halves of seed (low first), counter = (first_plant + p, t & 0xffffffff, t >> 32, j); t is the
 * policy's draw counter, a uint64 on the handle, advanced by every step the policy samples in; call j serves axes 2j and 2j + 1: u1 =
 * (w0 * 2^20 + (w1 >> 12) + 0.5) * 2^-52, u2 likewise from w2 and w3, r = sqrt(-2 * log(u1)), th = 6.283185307179586 * u2, z0 = r *
 * cos(th), z1 = r * sin(th), in double.  deterministic != 0: nothing is drawn, z = 0 and t does not advance.
 * The outputs, in double, every operation rounded on its own:
 *   a[i] = (double)mean[i] + (double)std[i] * z[i], narrowed to the controls' input type and written to their bound `in` tensor
 *   lp   = -(A * 0.9189385332046727), then for i ascending lp = (lp - 0.5 * (z[i] * z[i])) - (double)log_std[i]
 *   value[p] = the critic's float; logp[p] = (float)lp: the density of the UNROUNDED action.  With extras_in (the rollout's bound [n][E]
 *   input) value and logp also go to its columns value_slot and logp_slot (-1 = none), so the rollout's pre kernel records them.
 * A plant with a NaN or infinite feature gets THE quiet NaN in every output and touches no other plant.
 * npb_set_policy(h, desc): desc = NULL turns it off.  theta starts as zeros: npb_policy_load before the first step.  While a policy is
 * set npb_set_features, npb_set_controls and npb_set_rollout are refused, set and NULL alike, naming the policy: it reads and writes their
 * tensors in the shapes it was set with (so: features, controls, rollout, then the policy).  The policy is the one writer of the
 * controls' input: what the caller wrote there is overwritten by every step.  NPB_EINVAL with the reason in npb_last_error, before any
 * device work: no features or no controls set, and what npb_policy_check refuses -- that check alone, without a handle (features_cells
 * = K * C, n_axes = the controls' axis count), NULL = accepted, else the reason: n_plants < 1; features_cells outside 1 ..
 * NPB_FEATURES_CELLS_MAX; n_axes outside 1 .. NPB_CONTROLS_AXES_MAX; a layer count or a width out of range; an unknown activation;
 * first_plant negative or first_plant + n_plants beyond 2^32; a NULL or misaligned value or logp (4-byte aligned); slots without
 * extras_in, extras_in without a count in 1 .. NPB_ROLLOUT_EXTRAS_MAX, a slot outside -1 .. E - 1, both slots the same column, a
 * misaligned extras_in.
 * npb_policy_count(desc, features_cells, n_axes): the length of theta for these shapes (0 for a NULL descriptor).
 * npb_policy_load(h, theta, theta_is_device, stream): new parameters into the existing allocation and one launch that lays the weights
 *   out as the kernel reads them (transposed, padded with +0.0); no reallocation, and no synchronisation for a device source.
 * npb_policy_values(h, rows, type, n_rows, out, stream): the critic alone over any contiguous device [n_rows][K * C] tensor of float
 *   (NPB_FEATURES_F32) or double (NPB_FEATURES_F64); rows = NULL: the features' out.  out: device float [n_rows].  It gives the
 *   last_value (from the current features) and the final_value (from the rollout's final_obs) of npb_rollout_advantages.
 * npb_policy_noise(h, t, z, words, stream): the z of draw t, device double [n][A], and (words != NULL) the Philox words behind it,
 *   device uint32 [n][(A + 1) / 2][4], by the device function the step's launch inlines.  Either may be NULL, not both.
 * npb_policy_get_state / npb_policy_set_state carry t.  npb_destroy drops the policy.
 * npb_collect(h, steps, obs, reward, done, trip_flags, info, stream): `steps` calls of npb_step with NULL input columns and these output
 *   columns, without a return to the caller in between.  Refused before any device work unless a policy is set, a rollout is set with
 *   room for `steps` more slots, and every input column can be NULL: not under NPB_HEAT_EXTERNAL, not with the heat-source noise enabled
 *   unless episode streams drive it, not with a power profile seeded on the handle unless episode streams drive it.  Prime the features
 *   first (npb_features_prime).
 * The kernel (npb_policy.hip) runs on the f32 matrix cores (v_mfma_f32_32x32x2_f32: exact f32, the statement's fmaf chain two k a call; the
 * relu tests hold it to the statement's bits): one workgroup per 32 plants, the activations through LDS, no atomics, no scratch.
 * THE RECURRENT CORE (npb_set_policy_core; npb_policy_core.hip; nuclear_sim_amd/recurrent.py states it in numpy, and that statement is the
 * contract): one GRU cell of width H = 1 .. NPB_POLICY_WIDTH_MAX shared by actor and critic, in the same ONE launch.  Its input is the K * C
 * feature cells; both nets read the new hidden state h' in place of the features (their first layers have in = H).  Parameters in
 * torch.nn.GRUCell's layout and gate order (r, z, n), at the front of theta: W_ih[3H][K * C] | b_ih[3H] | W_hh[3H][H] | b_hh[3H] | the
 * actor | the critic | log_std | std.  One step of one plant, all float, every operation rounded on its own:
 *   gi = layer(x, W_ih, b_ih); gh = layer(h, W_hh, b_hh)      (the fmaf chain above)
 *   r[j] = S(gi[j] + gh[j]); z[j] = S(gi[H + j] + gh[H + j]); n[j] = T(gi[2H + j] + r[j] * gh[2H + j]); h'[j] = n[j] + z[j] * (h[j] - n[j])
 * NPB_POLICY_GATES_HARD (bit-exact): y = 0.25f * a + 0.5f, S = y < 0 ? +0.0 : (y > 1 ? 1 : y); T = a < -1 ? -1 : (a > 1 ? 1 : a).
 * NPB_POLICY_GATES_SOFT: T = the float tanh, S(a) = 0.5f * tanh(0.5f * a) + 0.5f: the float tanh stays the one licensed difference.
 * Restart: in front of a step a plant's h is +0.0 where the plant is unprimed (fresh, or restarted by npb_reset, npb_reset_reference,
 * npb_restore, npb_restore_bank, which unprime exactly the plants of their mask) or where its carried episode index is not the one the
 * policy saw last (the autoreset's restarts); a step then primes the plant and remembers the index.  A plant with a non-finite feature
 * gets THE quiet NaN in every output and h' = +0.0.
 * npb_policy_core_t: width, gates, and device tensors of the caller's: hidden [n][H], the live state, updated in place by every step;
 *   first [n][H] or NULL: on the step recorded into slot 0 of a set rollout, the h that step read, the restart rule applied; final
 *   [n * final_rows][H] or NULL with final_rows = 0 (else the set rollout's final_rows): behind the rollout's post kernel, hidden[p] -- the
 *   h' of this step -- into row final_row[t][p] for every plant that took a row of final_obs.  The value of a truncated transition's
 *   terminal state is critic(GRU(final_obs[row], final[row])).
 * npb_set_policy_core(h, desc, core): npb_set_policy with a core (core = NULL: without one).  npb_policy_core_check(core, n_plants,
 *   features_cells): that check alone, without a handle; NULL = accepted, else the reason: n_plants < 1; features_cells out of range; a width
 *   outside 1 .. NPB_POLICY_WIDTH_MAX; unknown gates; a NULL hidden; final_rows < 0; final without final_rows or final_rows without final;
 *   n_plants * final_rows beyond int32; a misaligned tensor.  npb_policy_core_count(desc, core, features_cells, n_axes): theta's length.
 * npb_policy_values_hidden(h, rows, type, n_rows, hidden_rows, out, stream): the critic over GRU(rows, hidden_rows), hidden_rows device float
 *   [n_rows][H] the states in front of the rows; rows = NULL and hidden_rows = NULL: the current features and the live hidden state under the
 *   restart rule (the last_value: a plant that restarted on the last step bootstraps from +0.0).  Nothing is written to hidden, seen or
 *   primed.  npb_policy_values is refused by name while a core is set.
 * npb_policy_core_get_state / _set_state carry hidden (HOST float [n][H]), seen and primed (HOST int32 [n]).
 * Training through time is not built into the row-wise entry points: npb_policy_grad, _update and _shard_sums (and their _more forms) refuse a
 *   policy with a core by name, because rows carry no order.  npb_policy_grad_seq, npb_policy_update_seq and npb_policy_shard_sums_seq (below:
 *   TRAINING THROUGH TIME) take whole sequences; npb_policy_train_begin, _apply_shards and _combine_shards read no rows and serve both.
 * Not here: a shared trunk; discrete or squashed (tanh-Gaussian) actions; a state-dependent std; LSTM cells, stacked or per-net cores; half types; noise that restarts with the episode; skipping the forward pass on held steps of interval > 1.
 * NPB_VERSION stays 154: a binding detects the entry points by name.  A handle that never calls this behaves as before in every entry
 * point. */
#define NPB_POLICY_HIDDEN_MAX 3
#define NPB_POLICY_WIDTH_MAX 128
enum { NPB_POLICY_RELU = 0, NPB_POLICY_TANH = 1 };
typedef struct npb_policy_desc_t {
  int actor_layers, actor_width[NPB_POLICY_HIDDEN_MAX];        /* hidden layers and their widths */
  int critic_layers, critic_width[NPB_POLICY_HIDDEN_MAX];
  int activation;                /* NPB_POLICY_RELU | NPB_POLICY_TANH */
  int deterministic;             /* != 0: z = 0, t stands */
  uint64_t seed;
  int64_t first_plant;           /* the counter's first word is first_plant + p */
  float *value, *logp;           /* device [n_plants] each */
  float *extras_in;              /* device [n_plants][n_extras]: the rollout's bound extras input, or NULL */
  int n_extras, value_slot, logp_slot;      /* E; columns of extras_in, -1 = none */
} npb_policy_desc_t;
NPB_API int npb_set_policy(NpbHandle *h, const npb_policy_desc_t *desc);
NPB_API const char *npb_policy_check(const npb_policy_desc_t *desc, int n_plants, int features_cells, int n_axes);
NPB_API int64_t npb_policy_count(const npb_policy_desc_t *desc, int features_cells, int n_axes);
NPB_API int npb_policy_load(NpbHandle *h, const float *theta, int theta_is_device, void *stream);
NPB_API int npb_policy_values(NpbHandle *h, const void *rows, int type, int n_rows, float *out, void *stream);
NPB_API int npb_policy_noise(NpbHandle *h, uint64_t t, double *z, uint32_t *words, void *stream);
NPB_API int npb_policy_get_state(NpbHandle *h, uint64_t *t);
NPB_API int npb_policy_set_state(NpbHandle *h, uint64_t t);
enum { NPB_POLICY_GATES_SOFT = 0, NPB_POLICY_GATES_HARD = 1 };
typedef struct npb_policy_core_t {
  int width;                     /* H */
  int gates;                     /* NPB_POLICY_GATES_SOFT | NPB_POLICY_GATES_HARD */
  float *hidden;                 /* device [n_plants][H] */
  float *first;                  /* device [n_plants][H], or NULL */
  float *final;                  /* device [n_plants * final_rows][H], or NULL */
  int final_rows;                /* R of the set rollout, 0 without final */
} npb_policy_core_t;
NPB_API int npb_set_policy_core(NpbHandle *h, const npb_policy_desc_t *desc, const npb_policy_core_t *core);
NPB_API const char *npb_policy_core_check(const npb_policy_core_t *core, int n_plants, int features_cells);
NPB_API int64_t npb_policy_core_count(const npb_policy_desc_t *desc, const npb_policy_core_t *core, int features_cells, int n_axes);
NPB_API int npb_policy_values_hidden(NpbHandle *h, const void *rows, int type, int n_rows, const float *hidden_rows, float *out, void *stream);
NPB_API int npb_policy_core_get_state(NpbHandle *h, float *hidden, int32_t *seen, int32_t *primed, void *stream);
NPB_API int npb_policy_core_set_state(NpbHandle *h, const float *hidden, const int32_t *seen, const int32_t *primed, void *stream);
NPB_API int npb_collect(NpbHandle *h, int steps, double *obs, double *reward, uint8_t *done, uint32_t *trip_flags, double *info, void *stream);

/* Training the set policy on the device: the PPO loss of one minibatch, its gradient through both nets, the gradient's clipping and one
 * Adam step, with no autograd graph and no optimiser outside the library.  nuclear_sim_amd/ppo.py states all of it in numpy, and that
 * statement is the contract; the device produces its bits for every count, storage type and launch geometry, with the forward pass's
 * licensed float tanh and two more licensed differences: the device's double exp for the ratio and for std.
 * One minibatch (npb_ppo_desc_t) is `count` rows as npb_rollout_minibatch gathers them: obs [count][K * C] (float or double: NPB_FEATURES_F32
 * / _F64), act [count][A] (NPB_CONTROLS_F32 / _F64), logp_old [count] float, adv and ret [count] of one type (NPB_ROLLOUT_F32 / _F64).
 * Forward: the step's own layer routine, every hidden activation kept.  Per row, in double, every operation rounded on its own:
 *   d[a] = ((double)act[a] - (double)mean[a]) / (double)std[a];  lp as the step forms logp, with d for z;  r = exp(lp - (double)logp_old)
 *   clipped = (adv > 0 and r > 1 + clip) or (adv < 0 and r < 1 - clip), every comparison strict;  c = clipped ? 0.0 : -(adv * r)
 *   the seeds, narrowed once: dmean[a] = (float)(((c * d[a]) / std[a]) / count), dv = (float)((vf_coef * ((double)v - ret)) / count)
 *   dls[a] = (c * (d[a] * d[a] - 1.0)) / count;  policy loss -min(r * adv, clamp(r, 1 - clip, 1 + clip) * adv);  value loss 0.5 * (v - ret)^2;
 *   kl = (r - 1.0) - (lp - logp_old)
 * A row with a feature, an action, logp_old, adv or ret that is not finite is SKIPPED: its features read as +0.0, every seed and term
 * of it is +0.0, it is counted, and its logp_new, value_new and ratio are THE quiet NaN; the divisor stays count.
 * Backward, float, per net from the head down: back[i][k] = the chain over j ascending of fmaf(delta[i][j], W[j][k], acc) from +0.0; relu:
 * delta' = h > 0 ? back : +0.0; tanh: delta' = back * (1.0f - h * h), three rounded operations.
 * The sums over rows are pinned: the rows are cut into chains of rows_per_chain rows (a positive multiple of 32); within a chain dW[j][k]
 * = fmaf(delta[i][j], h[i][k], acc) for i ascending from +0.0 (db: h = 1.0f); across chains the partials are widened, added in ascending
 * chain order onto 0.0 and narrowed once; the per-row doubles likewise.  grad(log_std[a]) = (float)(sum dls[a] - ent_coef), grad(std[a])
 * = 0.  Then norm = sqrt(the pinned tree of npb_rollout_moments over (double)g * (double)g) over every entry but std's, and with
 * max_grad_norm > 0 (0 = off) g = (float)((double)g * min(1.0, max_grad_norm / (norm + 1e-6))).
 * stats, NPB_PPO_STATS doubles: policy_loss, value_loss, entropy, approx_kl, clip_fraction (means over count), skipped, grad_norm, count.
 * Adam: the state is m, v (float, theta's layout) and step.  npb_policy_adam advances step and forms step_size = lr / (1 - b1^step)
 * and root = sqrt(1 - b2^step) on the host; per element in double, each result narrowed once: m' = b1 * m + (1 - b1) * g, v' = b2 * v +
 * (1 - b2) * (g * g), theta' = theta - step_size * (m' / (sqrt(v') / root + eps)); std's slots are skipped and then std[a] =
 * (float)exp((double)log_std'[a]); the launch that lays the weights out as the step reads them follows, so the next step runs the new policy.
 * npb_ppo_check(desc, features_cells, n_axes): the host-only validator, NULL = accepted, else the reason: a NULL descriptor; a NULL obs,
 * act, logp_old, adv or ret; an unknown type; count < 1; rows_per_chain not a positive multiple of 32; clip outside (0, 1); a vf_coef,
 * ent_coef or max_grad_norm that is not finite, or max_grad_norm < 0; max_blocks < 0; a tensor misaligned for its element.
 * npb_policy_grad(h, desc, stream): leaves grad [theta_count] and stats on the handle; the optional outputs logp_new, value_new (float)
 * and ratio (double), [count] each, may be NULL.  npb_policy_adam(h, lr, b1, b2, eps, stream): one step from the gradient on the handle.
 * npb_policy_update: both.  npb_policy_get_grad / _get_stats / _get_theta copy into DEVICE buffers (float [theta_count], double
 * [NPB_PPO_STATS], float [theta_count]) on the stream, nothing read back.  npb_policy_optimizer_get_state / _set_state carry m, v (HOST
 * float [theta_count]) and step.  The optimiser's buffers and the chains' workspace belong to the policy: allocated on first use, grown on
 * demand, dropped with it.  NPB_EINVAL by name before any device work: no policy set, and what npb_ppo_check refuses.
 * The gradient kernel (npb_ppo.hip) runs on the f32 matrix cores (v_mfma_f32_32x32x2_f32), a workgroup a chain, no atomics.
 * Not here: a shared trunk, learning-rate schedules (host arithmetic: lr is an argument of every update), half types.
 *
 * THE OPTIONS (npb_ppo_more_t; the entry points below that take one; a binding detects them by name, NPB_VERSION stays 154).  With
 * more == NULL, and with clip_vf == 0 and kl_limit == 0, every launch computes the bits of the calls above.
 * Value-loss clipping (clip_vf > 0; value_old device [count] float, what the rollout recorded in the policy's value slot), the max form
 * of baselines' PPO2.  Per row, in double, every operation rounded on its own, behind diff = (double)v - ret:
 *   dvo = (double)v - (double)value_old;  dc = dvo < -clip_vf ? -clip_vf : (dvo > clip_vf ? clip_vf : dvo)
 *   vc = (double)value_old + dc;  diffc = vc - ret;  sq = diff * diff;  sqc = diffc * diffc
 *   use = sqc > sq (strict);  out = dvo < -clip_vf or dvo > clip_vf (strict)
 *   value loss = 0.5 * (use ? sqc : sq);  dv = (float)((vf_coef * (use ? (out ? 0.0 : diffc) : diff)) / count);  vf_clipped = out ? 1.0 : 0.0
 * With clip_vf > 0 a value_old that is not finite makes the row a skipped row; with clip_vf == 0 value_old is not read and may be NULL.
 * More statistics, always formed: four more per-row doubles, +0.0 on a skipped row -- ret, ret * ret, diff, diff * diff (always the
 * unclipped diff) -- summed as the other per-row doubles are.  From the sums S_r, S_rr, S_d, S_dd and m = count - skipped:
 *   vr = S_rr / m - (S_r / m) * (S_r / m);  vd = S_dd / m - (S_d / m) * (S_d / m);  explained_variance = 1.0 - vd / vr
 * THE quiet NaN when m < 1 or not vr > 0.  more, NPB_PPO_STATS_MORE doubles: vf_clip_fraction (the pinned sum of vf_clipped over count),
 * explained_variance, applied, stopped (1.0 / 0.0: what the gate made of the last update; 1.0, 0.0 with no gate).
 * The gate (kl_limit > 0; target_kl early stopping as SB3 takes it, kl_limit = 1.5 * target_kl formed by the caller in double), on the
 * device between the finish kernel and the Adam kernel, so nothing is read back per update:
 *   stopped' = stopped or (approx_kl > kl_limit)  (strict; a NaN approx_kl does not stop);  applied = not stopped'
 * An update that is not applied leaves theta, std, m and v exactly as they were; its gradient and all its statistics are still formed.
 * Once stopped, every later update up to npb_policy_train_end is not applied.  step counts applied updates only: they are a prefix, so
 * update i (0-based) since npb_policy_train_begin, if applied, is step step0 + i + 1.
 * npb_ppo_more_check(more, count): the host-only validator, NULL = accepted (a NULL more is), else the reason: a clip_vf or kl_limit that
 * is negative or not finite; clip_vf > 0 with value_old NULL; a misaligned value_old (4-byte aligned).
 * npb_policy_grad_more(h, desc, more, stream): npb_policy_grad with the options; kl_limit > 0 is refused by name (the gate is an
 * update's).  npb_policy_update_more(h, desc, more, lr, b1, b2, eps, stream): npb_policy_update with the options.
 * npb_policy_train_begin(h, stream) clears stopped and applied on the device and remembers step0 = step.  npb_policy_train_end(h,
 * applied, stream) is THE ONE READ-BACK: it waits for the stream, reads the count of applied updates (into *applied unless NULL), sets
 * step = step0 + applied and disarms the gate.  Between the two, refused by name: npb_policy_optimizer_get_state,
 * npb_policy_optimizer_set_state, npb_policy_adam, a second npb_policy_train_begin, and an update with kl_limit == 0 (every update of
 * the pair is gated: that keeps the applied ones a prefix).  Outside a pair an update with kl_limit > 0 and npb_policy_train_end are
 * refused by name.  A policy set again or dropped takes an open pair with it.
 * npb_policy_get_stats_more(h, more, stream) copies into a DEVICE buffer, double [NPB_PPO_STATS_MORE], nothing read back. */
#define NPB_PPO_STATS 8
#define NPB_PPO_STATS_MORE 4
typedef struct npb_ppo_desc_t {
  const void *obs; int obs_type;             /* device [count][K * C]; NPB_FEATURES_F32 | NPB_FEATURES_F64 */
  const void *act; int act_type;             /* device [count][A]; NPB_CONTROLS_F32 | NPB_CONTROLS_F64 */
  const float *logp_old;                     /* device [count] */
  const void *adv, *ret; int adv_type;       /* device [count] each; NPB_ROLLOUT_F32 | NPB_ROLLOUT_F64, both */
  int count;
  float *logp_new, *value_new; double *ratio;      /* device [count] each, or NULL */
  double clip, vf_coef, ent_coef, max_grad_norm;   /* max_grad_norm 0 = off */
  int rows_per_chain;                        /* a positive multiple of 32: the statement's chains */
  int max_blocks;                            /* workgroups the gradient kernel launches at most, 0 = the library's choice; no bit depends on it */
} npb_ppo_desc_t;
NPB_API const char *npb_ppo_check(const npb_ppo_desc_t *desc, int features_cells, int n_axes);
NPB_API int npb_policy_grad(NpbHandle *h, const npb_ppo_desc_t *desc, void *stream);
NPB_API int npb_policy_adam(NpbHandle *h, double lr, double b1, double b2, double eps, void *stream);
NPB_API int npb_policy_update(NpbHandle *h, const npb_ppo_desc_t *desc, double lr, double b1, double b2, double eps, void *stream);
NPB_API int npb_policy_get_grad(NpbHandle *h, float *grad, void *stream);
NPB_API int npb_policy_get_stats(NpbHandle *h, double *stats, void *stream);
NPB_API int npb_policy_get_theta(NpbHandle *h, float *theta, void *stream);
NPB_API int npb_policy_optimizer_get_state(NpbHandle *h, float *m, float *v, uint64_t *step, void *stream);
NPB_API int npb_policy_optimizer_set_state(NpbHandle *h, const float *m, const float *v, uint64_t step, void *stream);
typedef struct npb_ppo_more_t {
  const float *value_old;                    /* device [count], or NULL with clip_vf == 0 */
  double clip_vf;                            /* 0 = off */
  double kl_limit;                           /* 0 = this update neither raises nor obeys the gate */
} npb_ppo_more_t;
NPB_API const char *npb_ppo_more_check(const npb_ppo_more_t *more, int count);
NPB_API int npb_policy_grad_more(NpbHandle *h, const npb_ppo_desc_t *desc, const npb_ppo_more_t *more, void *stream);
NPB_API int npb_policy_update_more(NpbHandle *h, const npb_ppo_desc_t *desc, const npb_ppo_more_t *more, double lr, double b1, double b2, double eps,
                                   void *stream);
NPB_API int npb_policy_train_begin(NpbHandle *h, void *stream);
NPB_API int npb_policy_train_end(NpbHandle *h, uint32_t *applied, void *stream);
NPB_API int npb_policy_get_stats_more(NpbHandle *h, double *more, void *stream);

/* TRAINING ONE POLICY ACROSS SHARDS (npb_ppo_shards_t; the entry points below; a binding detects them by name, NPB_VERSION stays 154).
 * An update is cut where the pinned double sums end: a handle exports the sums of its own rows (npb_policy_shard_sums), a second call
 * adds W such vectors in ascending shard order and finishes the update (npb_policy_apply_shards).  Every replica that applies the same
 * W vectors computes the same bits, so replicas stay identical with no broadcast of parameters; two handles on one device train one
 * policy the same way, and one handle accumulates several minibatches into one Adam step by writing their sums into the rows of one
 * buffer.  nuclear_sim_amd/ppo.py (shard_sums, combine) states both calls in numpy.  A handle that never calls these computes the bits
 * it computed before, in every entry point.
 * The vector: L = npb_ppo_shard_count(theta_count, n_axes) = theta_count - 2 * n_axes + NPB_PPO_SHARD_ROWS doubles -- every weight and
 * bias slot in theta's layout, up to where log_std starts, then the NPB_PPO_SHARD_ROWS (18) per-row sums: dls[a] at a (< 8, +0.0 beyond
 * A), policy_loss 8, kl 9, clipped 10, skipped 11, value_loss 12, vf_clipped 13, ret 14, ret2 15, diff 16, diff2 17.
 * npb_policy_shard_sums(h, desc, more, count_total, out, stream): the gradient kernel of npb_policy_grad_more over desc's count rows,
 * with ONE change in the per-row arithmetic: every seed is divided by the count of the whole update,
 *   dmean[a] = (float)(((c * d[a]) / std[a]) / (double)count_total);  dv = (float)((vf_coef * seed) / (double)count_total)
 *   dls[a] = (c * (d[a] * d[a] - 1.0)) / (double)count_total
 * then a lane an entry: sums[e] = the chains' partials (per-row sums) widened, added in ascending chain order onto 0.0, stored as a
 * double and NOT narrowed; ent_coef is not yet subtracted.  out: a DEVICE double [L], 8-byte aligned; it may be a row of a larger [W][L]
 * buffer.  ent_coef and max_grad_norm of desc are not read; more may be NULL, and its kl_limit must be 0 (the gate belongs to the
 * combine).  The handle's grad, stats, more and the gate's words are left as they were.  Refused by name: count_total < desc->count, a
 * NULL or misaligned out, kl_limit > 0, and what npb_ppo_check and npb_ppo_more_check refuse.
 * npb_policy_apply_shards(h, shards, lr, b1, b2, eps, stream): a lane a parameter,
 *   total[e] = 0.0;  for w ascending  total[e] = total[e] + sums[w][e]      (in double)
 *   grad[e] = (float)total[e];  grad(log_std[a]) = (float)(total_dls[a] - ent_coef);  grad(std[a]) = 0
 * then what npb_policy_grad does behind its own sums: the norm over the pinned tree, the scale by max_grad_norm (0 = off), stats and more
 * with count = count_total and the 18 totals for the sums, the gate on the GLOBAL approx_kl (kl_limit > 0), the Adam step (gated when
 * kl_limit > 0) and the launch that lays the weights out as the step reads them.  With n_shards == 1 and count_total == count the two
 * calls are npb_policy_update_more, bit for bit.  Between npb_policy_train_begin and npb_policy_train_end only an apply with kl_limit >
 * 0 is accepted; outside the pair one with kl_limit > 0 is refused by name.
 * npb_policy_combine_shards(h, shards, stream): the same without Adam and without the gate (kl_limit > 0 is refused by name, as
 * npb_policy_grad_more refuses it); grad, stats and more stay on the handle for npb_policy_get_grad / _get_stats / _get_stats_more.
 * npb_ppo_shards_check(shards, count, n_axes): the host-only validator (count: theta's element count), NULL = accepted, else the
 * reason: a NULL descriptor or NULL sums; sums misaligned for a double; n_shards outside 1 .. NPB_PPO_SHARDS_MAX (64); count_total < 1
 * or beyond 2^53; an ent_coef or max_grad_norm that is not finite, or max_grad_norm < 0; a kl_limit that is negative or not finite; an
 * axis count outside 1 .. 8 or a count that leaves no weights.  NPB_EINVAL by name before any device work: no policy set, and those.
 * One exchange moves 8 * L bytes a shard.  The kernels use plain vector stores, no atomics and no scratch.
 * Not here: synchronising the running normaliser between shards (normalizer.merge stays the host answer); advantage moments over all
 * shards (every shard normalises its own); shards with different numbers of updates; overlapping the exchange with the next minibatch's
 * gather; the exchange itself (the caller's all-gather: nuclear_sim_amd/sharding.py has one over torch.distributed); any measurement
 * across more than one device.  The first two have the section below. */
#define NPB_PPO_SHARD_ROWS 18
#define NPB_PPO_SHARDS_MAX 64
typedef struct npb_ppo_shards_t {
  const double *sums;                        /* device [n_shards][L], shard order */
  int n_shards;                              /* 1 .. NPB_PPO_SHARDS_MAX */
  int64_t count_total;                       /* the rows of the whole update: what every shard divided its seeds by */
  double ent_coef, max_grad_norm, kl_limit;  /* max_grad_norm 0 = off; kl_limit 0 = no gate */
} npb_ppo_shards_t;
NPB_API int64_t npb_ppo_shard_count(int64_t theta_count, int n_axes);
NPB_API const char *npb_ppo_shards_check(const npb_ppo_shards_t *shards, int64_t count, int n_axes);
NPB_API int npb_policy_shard_sums(NpbHandle *h, const npb_ppo_desc_t *desc, const npb_ppo_more_t *more, int64_t count_total, double *out,
                                  void *stream);
NPB_API int npb_policy_apply_shards(NpbHandle *h, const npb_ppo_shards_t *shards, double lr, double b1, double b2, double eps, void *stream);
NPB_API int npb_policy_combine_shards(NpbHandle *h, const npb_ppo_shards_t *shards, void *stream);

/* TRAINING THROUGH TIME (npb_ppo_seq_t; the entry points below; a binding detects them by name, NPB_VERSION stays 154): PPO over whole
 * sequences for a policy with a core (npb_set_policy_core) -- the loss above and its gradient through both nets, through the GRU cell and
 * through time, on the device.  nuclear_sim_amd/recurrent.py (gradient, shard_sums) states it in numpy, out of ppo.py's own functions, and
 * that statement is the contract: the device gives its bits with hard gates and relu nets when fed the device's ratio.  A handle that
 * never calls these computes the bits it computed before, in every entry point.
 * One sequence minibatch is npb_ppo_desc_t's tensors TIME-MAJOR, as npb_rollout_minibatch gathers them with NPB_MINIBATCH_PLANT: obs [t]
 * [plants][K * C], act [t][plants][A], logp_old, adv, ret (and value_old) [t][plants]; count = t * plants; rows_per_chain is read as the
 * PLANTS of a chain (a positive multiple of 32).  npb_ppo_seq_t says where the sequences came from: t, plants, index [plants] (the
 * minibatch's own index output: the rollout's plant of every sequence; NULL = identity), and the rollout's tensors episode [T][n_plants],
 * ended [T][n_plants] and the core's first [n_plants][H]; hidden, optional, receives every cell's h'.  The kernel reads a plant's restart words and its state in front of slot 0
 * through index; an index outside 0 .. n_plants - 1 makes every cell of that plant a skipped, poisoned cell and nothing is read through it.
 * first is the state the COLLECTING parameters produced: after the first update of an iteration it is stale; that is inherent, and what
 * every recurrent PPO does.  Here a sequence is differentiated whole; truncated segments have the section below (TRUNCATED SEGMENTS).
 * Forward: the step's recurrence under the current theta.  Slot s reads h_s, +0.0 where the plant restarted in front of s (episode[s] !=
 * episode[s - 1], or ended[s - 1] & NPB_ROLLOUT_CUT; a restart in front of slot 0 is in first); the cell gives h'_s, +0.0 on a poisoned
 * cell (a feature that is not finite); both nets read h'_s.  Per cell the row-wise epilogue, unchanged; a cell whose features are finite
 * and whose act, logp_old, adv, ret (or value_old) is not is a skipped row: its seeds are +0.0, the cell still runs, the carry still flows.
 * Backward, s descending, all float, every operation rounded on its own:
 *   dh' = (carry + back(delta_actor_layer0, W_actor0)) + back(delta_critic_layer0, W_critic0)      no derivative: h' is an input; carry = +0.0 behind the last slot
 * On a poisoned cell dh', every gate delta and the outgoing carry are +0.0.  Otherwise, with u = h - n:
 *   dn = dh' * (1.0f - z);  dz = dh' * u;  direct = dh' * z
 *   dan = dn * T'      soft: T' = 1.0f - n * n;  hard: +0.0 where the forward took a clamped branch (a < -1 or a > 1), else dn
 *   dghn = dan * r;  dr = dan * gh_n
 *   daz = dz * S'(z)   soft: S' = s * (1.0f - s);  hard: +0.0 where y < 0 or y > 1 (the forward's own strict tests), else d * 0.25f
 *   dar = dr * S'(r)   likewise
 *   delta_i = [dar | daz | dan];  delta_h = [dar | daz | dghn]      (3H wide, GRUCell's row order)
 *   carry_out = direct + back(delta_h, W_hh)      ONE fmaf chain over the 3H rows of W_hh ascending, from +0.0
 * and carry_out is +0.0 where the plant restarted in front of slot s.
 * The sums are pinned: a chain is rows_per_chain plants with all their slots; within a chain the rows enter in the order tiles of 32
 * plants ascending, within a tile s DESCENDING, within a slot the plants ascending.  dW_ih, db_ih come from (delta_i, x) and dW_hh, db_hh
 * from (delta_h, h); x of a poisoned cell reads +0.0; the nets' as above, their first layers reading h'.  Across chains as above.  The
 * gradient is in theta's layout, the core in front; clipping, stats, more, the options and Adam are unchanged.
 * npb_ppo_seq_check(desc, seq, features_cells, n_axes): the host-only validator, NULL = accepted, else the reason: a NULL seq; what
 * npb_ppo_check refuses of desc; t < 1; plants < 1; count != t * plants; n_plants < 1; t * n_plants beyond 2^31 - 1; a NULL episode, ended
 * or first; a misaligned index, episode, first or hidden (4-byte aligned).
 * npb_policy_grad_seq(h, desc, more, seq, stream): npb_policy_grad_more over sequences (more may be NULL; kl_limit > 0 is refused by name).
 * npb_policy_update_seq(h, desc, more, seq, lr, b1, b2, eps, stream): the gradient and the Adam step, gated as npb_policy_update_more is.
 * npb_policy_shard_sums_seq(h, desc, more, seq, count_total, out, stream): npb_policy_shard_sums over sequences; count_total counts cells
 * (t * plants of every shard).  npb_policy_apply_shards / _combine_shards take its vectors.  All three refuse a policy without a core by name.
 * The kernel (npb_ppo_seq.hip): one workgroup a chain, per tile of 32 plants a forward sweep that stores only h' ([t][plants][H] floats,
 * a workspace the handle grows on demand) and a backward sweep that recomputes the gates; f32 matrix cores, no atomics, no scratch.
 * Measured on an MI355X (tools/recurrent_train_cost.py): one update of t = 128 through a cell of 64 and (64, 64) nets takes 21.0 ms at
 * 4 096 plants and 30.1 ms at 8 192 (the same BPTT in eager torch: 26.3 / 39.8 ms); serial in t, plants / 32 workgroups.
 * Not here: sequences longer than one rollout; the exchange between shards (the caller's all-gather).  Truncated segments: the section below. */
typedef struct npb_ppo_seq_t {
  int t, plants;                             /* slots and sequences of the minibatch: desc->count == t * plants */
  const int32_t *index;                      /* device [plants]: the rollout's plant of every sequence, or NULL = identity */
  int n_plants;                              /* the rollout's plants: the row length of episode and ended, the rows of first */
  const int32_t *episode;                    /* device [>= t][n_plants]: the rollout's episode */
  const uint8_t *ended;                      /* device [>= t][n_plants]: the rollout's ended */
  const float *first;                        /* device [n_plants][H]: the core's first */
  float *hidden;                             /* device [t][plants][H], or NULL: where the states h' under the current theta go (NULL: the handle's workspace) */
} npb_ppo_seq_t;
NPB_API const char *npb_ppo_seq_check(const npb_ppo_desc_t *desc, const npb_ppo_seq_t *seq, int features_cells, int n_axes);
NPB_API int npb_policy_grad_seq(NpbHandle *h, const npb_ppo_desc_t *desc, const npb_ppo_more_t *more, const npb_ppo_seq_t *seq, void *stream);
NPB_API int npb_policy_update_seq(NpbHandle *h, const npb_ppo_desc_t *desc, const npb_ppo_more_t *more, const npb_ppo_seq_t *seq, double lr, double b1,
                                  double b2, double eps, void *stream);
NPB_API int npb_policy_shard_sums_seq(NpbHandle *h, const npb_ppo_desc_t *desc, const npb_ppo_more_t *more, const npb_ppo_seq_t *seq, int64_t count_total,
                                      double *out, void *stream);

/* TRUNCATED SEGMENTS (the entry points below; a binding detects them by name, NPB_VERSION stays 154; no existing struct changes): truncated
 * back-propagation through time for a policy with a core.  The rollout's t recorded slots are cut into chunks = t / every segments of
 * `every` slots; each starts from the state RECORDED in front of its first slot and is differentiated within itself only.  A segment id is
 * g = c * n_plants + p: chunk c, plant p, slots c * every .. c * every + every - 1 of plant p.  A segment of L slots with a stored start state
 * IS what the section above calls a sequence -- t = L, a `first` row, restart words found through an index -- so nothing of the loss, the
 * backward pass, the sums or the optimiser is restated.  nuclear_sim_amd/recurrent.py (starts, segment_words, gradient_segments,
 * shard_sums_segments) and rollout.py (minibatch with unit "segment") state it in numpy, out of the functions they already have.  Opt-in: a
 * handle that never calls these computes, in every entry point, the bits it computed before.
 * npb_policy_core_segments(h, every, starts, rows): starts a device float tensor [rows][n_plants][H] of the caller's, rows >= ceil(T / every), T
 *   the set rollout's horizon.  On the step recorded into slot s of the set rollout with s % every == 0 the run of h that the cell kernel read,
 *   the restart rule applied (+0.0 for a restarted plant), goes into row s / every -- what `first` receives at slot 0: starts[0] equals first
 *   bit for bit, and first is written as before.  Steps at other slots write nothing; npb_rollout_begin starts over at row 0.  every = 0 clears
 *   it (starts and rows are not read).  It follows `first`: set after npb_set_rollout and npb_set_policy_core, dropped with the policy.
 *   npb_policy_core_segments_check(every, starts, rows, horizon, core_width): that check alone, NULL = accepted, else the reason: no core
 *   (core_width < 1); no rollout (horizon < 1); every < 0 or every > horizon; rows < ceil(horizon / every); a NULL or misaligned starts (4-byte
 *   aligned).  every == 0 is accepted with anything.
 * npb_rollout_minibatch_segments(h, desc, every, stream): npb_rollout_minibatch with desc->unit == NPB_MINIBATCH_SEGMENT: N = chunks *
 *   n_plants; index[j] = permutation(N)[first + j] is a segment id g; every output is time-major [every][count]..., out[s][j] = src[c * every +
 *   s][p].  The normalisation, the permutation and the types are unchanged; the kernel is the same, its `slots` every and its source c * every
 *   slots down.  npb_minibatch_segments_check(desc, every, n_plants, t, features_cells, n_axes, n_extras): what npb_minibatch_check refuses,
 *   and a unit that is not NPB_MINIBATCH_SEGMENT, every < 1, every > t, t % every != 0 (ragged last segments are not here).
 *   npb_rollout_minibatch refuses NPB_MINIBATCH_SEGMENT as an unknown unit: its descriptor has no room for every.
 * npb_policy_grad_segments / _update_segments / _shard_sums_segments(h, desc, more, seq, seg, ...): their _seq forms with npb_ppo_segments_t
 *   {every, chunks} beside npb_ppo_seq_t, whose fields then mean: seq->t == every; seq->plants the SEGMENTS of the minibatch; seq->n_plants the
 *   rollout's plants; seq->index[j] = g; seq->first = starts read as [chunks * n_plants][H], row g; episode and ended [>= chunks * every]
 *   [n_plants].  The kernel's only differences: an index decodes to (c, p) = (g / n_plants, g % n_plants); a g outside 0 .. chunks * n_plants - 1
 *   poisons the sequence and nothing is read through it; the restart words of local slot s > 0 are read at rollout rows c * every + s and
 *   c * every + s - 1, column p; the restart in front of local slot 0 is in starts already and no word at row c * every - 1 is read; the state
 *   in front of local slot 0 is starts row g; the carry out of local slot 0 is dropped -- that is the truncation.  The order of the sums is
 *   unchanged (chains of rows_per_chain SEGMENTS: tiles ascending, slots descending, segments ascending), and so are the epilogue, clip_vf,
 *   the gate, more, Adam, and the shard sums with count_total counting cells.  The h' workspace stays count * H floats.
 *   npb_ppo_segments_check(desc, seq, seg, features_cells, n_axes): what npb_ppo_seq_check refuses, a NULL seg, every < 1, chunks < 1,
 *   seq->t != every, chunks * every * n_plants beyond 2^31 - 1.
 * npb_policy_segment_starts(h, every, stream): the refresh.  After the first update of an iteration the stored states are stale.  One
 *   forward-only launch recomputes rows 1 .. chunks - 1 of the set starts under the CURRENT theta from the rollout's own tensors: for every
 *   plant the recurrence from `first` over the recorded obs slots, the kernel's restart and poison rules; row c receives the state read in
 *   front of slot c * every; row 0 is left alone.  One workgroup per tile of 32 plants, serial in t: the gradient kernel's forward sweep, the
 *   same code.  Under the collecting parameters it reproduces the recorded rows bit for bit, soft gates included.  Refused by name: no core,
 *   no rollout, no starts set, every not the set one, nothing recorded, t % every != 0.
 * Measured on an MI355X (tools/recurrent_train_cost.py --segments, profiles/segment_train_cost.json): one update of t = 128 through a cell of
 *   64 and (64, 64) nets over all segments of 16 takes 7.8 / 15.6 / 31.4 ms at 2 048 / 4 096 / 8 192 plants against 19.8 / 20.6 / 30.0 ms over
 *   whole sequences in the same run: faster below 8 192 plants, 5 % slower at 8 192, where the chip is already full.  Recording adds nothing
 *   measurable to a step; the refresh launch takes 1.7 ms over 128 slots.
 * Not here: ragged last segments (t % every != 0 is refused by name); burn-in slots and overlapping segments; segments longer than one
 * rollout; per-slot storage of every state; LSTM cells; any change to the row-wise entry points or to the plant kernels. */
typedef struct npb_ppo_segments_t {
  int every;                                 /* L: the slots of a segment; seq->t */
  int chunks;                                /* t / L: the rows of starts; a segment id is c * n_plants + p with c < chunks */
} npb_ppo_segments_t;
NPB_API int npb_policy_core_segments(NpbHandle *h, int every, float *starts, int rows);
NPB_API const char *npb_policy_core_segments_check(int every, const float *starts, int rows, int horizon, int core_width);
NPB_API int npb_rollout_minibatch_segments(NpbHandle *h, const npb_minibatch_desc_t *desc, int every, void *stream);
NPB_API const char *npb_minibatch_segments_check(const npb_minibatch_desc_t *desc, int every, int n_plants, int t, int features_cells, int n_axes, int n_extras);
NPB_API const char *npb_ppo_segments_check(const npb_ppo_desc_t *desc, const npb_ppo_seq_t *seq, const npb_ppo_segments_t *seg, int features_cells, int n_axes);
NPB_API int npb_policy_grad_segments(NpbHandle *h, const npb_ppo_desc_t *desc, const npb_ppo_more_t *more, const npb_ppo_seq_t *seq, const npb_ppo_segments_t *seg,
                                     void *stream);
NPB_API int npb_policy_update_segments(NpbHandle *h, const npb_ppo_desc_t *desc, const npb_ppo_more_t *more, const npb_ppo_seq_t *seq, const npb_ppo_segments_t *seg,
                                       double lr, double b1, double b2, double eps, void *stream);
NPB_API int npb_policy_shard_sums_segments(NpbHandle *h, const npb_ppo_desc_t *desc, const npb_ppo_more_t *more, const npb_ppo_seq_t *seq,
                                           const npb_ppo_segments_t *seg, int64_t count_total, double *out, void *stream);
NPB_API int npb_policy_segment_starts(NpbHandle *h, int every, void *stream);

/* ONE NORMALISER AND ONE SET OF ADVANTAGE MOMENTS ACROSS SHARDS (the entry points below; a binding detects them by name, NPB_VERSION
 * stays 154; no new struct).  What still made a sharded run W different runs: every shard folded only its own plants into its running
 * normaliser, and every shard normalised its advantages with its own moments.  Both are cut where the pinned sums end, as the gradient
 * is: a shard exports a short double vector, the caller all-gathers it, and every shard combines the W rows in ascending shard order.
 * Replicas that combine the same rows hold the same bits, so nothing is broadcast.  nuclear_sim_amd/normalizer.py (shard_delta, combine)
 * and nuclear_sim_amd/rollout.py (moments_part, moments_combine, moments_shards) state the calls in numpy, every operation in double and
 * rounded on its own; the device produces their bits.  A handle that never calls these computes the bits it computed before, in every
 * entry point; no step, fold, moments, permutation or minibatch kernel changes.
 * THE NORMALISER.  Beside its state a handle keeps the BASE, double [3][S] (count, then mean, then M2): what the shards agreed on at the
 * last synchronisation, zeros from npb_set_normalizer on.  npb_normalizer_shard_count(h) = 3 * S (0, with the reason in npb_last_error,
 * when no normaliser is set).
 * npb_normalizer_shard_delta(h, out, stream): out, a DEVICE double [3][S], 8-byte aligned, takes per stream the population folded since
 * the base -- Chan's merge run backwards, a lane per stream:
 *     na, ma, Ma = base;  N, m, M = the state;  nb = N - na
 *     nb > 0:   mb = m + (m - ma) * (na / nb);   d = mb - ma
 *               Mb = (M - Ma) - (d * d) * ((na * nb) / N),   0.0 where that is negative
 *               delta = (nb, mb, Mb)
 *     else:     delta = (0.0, 0.0, 0.0)        (a frozen shard, or one that did not step)
 *   With a zero base the delta is the state exactly.  Neither the state nor the base is written.
 * npb_normalizer_apply_shards(h, deltas, n_shards, stream): deltas a DEVICE double [W][3][S] in shard order, W = 1 ..
 * NPB_PPO_SHARDS_MAX.  A lane per stream starts from the base and goes through w ascending; only a shard with nb > 0 is merged:
 *     N = n + nb;  d = mb - mean;  mean = mean + d * (nb / N)
 *     M2 = (M2 + Mb) + (d * d) * ((n * nb) / N);  n = N
 *   The result is written as the state AND as the base; one finish launch without a batch follows, so scale (the return stream's rscale)
 *   and the features' table follow it exactly as they follow npb_normalizer_set_state.  The per-plant return carry (ret, primed, seen,
 *   ended) stays with its shard.  It is allowed while frozen: npb_normalizer_training(h, 0) stops folds, not synchronisation.  W = 1 is
 *   the identity only from a zero base: un-merging and re-merging rounds.
 * npb_normalizer_get_base / npb_normalizer_set_base move the base to and from a HOST double [3][S], synchronous on `stream`, for
 * checkpoints.  npb_set_normalizer zeroes the base; npb_normalizer_set_state leaves it alone.
 * npb_normalizer_shards_check(deltas, n_shards): the host-only validator, NULL = accepted, else the reason: deltas NULL; deltas
 * misaligned for a double; n_shards outside 1 .. NPB_PPO_SHARDS_MAX (64).  NPB_EINVAL by name before any device work: no normaliser set,
 * a NULL or misaligned out or base, and those.
 * THE MOMENTS.  npb_rollout_moments is cut in four: every shard's part, the combine, every shard's part around the GLOBAL mean, the
 * combine.  Both calls take the existing npb_moments_desc_t.
 * npb_rollout_moments_part(h, desc, squares, part, stream): part, a DEVICE double [2] = {count, total}.  count = rows * cols; total is
 * the undivided value npb_rollout_moments has before its division: a column's rows added in order onto 0.0, then the tree over the
 * columns.  With squares != 0 the summands are the rounded squares of (double)x - desc->out[1]: the mean is read where
 * npb_rollout_moments reads it.  desc->out is never written.  desc->ddof is not used -- the combine divides -- but the descriptor is
 * checked as npb_rollout_moments checks it: pass 0.
 * npb_rollout_moments_combine(h, parts, n_shards, squares, ddof, out, stream): parts a DEVICE double [W][2] in shard order; one lane,
 *     C = 0.0;  T = 0.0;  for w ascending  C = C + count_w;  T = T + total_w
 *   squares == 0: out[0] = C, out[1] = T / C.  squares != 0: out[2] = T / (C - ddof), out[3] = sqrt(out[2]).  IEEE division and root.
 *   With W = 1 the four calls are npb_rollout_moments, bit for bit: no total is ever -0.0, so 0.0 + T is T.
 * npb_moments_shards_check(desc, part, parts, n_shards, ddof, out): the host-only validator of both.  desc != NULL: the part is checked
 * -- whatever npb_rollout_moments refuses a descriptor for (a count <= desc->ddof among it), part NULL, part misaligned for a double.
 * desc == NULL: the combine is checked -- parts NULL or misaligned; n_shards outside 1 .. NPB_PPO_SHARDS_MAX (64); ddof < 0; out NULL or
 * misaligned.  The shards' counts are device values: a total count <= ddof cannot be seen on the host and gives an infinity or a NaN, as
 * the division says; a part's count is >= 1 because its descriptor's is.
 * One exchange moves 24 * S bytes a shard for the normaliser and 16 bytes, twice, for the moments.  The kernels (npb_minibatch.hip, for
 * its IEEE division and root) use plain vector stores, no atomics and no scratch.
 * Still not here: the exchange itself (the caller's all-gather; sharding.gather_shard_sums serves every vector); any measurement across
 * more than one device; a synchronisation of the per-plant return carry (it belongs to its plants). */
NPB_API int npb_normalizer_shard_count(NpbHandle *h);
NPB_API const char *npb_normalizer_shards_check(const double *deltas, int n_shards);
NPB_API int npb_normalizer_shard_delta(NpbHandle *h, double *out, void *stream);
NPB_API int npb_normalizer_apply_shards(NpbHandle *h, const double *deltas, int n_shards, void *stream);
NPB_API int npb_normalizer_get_base(NpbHandle *h, double *base, void *stream);
NPB_API int npb_normalizer_set_base(NpbHandle *h, const double *base, void *stream);
NPB_API const char *npb_moments_shards_check(const npb_moments_desc_t *desc, const double *part, const double *parts, int n_shards, int ddof,
                                             const double *out);
NPB_API int npb_rollout_moments_part(NpbHandle *h, const npb_moments_desc_t *desc, int squares, double *part, void *stream);
NPB_API int npb_rollout_moments_combine(NpbHandle *h, const double *parts, int n_shards, int squares, int ddof, double *out, void *stream);

/* Measurement aid (no reference counterpart): streams every state column through the GPU unchanged,
 * 2 * npb_state_bytes() * pitch bytes with the step kernel's access shape; used to calibrate the
 * rocprofv3 FETCH_SIZE / WRITE_SIZE counters (tools/profile_traffic.py). */
NPB_API int npb_debug_touch(NpbHandle *h, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NPB_H */
