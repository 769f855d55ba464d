/*
 * npb_kernels.hip -- the plant kernels for gfx950 (MI355X): the fused step kernels bench.py times and the maintenance rule they call,
 * and the kernels that move whole plants -- observe, init, reset, restore, episode, the operator's maintenance orders, field get / set /
 * gather.  Compiled once per storage type; its launchers make up npb_launch_table / npb32_launch_table.  What else libnpb.so holds,
 * and why in units of its own: DESIGN.md, "The translation units of libnpb.so".
 *
 * One wavefront lane = one plant.  State lives in HBM as a struct-of-arrays: column `slot` of the
 * fp64 table is f64[slot * Npad + plant], so every load/store instruction of a wave touches 64
 * consecutive doubles (512 B, fully coalesced).  A plant's ~530 carried scalars do not fit a lane's
 * register file at once, so the step STREAMS the plant subsystem by subsystem in the reference's own
 * order (NuclearPlantSimulator.step, simulator/core/sim.py:130-258; SecondaryReactorPhysics.update_system,
 * systems/secondary/__init__.py:340-1021):
 *
 *   primary -> coupling -> feedwater (4 pumps, one at a time) -> 3 steam generators (one at a time)
 *   -> turbine -> condenser -> electrical-power gates -> feedback -> observation / reward / done
 *
 * Each phase's section struct reaches the registers through the LDS staging pipeline of npd_stage.h (LDS-DMA
 * one phase ahead, because one wave per SIMD has nothing else to hide HBM latency behind), is updated in
 * registers and stored back at the next phase boundary; only the ~30 coupling scalars stay live between
 * phases.  No MFMA (there is no dense contraction on this path), no inter-lane communication except the
 * turbine stage pass's ballot and the LDS transposes that turn the wave's 64 x 22 observation block into
 * coalesced row-major stores.  Plants are independent, so blocks never share data and the block -> XCD
 * placement cannot matter.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "npd_common.h"
/* diagnostic build only (-DNPB_STAMPS, tools/phase_stamps.py): lane 0 of every wave records s_memtime
 * at phase boundaries so the kernel's time can be attributed to phases on the GPU */
#ifdef NPB_STAMPS
#ifdef NPB_BUILD_F32
#define npb_stamp_buf npb32_stamp_buf
#define npb_debug_set_stamp_buffer npb32_debug_set_stamp_buffer
#endif
__device__ unsigned long long *npb_stamp_buf;
#define NPD_STAMP(k) do { if (threadIdx.x == 0 && npb_stamp_buf) npb_stamp_buf[(size_t)blockIdx.x * 32 + (k)] = __builtin_readcyclecounter(); } while (0)
extern "C" __attribute__((visibility("default"))) int npb_debug_set_stamp_buffer(unsigned long long *dev) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(npb_stamp_buf), &dev, sizeof(dev));
}
#define NPD_WAIT_ACC_STORE() do { if (threadIdx.x == 0 && npb_stamp_buf) npb_stamp_buf[(size_t)blockIdx.x * 32 + 23] = npd_wait_acc_s; } while (0)
#else
#define NPD_STAMP(k)
#define NPD_WAIT_ACC_STORE()
#endif
#include "npd_stage.h"
#include "npd_arena.h"
#include "npd_record_log.h"
#include "npd_primary.h"
#include "npd_sg.h"
#include "npd_feedwater.h"
#include "npd_turbine.h"
#include "npd_condenser.h"
#include "npd_ph.h"
#include "npd_maintenance.h"
#include "npd_component_maintenance.h"
#include "npd_turbine_maintenance.h"
#include "npd_component_auto.h"
#include "npd_init.h"
#include "npd_reset.h"
#include "npd_step.h"
#include "npb_kernels.h"

#ifndef NPD_OUT_STORE
#define NPD_OUT_STORE 1   /* how a narrow column of output members only is stored (npd_st_store_elide): 1 = plain store, never fetched (round 4: 65 536 plants 0.0884 -> 0.0838 ms, calibrated reads 269.8 -> 255.7 MB per launch, profiles/r4_out_store.txt) */
#endif
#define NPB_OBS_PAD 23 /* LDS row stride in doubles: 22 + 1 keeps the transpose at <= 2-way bank conflicts */


/* ---- step kernel: section stores through the pinned 32-bit-offset addressing of npd_stage.h.
 * bits of narrow member j of a section struct: outputs as float, then the int32 members */
template <int NF, int NO, int NI, typename S>
__device__ __forceinline__ uint32_t npd_narrow_bits(const S &s, int j) {
  const double *d = reinterpret_cast<const double *>(&s);
  const int32_t *q = reinterpret_cast<const int32_t *>(d + NF);
  if (j < NO) return __float_as_uint((float)d[NF - NO + j]);
  if (j < NO + NI) return (uint32_t)q[j - NO];
  return 0u;
}
/* store the narrow column c of a section instance (col = its arena column) from NPD_NPC 32-bit words */
#define NPD_STORE_REAL(col, v) npd_store_real<SM>(st, (col), (v))
template <int SM = 0>
__device__ __forceinline__ void npd_st_store_narrow(const npd_stage_t &st, int col, uint32_t w0, uint32_t w1) {
#ifdef NPB_BUILD_F32
  npd_gstore<SM == 2>(NPD_NP(uint32_t, col, 0), w0);
#else
  typedef uint32_t npd_u32x2 __attribute__((ext_vector_type(2)));
  npd_u32x2 v; v.x = w0; v.y = w1;
  if constexpr (SM >= 1) npd_store8<SM == 2>(st, (uint32_t)col, v);
  else npd_gstore<false>(NPD_RPO(npd_u32x2, col, st.laner), v);
#endif
}
template <int NF, int NO, int NI, typename S, int SM = 0>
__device__ __forceinline__ void npd_st_store(const S &s, const npd_stage_t &st, int col0) {
  const double *d = reinterpret_cast<const double *>(&s);
  constexpr int NC = NF - NO, NNC = (NO + NI + NPD_NPC - 1) / NPD_NPC;
#pragma unroll
  for (int k = 0; k < NC; k++) NPD_STORE_REAL(col0 + k, d[k]);
#pragma unroll
  for (int c = 0; c < NNC; c++)
    npd_st_store_narrow<SM>(st, col0 + NC + c, npd_narrow_bits<NF, NO, NI>(s, c * NPD_NPC), npd_narrow_bits<NF, NO, NI>(s, c * NPD_NPC + 1));
}
template <int NF, int NO, int NI, int SID, typename S>
__device__ __forceinline__ void npd_st_load(S &s, const npd_stage_t &st, int col0) {
  double *d = reinterpret_cast<double *>(&s);
  constexpr int NC = NF - NO;
#pragma unroll
  for (int k = 0; k < NC; k++) d[k] = (double)*NPD_RP(col0 + k);
#pragma unroll
  for (int j = 0; j < NO; j++) d[NC + j] = (double)*NPD_NP(const float, col0 + NC + j / NPD_NPC, j % NPD_NPC);
  int32_t *q = reinterpret_cast<int32_t *>(d + NF);
#pragma unroll
  for (int k = 0; k < NI; k++) q[k] = *NPD_NP(const int32_t, col0 + NC + (NO + k) / NPD_NPC, (NO + k) % NPD_NPC);
  NPD_PROBE_STRUCT(SID, NF, NI, d, q);
}
#define NPD_ST_LOAD(T, stype, s, inst) \
  npd_st_load<NPB_##T##_NF64, NPB_##T##_NOUT, NPB_##T##_NI32, NPB_##T##_F64_BASE, stype>(s, st, NPD_SEC_COL(T, inst))
#define NPD_ST_STORE(T, stype, s, inst) \
  npd_st_store<NPB_##T##_NF64, NPB_##T##_NOUT, NPB_##T##_NI32, stype, NPD_SM>(s, st, NPD_SEC_COL(T, inst))
/* only the narrow columns of a section (its outputs and int32 members) */
template <int NF, int NO, int NI, typename S, int SM = 0>
__device__ __forceinline__ void npd_st_store_narrow_cols(const S &s, const npd_stage_t &st, int col0) {
  constexpr int NC = NF - NO, NNC = (NO + NI + NPD_NPC - 1) / NPD_NPC;
#pragma unroll
  for (int c = 0; c < NNC; c++)
    npd_st_store_narrow<SM>(st, col0 + NC + c, npd_narrow_bits<NF, NO, NI>(s, c * NPD_NPC), npd_narrow_bits<NF, NO, NI>(s, c * NPD_NPC + 1));
}
#define NPD_ST_STORE_NARROW(T, stype, s, inst) \
  npd_st_store_narrow_cols<NPB_##T##_NF64, NPB_##T##_NOUT, NPB_##T##_NI32, stype, NPD_SM>(s, st, NPD_SEC_COL(T, inst))
/* ---- unchanged-column elision.  Measured on the bench workload (and on a reactor-heat-source batch): about a
 * quarter of the carried columns keep their exact bits over a step for every plant of a wave -- flags, status
 * codes, protection timers at rest, pump pressures and cavitation state in normal operation, the spare pump,
 * the kinetics block under the constant heat source.  A global store occupies the lone wave of a SIMD for its
 * transfer time, a bitwise compare + wave ballot costs three instructions, so the
 * members named in the masks below are stored only if some lane's bits changed.  Which members are listed is a
 * performance choice only: the compare is on the bit patterns, so the arena always ends up with exactly the
 * bits a plain store would have written.  "old" is the copy of the section as it was staged in. */
/* SKIP0 .. SKIP1: carried members that were not loaded this step and must not be stored (wave-uniform `skip`) */
template <int NF, int NO, int NI, int SKIP0 = 0, int SKIP1 = 0, typename S, int SM = 0>
__device__ __forceinline__ void npd_st_store_elide(const S &s, const S &old, const npd_stage_t &st, int col0, uint64_t fmask, bool skip = false) {
  const double *d = reinterpret_cast<const double *>(&s), *od = reinterpret_cast<const double *>(&old);
  constexpr int NC = NF - NO, NNC = (NO + NI + NPD_NPC - 1) / NPD_NPC;
#ifdef NPB_PROBE
  fmask = 0; /* the liveness probe looks at the physics only, not at the elision's old copies */
#endif
  if (SKIP1 > SKIP0 && !skip) {
#pragma unroll
    for (int k = SKIP0; k < SKIP1; k++) {
      if ((fmask >> k) & 1) {
        if (__builtin_amdgcn_ballot_w64(npd_real_bits(d[k]) != npd_real_bits(od[k])) != 0) NPD_STORE_REAL(col0 + k, d[k]);
      } else {
        NPD_STORE_REAL(col0 + k, d[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NC; k++) {
    if (k >= SKIP0 && k < SKIP1) continue;
    if ((fmask >> k) & 1) {
      if (__builtin_amdgcn_ballot_w64(npd_real_bits(d[k]) != npd_real_bits(od[k])) != 0) NPD_STORE_REAL(col0 + k, d[k]);
    } else {
      NPD_STORE_REAL(col0 + k, d[k]);
    }
  }
  /* narrow columns (outputs as float, flags, status codes, counters): compared -- except the columns that hold nothing but
   * OUTPUT members (the first NO / NPD_NPC of them): the step never reads an output, so comparing its old bits is the only
   * reason the column would be fetched at all (round 3's counters: reads 1.16x algorithmic, 284 B per plant of it these).
   * NPD_OUT_STORE: 0 = compare like the rest (round 3), 1 = plain store, no compare, no load, 2 = the same, non-temporal */
#pragma unroll
  for (int c = 0; c < NNC; c++) {
    const uint32_t w0 = npd_narrow_bits<NF, NO, NI>(s, c * NPD_NPC), w1 = npd_narrow_bits<NF, NO, NI>(s, c * NPD_NPC + 1);
#ifdef NPB_PROBE
    npd_st_store_narrow<SM>(st, col0 + NC + c, w0, w1);
#else
    if (NPD_OUT_STORE != 0 && (c + 1) * NPD_NPC <= NO) {
      npd_st_store_narrow<(NPD_OUT_STORE == 2 ? 2 : SM)>(st, col0 + NC + c, w0, w1);
      continue;
    }
    const uint32_t o0 = npd_narrow_bits<NF, NO, NI>(old, c * NPD_NPC), o1 = npd_narrow_bits<NF, NO, NI>(old, c * NPD_NPC + 1);
    if (__builtin_amdgcn_ballot_w64(NPD_NPC == 2 ? ((w0 != o0) | (w1 != o1)) : (w0 != o0)) != 0) npd_st_store_narrow<SM>(st, col0 + NC + c, w0, w1);
#endif
  }
}
#define NPD_ST_STORE_ELIDE(T, stype, s, old, inst) \
  npd_st_store_elide<NPB_##T##_NF64, NPB_##T##_NOUT, NPB_##T##_NI32, 0, 0, stype, NPD_SM>(s, old, st, NPD_SEC_COL(T, inst), NPD_ELIDE_##T##_F)
/* the primary section: the point-kinetics members move only under ReactorHeatSource (npb_fields.h, NPB_PRIM_NKIN) */
#define NPD_PRIM_KIN0 (NPB_PRIM_NCARRY - NPB_PRIM_NKIN)
#define NPD_ST_STORE_ELIDE_PRIM(s, old) \
  npd_st_store_elide<NPB_PRIM_NF64, NPB_PRIM_NOUT, NPB_PRIM_NI32, NPD_PRIM_KIN0, NPB_PRIM_NCARRY, npb_prim_t, NPD_SM>( \
      s, old, st, NPD_SEC_COL(PRIM, 0), NPD_ELIDE_PRIM_F, !kinetics)
#define NPD_FB(stype, m) (1ull << NPB_F64_SLOT(stype, m))
#define NPD_FBN(stype, m, n) ((((1ull << (n)) - 1)) << NPB_F64_SLOT(stype, m))
static constexpr uint64_t NPD_ELIDE_PRIM_F =
    NPD_FB(npb_prim_t, neutron_flux) | NPD_FB(npb_prim_t, reactivity) | NPD_FBN(npb_prim_t, precursors, 6) |
    NPD_FB(npb_prim_t, coolant_flow_rate) | NPD_FB(npb_prim_t, coolant_void_fraction) | NPD_FB(npb_prim_t, steam_pressure) |
    NPD_FB(npb_prim_t, feedwater_flow_rate) | NPD_FB(npb_prim_t, control_rod_position) | NPD_FB(npb_prim_t, steam_valve_position) |
    NPD_FB(npb_prim_t, boron_concentration) | NPD_FB(npb_prim_t, xenon_concentration) | NPD_FB(npb_prim_t, iodine_concentration) |
    NPD_FB(npb_prim_t, samarium_concentration) | NPD_FB(npb_prim_t, burnable_poison_worth) | NPD_FB(npb_prim_t, fuel_burnup) |
    NPD_FB(npb_prim_t, total_reactivity_pcm) | NPD_FB(npb_prim_t, hs_filtered_noise_mw);
static constexpr uint64_t NPD_ELIDE_SG_F = NPD_FB(npb_sg_t, water_level);
static constexpr uint64_t NPD_ELIDE_PUMP_F =
    NPD_FB(npb_pump_t, suction_pressure) | NPD_FB(npb_pump_t, discharge_pressure) | NPD_FB(npb_pump_t, npsh_available) |
    NPD_FB(npb_pump_t, differential_pressure) | NPD_FB(npb_pump_t, cavitation_intensity) | NPD_FB(npb_pump_t, cavitation_damage) |
    NPD_FB(npb_pump_t, cavitation_time) | NPD_FB(npb_pump_t, head_degradation) | NPD_FB(npb_pump_t, seal_leakage_rate) |
    /* the spare pump */ NPD_FB(npb_pump_t, speed_percent) | NPD_FB(npb_pump_t, speed_setpoint) | NPD_FB(npb_pump_t, flow_rate) |
    NPD_FB(npb_pump_t, power_consumption) | NPD_FB(npb_pump_t, flow_demand) | NPD_FB(npb_pump_t, motor_temperature) |
    NPD_FB(npb_pump_t, vibration_level) | NPD_FB(npb_pump_t, wear_motor_bearings) | NPD_FB(npb_pump_t, wear_pump_bearings) |
    NPD_FB(npb_pump_t, wear_thrust_bearing) | NPD_FB(npb_pump_t, wear_coupling_system) | NPD_FB(npb_pump_t, flow_degradation) |
    NPD_FB(npb_pump_t, vibration_increase);
static constexpr uint64_t NPD_ELIDE_FW_F =
    NPD_FBN(npb_fw_t, previous_level_errors, 3) | NPD_FB(npb_fw_t, cav_accumulated_damage) | NPD_FB(npb_fw_t, cav_time_in_cavitation) |
    NPD_FB(npb_fw_t, npsh_low_low_timer) | NPD_FB(npb_fw_t, timer_low_flow) | NPD_FB(npb_fw_t, timer_high_flow) |
    NPD_FB(npb_fw_t, timer_bearing_temp) | NPD_FB(npb_fw_t, timer_motor_temp) | NPD_FB(npb_fw_t, timer_vibration) |
    NPD_FB(npb_fw_t, quality_integral_error);
static constexpr uint64_t NPD_ELIDE_TURB_F =
    NPD_FB(npb_turb_t, rotor_speed) | NPD_FB(npb_turb_t, thermal_bow) | NPD_FBN(npb_turb_t, bearing_metal_temp, 4) |
    NPD_FBN(npb_turb_t, bearing_wear_factor, 4) | NPD_FB(npb_turb_t, timer_overspeed) | NPD_FB(npb_turb_t, timer_vibration) |
    NPD_FB(npb_turb_t, timer_bearing_temp) | NPD_FB(npb_turb_t, total_power_output) | NPD_FB(npb_turb_t, vibration_displacement);
static constexpr uint64_t NPD_ELIDE_CHEM_F =
    NPD_FB(npb_chem_t, dissolved_oxygen) | NPD_FB(npb_chem_t, corrosion_inhibitor_level) | NPD_FB(npb_chem_t, treatment_efficiency) |
    NPD_FB(npb_chem_t, chlorine_residual) | NPD_FB(npb_chem_t, antiscalant_concentration) | NPD_FB(npb_chem_t, water_aggressiveness);
static constexpr uint64_t NPD_ELIDE_PH_F = NPD_FB(npb_ph_t, morpholine_tank_level) | NPD_FB(npb_ph_t, pending_morpholine_dose) |
                                           NPD_FB(npb_ph_t, integral_sum);
static constexpr uint64_t NPD_ELIDE_COND_F =
    NPD_FB(npb_cond_t, vibration_damage) | NPD_FB(npb_cond_t, condenser_pressure) | NPD_FB(npb_cond_t, air_partial_pressure) |
    NPD_FB(npb_cond_t, air_mass_in_condenser) | /* the idle ejector */ NPD_FBN(npb_cond_t, ej_nozzle_fouling, 2) |
    NPD_FBN(npb_cond_t, ej_diffuser_fouling, 2) | NPD_FBN(npb_cond_t, ej_nozzle_erosion, 2);

/* single carried column, same rule (output / int32 members are stored as whole narrow columns, see the tail) */
#define NPD_ST_F64_ELIDE(T, stype, member, inst, k, newv, oldv) do { \
    const double nv__ = (newv); \
    if (__builtin_amdgcn_ballot_w64(npd_real_bits(nv__) != npd_real_bits(oldv)) != 0) NPD_ST_F64(T, stype, member, inst, k) = (npd_real_t)nv__; } while (0)
#define NPD_ST_F64(T, stype, member, inst, k) \
  (*NPD_RP(NPD_SEC_COL(T, inst) + npd_carried_slot<NPB_##T##_NCARRY>(NPB_F64_SLOT(stype, member) + (k))))
template <int NC> __device__ __forceinline__ constexpr int npd_carried_slot(int idx) { return idx; }

/* wave-cooperative store of a [64][W] block held one row per lane into row-major global memory (non-temporal: see
 * the reward / done / flags stores) */
template <int W>
__device__ __forceinline__ void npd_store_rows(const double *row, double *__restrict__ out, double *lds,
                                               size_t block_base, size_t n_valid) {
  const int lane = threadIdx.x;
#pragma unroll
  for (int j = 0; j < W; j++) lds[lane * NPB_OBS_PAD + j] = row[j];
  NPD_LDS_DRAIN(); /* the block is one wave: LDS ordering inside a wave needs no barrier (and no vmcnt drain) */
#pragma unroll
  for (int k = 0; k < W; k++) {
    int idx = k * NPB_WAVE + lane;
    int r = idx / W, c = idx % W;
    if (block_base + r < n_valid) __builtin_nontemporal_store(lds[r * NPB_OBS_PAD + c], &out[block_base * W + idx]);
  }
  NPD_LDS_DRAIN();
}

__device__ __forceinline__ double npd_sel3(int i, double a0, double a1, double a2) { return (i == 0) ? a0 : ((i == 1) ? a1 : a2); }

/* info["reactivity_components"] (sim.py:205): the second block of the info buffer, only for a caller that asked
 * (params.info_reactivity_components) under the reactor heat source -- include/npb.h NPB_RHO_* */
__device__ __forceinline__ void npd_store_reactivity_components(const npb_params_t &P, const double *rho, double *__restrict__ info_out,
                                                                int n_plants, size_t p) {
  if (P.info_reactivity_components && P.heat_source == NPB_HEAT_REACTOR && info_out && p < (size_t)n_plants) {
    double *out = info_out + (size_t)n_plants * NPB_INFO_DIM + p * NPB_INFO_NRHO;
#pragma unroll
    for (int k = 0; k < NPB_INFO_NRHO; k++) out[k] = rho[k];
  }
}

/* NuclearPlantSimulator(enable_secondary=False).step  sim.py:141-151,186-206,253-258: the primary side alone (no coupling,
 * no secondary update, no feedback), twelve observations (the other ten columns of the obs row are written as 0), the
 * base reward, and NaN in the info columns whose keys the reference's dict then lacks.  A small kernel of its own: nothing
 * here is worth the staging pipeline. */
__global__ __launch_bounds__(NPB_WAVE) void npb_step_primary_kernel(
    npb_params_t P, int n_plants, size_t N, npd_real_t *__restrict__ f64,
    const int32_t *__restrict__ action, const double *__restrict__ magnitude, const double *__restrict__ setpoint,
    const double *__restrict__ noise_z, double *__restrict__ obs_out, double *__restrict__ reward_out,
    uint8_t *__restrict__ done_out, uint32_t *__restrict__ trip_out, double *__restrict__ info_out) {
  __shared__ double lds[NPB_WAVE * NPB_OBS_PAD];
  const size_t block_base = (size_t)blockIdx.x * NPB_WAVE;
  NPD_SEGMENT(f64, N, block_base);
  const size_t p = block_base + threadIdx.x;
  const bool live = p < (size_t)n_plants;
  const npd_inputs_t in = npd_step_inputs(live, p, action, magnitude, setpoint, noise_z, nullptr);
  npb_prim_t s;
  NPD_LOAD(PRIM, npb_prim_t, s, 0);
  if (P.heat_source != NPB_HEAT_EXTERNAL && !isnan(in.power_setpoint)) s.hs_setpoint_percent = npd_clip(in.power_setpoint, 0.0, 150.0);
  int nan_reset;
  double rho[NPB_INFO_NRHO];
  const int scram_fired = npd_primary_update(&s, &P, &in, &nan_reset, rho);
  npd_store_reactivity_components(P, rho, info_out, n_plants, p);
  s.sim_time += P.dt;
  NPD_STORE(PRIM, npb_prim_t, s, 0);
  double obs[NPB_OBS_DIM], info[NPB_INFO_DIM];
  npd_obs_primary(s, obs);
#pragma unroll
  for (int k = 12; k < NPB_OBS_DIM; k++) obs[k] = 0.0;
  if (live) {
    if (reward_out) reward_out[p] = npd_base_reward(s);
    if (done_out) done_out[p] = (uint8_t)scram_fired;
    if (trip_out) trip_out[p] = (s.scram_status ? NPB_TRIP_SCRAM : 0u) | (scram_fired ? NPB_TRIP_SCRAM_FIRED : 0u) | (nan_reset ? NPB_TRIP_NAN_RESET : 0u);
  }
  if (obs_out) npd_store_rows<NPB_OBS_DIM>(obs, obs_out, lds, block_base, (size_t)n_plants);
  if (info_out) {
#pragma unroll
    for (int k = 0; k < NPB_INFO_DIM; k++) info[k] = NAN;
    npd_info_primary(info, s.thermal_power_mw, s.total_reactivity_pcm, s.sim_time);
    npd_store_rows<NPB_INFO_DIM>(info, info_out, lds, block_base, (size_t)n_plants);
  }
}

/* automatic maintenance after a step (params.maint_enabled): AutoMaintenanceSystem.update, then the state manager's
 * threshold scan with work-order creation (npd_maintenance.h), for the four feedwater pumps -- inside the step kernels:
 *   the screen   what nearly every step of nearly every plant ends with is "nothing new".  The pump phase answers "is any
 *     threshold of this pump crossed outside its cooldown" from the registers it has just updated, the primary phase moves
 *     last_check_time where a check fell due with no order open (npd_maintenance.h).
 *   the rule     a wave that did find something calls npd_maint_rule_for_wave before it ends: first a proper look -- the
 *     rows' real comparisons on the stored state, then that pump's 16 last-violation stamps: a crossed threshold inside
 *     its cooldown is no work -- and only then the full rule for its 64 plants: work orders, the orchestrator, the
 *     thirteen handlers.  A real function call (noinline), so that its registers and its scratch are its own: rare, so it is
 *     written for clarity, not for registers, and the step kernels' own allocation does not see it.  Its constants -- the
 *     parameters, the table -- come from device memory (npd_maint_rule_consts_t, uploaded by npb_step when they change).
 * No second launch: a separate rule kernel cost 4-5 us per step just to find nothing flagged (its code and arguments are
 * cold behind the step kernel's 500 MB sweep), more than the whole screen.  npb_maint_kernel below is the same rule for the
 * modes whose step kernels do not step the pumps. */
#define NPD_MP_COL(inst, member, k) (NPD_SEC_COL(MPUMP, inst) + NPB_F64_SLOT(npb_mpump_t, member) + (k))
#define NPD_MP_LOAD(inst, member, count) do { _Pragma("unroll") for (int q__ = 0; q__ < (count); q__++) \
    mp.member[q__] = (double)*(const npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(inst, member, q__)); } while (0)
#define NPD_MP_STORE(inst, member, count) do { _Pragma("unroll") for (int q__ = 0; q__ < (count); q__++) \
    *(npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(inst, member, q__)) = (npd_real_t)mp.member[q__]; } while (0)
/* npd_maint_log, npd_maint_log_operator: the log's event sites (npd_record_log.h) */
/* does pump k of this lane's plant have a crossed threshold outside its cooldown?  (StateManager._check_maintenance_thresholds up
 * to the point where a violation is recorded, state_manager.py:1307-1369) */
__device__ __forceinline__ bool npd_maint_second_look(const npd_maint_screen_t &S, const npd_real_t *f64c, size_t N, size_t p, int k, double t) {
  npd_real_t *f64 = const_cast<npd_real_t *>(f64c);
  npb_pump_t pm;      /* only the members npd_maint_values reads are loaded */
#define NPD_PM(member) pm.member = NPD_F64_COL(PUMP, npb_pump_t, member, k)
  NPD_PM(oil_level); NPD_PM(oil_contamination); NPD_PM(lubrication_effectiveness); NPD_PM(wear_impeller); NPD_PM(cavitation_damage);
  NPD_PM(cavitation_intensity); NPD_PM(npsh_available); NPD_PM(wear_motor_bearings); NPD_PM(wear_pump_bearings); NPD_PM(wear_thrust_bearing);
  NPD_PM(wear_mechanical_seals); NPD_PM(vibration_level); NPD_PM(oil_temperature); NPD_PM(motor_temperature); NPD_PM(seal_leakage_rate);
#undef NPD_PM
  double values[NPB_MAINT_NPARAM];
  npd_maint_values(&pm, values);
  uint32_t hits = 0;
#pragma unroll
  for (int q = 0; q < NPB_MAINT_NPARAM; q++) {
    const double v = values[q], thr = S.threshold[q];
    const bool near_eq = fabs(v - thr) < 0.001;                                  /* _check_threshold_condition */
    const bool hit = ((((S.want_gt >> q) & 1u) != 0) & (v > thr)) | ((((S.want_lt >> q) & 1u) != 0) & (v < thr)) |
                     ((((S.want_eq >> q) & 1u) != 0) & (v == thr)) | ((((S.want_near >> q) & 1u) != 0) & near_eq) |
                     ((((S.want_far >> q) & 1u) != 0) & !near_eq);
    hits |= (uint32_t)hit << q;
  }
  bool work = false;
  if (__any(hits != 0)) {
#pragma unroll
    for (int q = 0; q < NPB_MAINT_NPARAM; q++) {
      const double lv = (double)*(const npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(k, last_violation_time, q));
      const bool cooling = (lv >= 0.0) & (t - lv < S.cooldown_minutes[q]);        /* _is_threshold_in_cooldown */
      work |= (((hits >> q) & 1u) != 0) & !cooling;
    }
  }
  return work;
}
/* the first half of that look alone: bit q = row q of the table is crossed by pump k of this lane's plant, cooldowns aside (npb_maint_all_kernel) */
__device__ __forceinline__ uint32_t npd_maint_crossed_rows(const npd_maint_screen_t &S, const npd_real_t *f64c, size_t N, size_t p, int k) {
  npd_real_t *f64 = const_cast<npd_real_t *>(f64c);
  npb_pump_t pm;
#define NPD_PM(member) pm.member = NPD_F64_COL(PUMP, npb_pump_t, member, k)
  NPD_PM(oil_level); NPD_PM(oil_contamination); NPD_PM(lubrication_effectiveness); NPD_PM(wear_impeller); NPD_PM(cavitation_damage);
  NPD_PM(cavitation_intensity); NPD_PM(npsh_available); NPD_PM(wear_motor_bearings); NPD_PM(wear_pump_bearings); NPD_PM(wear_thrust_bearing);
  NPD_PM(wear_mechanical_seals); NPD_PM(vibration_level); NPD_PM(oil_temperature); NPD_PM(motor_temperature); NPD_PM(seal_leakage_rate);
#undef NPD_PM
  double values[NPB_MAINT_NPARAM];
  npd_maint_values(&pm, values);
  uint32_t hits = 0;
#pragma unroll
  for (int q = 0; q < NPB_MAINT_NPARAM; q++) {
    const double v = values[q], thr = S.threshold[q];
    const bool near_eq = fabs(v - thr) < 0.001;                                  /* _check_threshold_condition */
    const bool hit = ((((S.want_gt >> q) & 1u) != 0) & (v > thr)) | ((((S.want_lt >> q) & 1u) != 0) & (v < thr)) |
                     ((((S.want_eq >> q) & 1u) != 0) & (v == thr)) | ((((S.want_near >> q) & 1u) != 0) & near_eq) |
                     ((((S.want_far >> q) & 1u) != 0) & !near_eq);
    hits |= (uint32_t)hit << q;
  }
  return hits;
}
/* the cooldown cache of the step kernels' screen (npd_maintenance.h) for the four pumps of this lane's plant, from the stamps as
 * they are now: whenever the rule has looked at a wave */
__device__ __forceinline__ void npd_maint_refresh_cache(const npd_maint_screen_t &S, npd_u32x4 *cache_entry, const npd_real_t *f64c, size_t N, size_t p, double t) {
  npd_real_t *f64 = const_cast<npd_real_t *>(f64c);
  const uint32_t scan_mask = S.want_gt | S.want_lt | S.want_eq | S.want_near | S.want_far;
#pragma unroll 1
  for (int k = 0; k < NPB_NUM_PUMPS; k++) {
    double lv[NPB_MAINT_NPARAM];
#pragma unroll
    for (int q = 0; q < NPB_MAINT_NPARAM; q++) lv[q] = (double)*(const npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(k, last_violation_time, q));
    uint32_t mask; float until;
    npd_maint_cache_entry(lv, S.cooldown_minutes, scan_mask, t, &mask, &until);
    uint32_t *e = (uint32_t *)(cache_entry + p * 2) + 2 * k;
    e[0] = mask; e[1] = __float_as_uint(until);
  }
}
/* ---- the two pump bodies of the rule as npd_maint_all_rule uses them.  They are npd_maint_rule_for_wave's own statements, and a change to
 * one belongs in the other: calling these helpers from npd_maint_rule_for_wave was tried and changes the code the compiler emits for every
 * npb_step*_maint_kernel and every instantiation of the rule (tools/compare_step_kernels.py), which the step kernels must not.
 * A due order (pump `pick`, action `pick_action`, number `best`) is carried out: closed, its handler run, the diagnostics flags set; with the
 * log on, ev takes the order as the arena holds it before it is closed */
__device__ __forceinline__ void npd_maint_carry_out_pump_order(const npb_params_t &P, const npd_maint_cache_t &MC, npd_real_t *f64, size_t N, size_t p, int pick,
                                                               int pick_action, double best, bool log_on, npb_maint_t &m, npb_maint_event_t &ev) {
  npb_mpump_t mp;
  NPD_MP_LOAD(pick, wo_order, NPB_MAINT_NACT); NPD_MP_LOAD(pick, wo_planned_start, NPB_MAINT_NACT);
  mp.wo_bearing = (double)*(const npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(pick, wo_bearing, 0));
  if (log_on) {      /* the order as the arena holds it, before it is closed */
    ev.created = (double)*(const npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(pick, last_trigger_time, pick_action));
    ev.planned_start = (double)*(const npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(pick, wo_planned_start, pick_action));
    ev.order = (int32_t)best; ev.action = (uint8_t)pick_action;
    ev.bearing = pick_action == NPB_MA_BEARING_REPLACEMENT ? (uint8_t)mp.wo_bearing : 0;
  }
  const int bearing = npd_maint_close_order(&mp, &m, pick_action);
  NPD_MP_STORE(pick, wo_order, NPB_MAINT_NACT); NPD_MP_STORE(pick, wo_planned_start, NPB_MAINT_NACT);
  *(npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(pick, wo_bearing, 0)) = (npd_real_t)mp.wo_bearing;
  npb_pump_t pm;
  NPD_LOAD(PUMP, npb_pump_t, pm, pick);
  npd_maint_execute(&pm, &P, pick_action, bearing);
  NPD_STORE(PUMP, npb_pump_t, pm, pick);
  if (MC.diag && ((NPD_MA_HANDLER_MASK >> pick_action) & 1u)) {    /* pump_lubrication.py:642-643, 1636-1637: the flags of this step's state-log row (action types the dispatcher knows) */
    MC.diag[(size_t)(NPB_DIAG_PUMP_MAINTENANCE_OCCURRED + pick) * MC.diag_pitch + p] = 1.0;
    if (pick_action == NPB_MA_OIL_TOP_OFF) MC.diag[(size_t)(NPB_DIAG_PUMP_OIL_TOP_OFF_OCCURRED + pick) * MC.diag_pitch + p] = 1.0;
    MC.diag[(size_t)(NPB_DIAG_PUMP_MAINTENANCE_ACTION + pick) * MC.diag_pitch + p] = (double)(pick_action + 1);
  }
}
/* the scan of pump k with the work order it may create, stored and logged (at most one creation per pump, plant and step) */
__device__ __forceinline__ void npd_maint_scan_pump_logged(const npd_maint_rule_consts_t *RC, npd_real_t *f64, size_t N, size_t p, int k, double t, bool log_on,
                                                           bool live, npb_maint_t &m, npb_maint_event_t &ev, int &dirty) {
  const npb_params_t &P = RC->P; const npb_maint_table_t &T = RC->T;
    npb_pump_t pm;
    NPD_LOAD(PUMP, npb_pump_t, pm, k);
    npb_mpump_t mp;
    NPD_LOAD(MPUMP, npb_mpump_t, mp, k);
    const int created_before = m.work_orders_created;
    if (npd_maint_scan_pump(&mp, &m, &P, &T, &pm, t)) {
      dirty = 1;
      if (log_on && m.work_orders_created != created_before) {    /* a work order was created: the action whose wo_order is the new count */
        const double n = (double)m.work_orders_created;
        ev.action = 0; ev.planned_start = 0.0;
#pragma unroll
        for (int a = 0; a < NPB_MAINT_NACT; a++)
          if (mp.wo_order[a] == n) { ev.action = (uint8_t)a; ev.planned_start = (double)(npd_real_t)mp.wo_planned_start[a]; }
        /* the rows this scan stamped (the arena still holds the stamps from before it) and the batched event's priority, their highest */
        uint32_t trigger = 0; int priority = 0;
#pragma unroll
        for (int q = 0; q < NPB_MAINT_NPARAM; q++)
          if (mp.last_violation_time[q] != (double)*(const npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(k, last_violation_time, q))) {
            trigger |= 1u << q; priority = T.priority[q] > priority ? T.priority[q] : priority;
          }
        ev.created = t; ev.order = m.work_orders_created; ev.trigger = (uint16_t)trigger; ev.priority = (uint8_t)priority;
        ev.bearing = ev.action == NPB_MA_BEARING_REPLACEMENT ? (uint8_t)mp.wo_bearing : 0;
      }
      NPD_STORE(MPUMP, npb_mpump_t, mp, k);
    }
    if (log_on) {    /* at most one creation per pump, plant and step */
      ev.kind = NPB_MAINT_EVENT_CREATED; ev.pump = (uint8_t)k;
      npd_maint_log(RC->L, live && m.work_orders_created != created_before, ev);
    }
}
/* one wave = the 64 plants p - lane .. p - lane + 63, whose step (all its stores) is complete.  hit_bits: bit k = the screen
 * flagged pump k for some lane; due_with_orders: some lane's check falls on open orders (wave-uniform both) */
/* WHO: one instantiation per calling kernel, so that each inherits its caller's register budget (the build of the two-wave
 * kernel that shares a SIMD between two waves must not be dragged to one wave per SIMD by a callee with the whole file) */
template <int WHO>
__device__ __attribute__((noinline)) void npd_maint_rule_for_wave(const npd_maint_rule_consts_t *RC, npd_maint_cache_t MC, npd_real_t *f64, size_t N, size_t p,
                                                                 unsigned hit_bits, unsigned due_with_orders) {
  const npb_params_t &P = RC->P; const npb_maint_table_t &T = RC->T; const npd_maint_screen_t &S = RC->S;
  const double t = NPD_F64_COL(PRIM, npb_prim_t, sim_time, 0);
  /* look properly, pump by pump, before anything heavy is fetched: the screen's bit k says "something may be new at pump k for some
   * plant of the wave"; the second look says whether the scan below would record a violation there (npd_maint_scan_pump returns
   * without touching anything when no threshold is crossed outside its cooldown), so a pump without one is not scanned at all --
   * the pump and mpump sections are ~140 columns per pump, the second look 15 */
  unsigned scan_bits = 0;
#pragma unroll 1
  for (int k = 0; k < NPB_NUM_PUMPS; k++) {
    if (((hit_bits >> k) & 1u) && __any(npd_maint_second_look(S, f64, N, p, k, t))) scan_bits |= 1u << k;
  }
  if (!due_with_orders && !scan_bits) { npd_maint_refresh_cache(S, MC.entry, f64, N, p, t); return; }
  npb_maint_t m;
  NPD_LOAD(MAINT, npb_maint_t, m, 0);
  int dirty = 0, executed = -1;      /* executed: the pump this lane's plant has just maintained (its readings have moved: scanned in any case) */
  const bool log_on = RC->L.cursor != nullptr, live = p < (size_t)MC.n_plants;    /* padding lanes never log */
  npb_maint_event_t ev = {};         /* the event log's record of this lane (npb_set_maintenance_log) */
  ev.time = t; ev.plant = (int32_t)p;
  /* ---- AutoMaintenanceSystem.update: one due order, the earliest created, is carried out */
  if (npd_maint_check_due(&m, &P, t)) {
    dirty = 1;
    if (m.work_orders_created > m.maintenance_actions_performed) {      /* some order is open */
      double best = 0.0; int pick = -1, pick_action = -1;
#pragma unroll 1
      for (int k = 0; k < NPB_NUM_PUMPS; k++) {
        npb_mpump_t mp;
        NPD_MP_LOAD(k, wo_order, NPB_MAINT_NACT); NPD_MP_LOAD(k, wo_planned_start, NPB_MAINT_NACT);
        int a; const double o = npd_maint_first_due(&mp, t, &a);
        if (o > 0.0 && (best == 0.0 || o < best)) { best = o; pick = k; pick_action = a; }
      }
      if (pick >= 0) {
        npb_mpump_t mp;
        NPD_MP_LOAD(pick, wo_order, NPB_MAINT_NACT); NPD_MP_LOAD(pick, wo_planned_start, NPB_MAINT_NACT);
        mp.wo_bearing = (double)*(const npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(pick, wo_bearing, 0));
        if (log_on) {      /* the order as the arena holds it, before it is closed */
          ev.created = (double)*(const npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(pick, last_trigger_time, pick_action));
          ev.planned_start = (double)*(const npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(pick, wo_planned_start, pick_action));
          ev.order = (int32_t)best; ev.action = (uint8_t)pick_action;
          ev.bearing = pick_action == NPB_MA_BEARING_REPLACEMENT ? (uint8_t)mp.wo_bearing : 0;
        }
        const int bearing = npd_maint_close_order(&mp, &m, pick_action);
        NPD_MP_STORE(pick, wo_order, NPB_MAINT_NACT); NPD_MP_STORE(pick, wo_planned_start, NPB_MAINT_NACT);
        *(npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(pick, wo_bearing, 0)) = (npd_real_t)mp.wo_bearing;
        npb_pump_t pm;
        NPD_LOAD(PUMP, npb_pump_t, pm, pick);
        npd_maint_execute(&pm, &P, pick_action, bearing);
        NPD_STORE(PUMP, npb_pump_t, pm, pick);
        executed = pick;
        if (MC.diag && ((NPD_MA_HANDLER_MASK >> pick_action) & 1u)) {    /* pump_lubrication.py:642-643, 1636-1637: the flags of this step's state-log row (action types the dispatcher knows) */
          MC.diag[(size_t)(NPB_DIAG_PUMP_MAINTENANCE_OCCURRED + pick) * MC.diag_pitch + p] = 1.0;
          if (pick_action == NPB_MA_OIL_TOP_OFF) MC.diag[(size_t)(NPB_DIAG_PUMP_OIL_TOP_OFF_OCCURRED + pick) * MC.diag_pitch + p] = 1.0;
          MC.diag[(size_t)(NPB_DIAG_PUMP_MAINTENANCE_ACTION + pick) * MC.diag_pitch + p] = (double)(pick_action + 1);
        }
      }
    }
  }
  if (log_on) {      /* at most one completion per plant and step */
    ev.kind = NPB_MAINT_EVENT_COMPLETED; ev.pump = (uint8_t)(executed < 0 ? 0 : executed);
    npd_maint_log(RC->L, live && executed >= 0, ev);
  }
  /* ---- StateManager.collect_states: threshold scan, one orchestrated event per pump (after the work above, as the
   * reference orders it) */
#pragma unroll 1
  for (int k = 0; k < NPB_NUM_PUMPS; k++) {
    if (!((scan_bits >> k) & 1u) && !__any(executed == k)) continue;
    npb_pump_t pm;
    NPD_LOAD(PUMP, npb_pump_t, pm, k);
    npb_mpump_t mp;
    NPD_LOAD(MPUMP, npb_mpump_t, mp, k);
    const int created_before = m.work_orders_created;
    if (npd_maint_scan_pump(&mp, &m, &P, &T, &pm, t)) {
      dirty = 1;
      if (log_on && m.work_orders_created != created_before) {    /* a work order was created: the action whose wo_order is the new count */
        const double n = (double)m.work_orders_created;
        ev.action = 0; ev.planned_start = 0.0;
#pragma unroll
        for (int a = 0; a < NPB_MAINT_NACT; a++)
          if (mp.wo_order[a] == n) { ev.action = (uint8_t)a; ev.planned_start = (double)(npd_real_t)mp.wo_planned_start[a]; }
        /* the rows this scan stamped (the arena still holds the stamps from before it) and the batched event's priority, their highest */
        uint32_t trigger = 0; int priority = 0;
#pragma unroll
        for (int q = 0; q < NPB_MAINT_NPARAM; q++)
          if (mp.last_violation_time[q] != (double)*(const npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(k, last_violation_time, q))) {
            trigger |= 1u << q; priority = T.priority[q] > priority ? T.priority[q] : priority;
          }
        ev.created = t; ev.order = m.work_orders_created; ev.trigger = (uint16_t)trigger; ev.priority = (uint8_t)priority;
        ev.bearing = ev.action == NPB_MA_BEARING_REPLACEMENT ? (uint8_t)mp.wo_bearing : 0;
      }
      NPD_STORE(MPUMP, npb_mpump_t, mp, k);
    }
    if (log_on) {    /* at most one creation per pump, plant and step */
      ev.kind = NPB_MAINT_EVENT_CREATED; ev.pump = (uint8_t)k;
      npd_maint_log(RC->L, live && m.work_orders_created != created_before, ev);
    }
  }
  if (dirty) {
    NPD_STORE(MAINT, npb_maint_t, m, 0);
    if (MC.counts && p < (size_t)MC.n_plants) MC.counts[p] = m.maintenance_actions_performed;
  }
  npd_maint_refresh_cache(S, MC.entry, f64, N, p, t);
}
/* the same rule as a launch of its own, every wave looked at in full: for the modes whose step kernels do not step the pumps
 * (primary-only, primary + steam generators), where nothing has screened anything */
__global__ __launch_bounds__(NPB_WAVE) void npb_maint_kernel(const npd_maint_rule_consts_t *RC, npd_maint_cache_t MC, size_t N, npd_real_t *__restrict__ f64) {
  NPD_SEGMENT(f64, N, (size_t)blockIdx.x * NPB_WAVE);
  npd_maint_rule_for_wave<0>(RC, MC, f64, N, (size_t)blockIdx.x * NPB_WAVE + threadIdx.x, 0xFu, 1u);
}

#define NPD_SM 1          /* store mode of the kernels below (npd_store_real): the one-wave kernel's own 8-byte stores ... */
#define NPD_STEP1_KERNEL npb_step_kernel
#define NPD_STEP1_MAINT 0
#define NPD_STEP1_WHO 1
#include "npd_step1.h"
#undef NPD_STEP1_KERNEL
#undef NPD_STEP1_MAINT
/* the same with the automatic maintenance compiled in (what npb_step launches when params.maint_enabled) */
#define NPD_STEP1_KERNEL npb_step_maint_kernel
#define NPD_STEP1_MAINT 1
#include "npd_step1.h"
#undef NPD_STEP1_KERNEL
/* the same step with the step-internal diagnostics written (npb_set_diagnostics): for state logging, not for throughput */
#define NPD_STEP1_KERNEL npb_step_diag_kernel
#undef NPD_STEP1_WHO
#define NPD_STEP1_WHO 2
#define NPD_STEP1_DIAG
#include "npd_step1.h"
#undef NPD_STEP1_DIAG
#undef NPD_STEP1_KERNEL
#undef NPD_STEP1_MAINT
/* ... with the non-temporal bit in this one, for batches whose sweep is far past the 256 MB Infinity Cache: nothing a step writes is still
 * cached when the next step reads it, and stores that do not allocate leave the caches to the loads (131 072 plants: 0.218 ->
 * 0.196 ms; at 65 536, where a tenth of the arena still hits, they cost 4 %: profiles/r2_ab_streaming_state_stores.txt) */
#undef NPD_SM
#define NPD_SM 2
#define NPD_STEP1_KERNEL npb_step_nt_kernel
#define NPD_STEP1_MAINT 0
#undef NPD_STEP1_WHO
#define NPD_STEP1_WHO 3
#include "npd_step1.h"
#undef NPD_STEP1_KERNEL
#undef NPD_STEP1_MAINT
#define NPD_STEP1_KERNEL npb_step_nt_maint_kernel
#define NPD_STEP1_MAINT 1
#include "npd_step1.h"
#undef NPD_STEP1_KERNEL
#undef NPD_STEP1_MAINT
#undef NPD_SM
#define NPD_SM 0          /* ... and the two-wave kernels leave theirs to the compiler */

#include "npd_step2.h"
#include "npd_step4.h"

/* get_observation() of one plant from the arena as it stands (sim.py:290-333), in each of the three modes; f64 / N already moved to
 * the plant's segment */
__device__ __forceinline__ void npd_observe_row(int mode, npd_real_t *f64, size_t N, size_t p, double *obs) {
  npb_prim_t s;
  NPD_LOAD(PRIM, npb_prim_t, s, 0);
  npd_obs_primary(s, obs);
  if (mode == NPB_MODE_PRIMARY) {   /* sim.py:333: twelve values */
#pragma unroll
    for (int k = 12; k < NPB_OBS_DIM; k++) obs[k] = 0.0;
    return;
  }
  double fwf, fwp; int fwa;
  if (mode == NPB_MODE_PRIMARY_SG) { fwf = NPD_F64_COL(SEC, npb_sec_t, total_feedwater_flow, 0); fwp = 0.0; fwa = 1; }
  else {
    fwf = NPD_F64_COL(FW, npb_fw_t, total_flow_rate, 0);
    fwp = NPD_F64_COL(FW, npb_fw_t, total_power_consumption, 0);
    fwa = NPD_I32_COL(FW, npb_fw_t, system_availability, 0) != 0;
  }
  npd_obs_secondary(obs, s.steam_flow_rate, NPD_F64_COL(SEC, npb_sec_t, electrical_power_output, 0), NPD_F64_COL(SEC, npb_sec_t, thermal_efficiency, 0),
                    NPD_F64_COL(SEC, npb_sec_t, total_steam_flow, 0), NPD_F64_COL(SEC, npb_sec_t, load_demand, 0),
                    NPD_F64_COL(SEC, npb_sec_t, cooling_water_temperature, 0), fwf, fwp, (double)fwa);
}

/* get_observation() without stepping (after reset / set_field): sim.py:290-333 */
__global__ __launch_bounds__(NPB_WAVE) void npb_observe_kernel(int mode, int n_plants, size_t N, const npd_real_t *__restrict__ f64c,
                                                               double *__restrict__ obs_out) {
  __shared__ double lds[NPB_WAVE * NPB_OBS_PAD];
  npd_real_t *f64 = const_cast<npd_real_t *>(f64c);
  const size_t block_base = (size_t)blockIdx.x * NPB_WAVE;
  NPD_SEGMENT(f64, N, block_base);
  double obs[NPB_OBS_DIM];
  npd_observe_row(mode, f64, N, block_base + threadIdx.x, obs);
  npd_store_rows<NPB_OBS_DIM>(obs, obs_out, lds, block_base, (size_t)n_plants);
}

/* ---- episodes: restore from the handle's snapshot arena (npb_snapshot / npb_restore) or from a start bank (npb_set_start_bank /
 * npb_restore_bank), and same-step autoreset after npb_step (npb_set_autoreset).  Either source is an arena in a handle's own layout
 * (segments, pitch, storage type; npb_source_t): restoring a plant is a copy of one lane of every column, nothing is decoded. */
#ifdef NPB_BUILD_F32
typedef uint32_t npd_word_t;
#else
typedef uint64_t npd_word_t;
#endif
/* where the restore writes besides the arena: the maintenance screen's cooldown cache (zeroed = "look", npd_maintenance.h) and the
 * caller's event-count column (npb_set_maintenance_count_buffer), both NULL unless params.maint_enabled */
struct npd_restore_side_t { npd_u32x4 *maint_entry; int32_t *maint_counts; int n_plants;
                             npb_side_restore_t cm;        /* the side state of the component maintenance (npd_component_auto.h): live NULL = off */
                             npb_side_restore_t dg;        /* the carried diagnostics rows (npb_carry_diagnostics): live NULL = not carried */ };
/* the bank entry a restored plant takes from its slot, and the slot and start columns it leaves behind (include/npb.h) */
__device__ __forceinline__ int32_t npd_bank_take(const npb_source_t &B, size_t p) {
  int32_t s = B.next_slot[p] % B.M;
  if (s < 0) s += B.M;                  /* ((next % M) + M) % M, for any value the caller wrote */
  B.next_slot[p] = (int32_t)(((uint32_t)s + (uint32_t)B.advance) % (uint32_t)B.M);    /* s, advance < 2^31: no wrap */
  if (B.episode_start) B.episode_start[p] = s;
  B.start[p] = s;
  return s;
}
/* the wave's plants with `reset` set from entry s of the source (the snapshot: s = p; a bank: the entry the plant took); f64 / N
 * already moved to the wave's segment, the source is moved per lane through its own pitch and segment.  Only reset lanes load and
 * store: a wave whose 64 plants all reset from the snapshot moves 512 B per column and direction, coalesced; one with a single reset
 * plant touches one line per column, and so does every lane of a bank restore, whose neighbouring lanes generally read different
 * entries.  The copy is latency-bound, so the loads of U columns are issued before their stores */
__device__ __forceinline__ void npd_restore_lanes(npd_real_t *__restrict__ f64, size_t N, size_t p, bool reset, const npb_source_t &src, size_t s,
                                                  const npd_restore_side_t &R) {
  if (!reset) return;
  const npd_real_t *from = (const npd_real_t *)src.arena;
  size_t Ns = src.N;
  NPD_SEGMENT(from, Ns, s);
  npd_word_t *dst = reinterpret_cast<npd_word_t *>(f64) + p;
  const npd_word_t *in = reinterpret_cast<const npd_word_t *>(from) + s;
  constexpr int U = 32;
#pragma unroll 1
  for (int c0 = 0; c0 < NPD_ARENA_COLS; c0 += U) {
    npd_word_t v[U];
#pragma unroll
    for (int u = 0; u < U; u++)
      if (c0 + u < NPD_ARENA_COLS) v[u] = __builtin_nontemporal_load(&in[(size_t)(c0 + u) * Ns]);
#pragma unroll
    for (int u = 0; u < U; u++)
      if (c0 + u < NPD_ARENA_COLS) dst[(size_t)(c0 + u) * N] = v[u];
  }
  if (R.maint_entry) {                /* the cooldowns of the restored stamps are unknown to the cache: look */
    const npd_u32x4 zero = {0u, 0u, 0u, 0u};
    R.maint_entry[p * 2] = zero; R.maint_entry[p * 2 + 1] = zero;
  }
  if (R.maint_counts && p < (size_t)R.n_plants) {
    int32_t *counts = R.maint_counts + p;
    const npd_real_t *f64 = from;     /* (the member macro reads `f64`, `N` and `p`: the source entry's) */
    const size_t N = Ns, p = s;
    *counts = NPD_I32_COL(MAINT, npb_maint_t, maintenance_actions_performed, 0);
  }
  if (R.cm.live) {                    /* the stamps and open orders of the generators and the condenser travel with the plant's */
#pragma unroll 1
    for (int k = 0; k < NPB_CMAINT_SIDE_DOUBLES; k++) R.cm.live[(size_t)k * R.cm.pitch + p] = R.cm.src[(size_t)k * R.cm.src_pitch + s];
  }
  if (R.dg.live) {                    /* the rows the diagnostics build carries in the caller's buffer (include/npb.h NPB_DIAG_CARRIED): p is the
                                       * global plant number, which is how that unsegmented buffer is indexed; the loads first */
    double v[NPB_DIAG_NUM_CARRIED];
#pragma unroll
    for (int k = 0; k < NPB_DIAG_NUM_CARRIED; k++) v[k] = R.dg.src[(size_t)k * R.dg.src_pitch + s];
    int k = 0;
#define NPB__X(row, fresh) R.dg.live[(size_t)(row) * R.dg.pitch + p] = v[k++];
    NPB_DIAG_CARRIED(NPB__X)
#undef NPB__X
  }
}
/* [64][W] rows held one per lane -> row-major global memory, only the rows whose bit is set in `rows` (npd_store_rows otherwise) */
template <int W>
__device__ __forceinline__ void npd_store_rows_masked(const double *row, double *__restrict__ out, double *lds, size_t block_base, uint64_t rows) {
  const int lane = threadIdx.x;
#pragma unroll
  for (int j = 0; j < W; j++) lds[lane * NPB_OBS_PAD + j] = row[j];
  NPD_LDS_DRAIN();
#pragma unroll
  for (int k = 0; k < W; k++) {
    const int idx = k * NPB_WAVE + lane, r = idx / W, c = idx % W;
    if ((rows >> r) & 1u) out[block_base * W + idx] = lds[r * NPB_OBS_PAD + c];
  }
  NPD_LDS_DRAIN();
}
/* the episode bookkeeping of one step, after the step kernel (and the maintenance kernel) on the same stream */
struct npd_episode_t {
  int32_t *len; double *ret;                                  /* carried: steps and summed reward of the running episode */
  int32_t *index; int32_t *out_index;                         /* carried: the running episode's number; the caller's column of it, or NULL */
  int32_t *out_len; double *out_ret; uint8_t *out_truncated; double *final_obs;   /* the caller's columns, each may be NULL */
  int max_steps;                                              /* 0 = no limit */
};
/* src: the snapshot, or a bank with its slots (then it also hands out the bank entry of each plant's episode as of this step) */
__global__ __launch_bounds__(NPB_WAVE) void npb_episode_kernel(int mode, int n_plants, size_t N, npd_real_t *__restrict__ f64, npb_source_t src,
                                                               const uint8_t *__restrict__ done, const double *__restrict__ reward, double *__restrict__ obs_out,
                                                               npd_episode_t E, npd_restore_side_t R) {
  __shared__ double lds[NPB_WAVE * NPB_OBS_PAD];
  const size_t block_base = (size_t)blockIdx.x * NPB_WAVE;
  NPD_SEGMENT(f64, N, block_base);
  const size_t p = block_base + threadIdx.x;
  bool reset = false;
  if (p < (size_t)n_plants) {
    const bool terminated = done[p] != 0;
    const int32_t len = E.len[p] + 1;
    const double ret = reward ? E.ret[p] + reward[p] : E.ret[p];
    const bool truncated = E.max_steps > 0 && len >= E.max_steps && !terminated;     /* termination wins */
    reset = terminated || truncated;
    if (E.out_len) E.out_len[p] = len;
    if (E.out_ret) E.out_ret[p] = ret;
    if (E.out_truncated) E.out_truncated[p] = (uint8_t)truncated;
    if (src.out_start) src.out_start[p] = src.start[p];      /* the episode this step's transition belonged to */
    if (E.out_index) E.out_index[p] = E.index[p];
    if (reset) E.index[p] += 1;
    E.len[p] = reset ? 0 : len;
    E.ret[p] = reset ? 0.0 : ret;
  }
  if (!__any(reset)) return;
  const uint64_t rows = __ballot(reset);
  if (obs_out && E.final_obs) {     /* the terminal observation: this step's row, before it is replaced */
#pragma unroll
    for (int k = 0; k < NPB_OBS_DIM; k++) {
      const int idx = k * NPB_WAVE + threadIdx.x;
      if ((rows >> (idx / NPB_OBS_DIM)) & 1u) E.final_obs[block_base * NPB_OBS_DIM + idx] = obs_out[block_base * NPB_OBS_DIM + idx];
    }
  }
  const size_t s = reset && src.next_slot ? (size_t)npd_bank_take(src, p) : p;
  npd_restore_lanes(f64, N, p, reset, src, s, R);
  if (obs_out) {
    double obs[NPB_OBS_DIM];
    npd_observe_row(mode, f64, N, p, obs);
    npd_store_rows_masked<NPB_OBS_DIM>(obs, obs_out, lds, block_base, rows);
  }
}
/* npb_restore / npb_restore_bank: the lanes below `lanes` of mask (NULL = all of them) from the source, their episode counters (if
 * any) to zero */
__global__ __launch_bounds__(NPB_WAVE) void npb_restore_kernel(int lanes, size_t N, npd_real_t *__restrict__ f64, npb_source_t src,
                                                               const uint8_t *__restrict__ mask, int32_t *__restrict__ len, double *__restrict__ ret,
                                                               int32_t *__restrict__ index, npd_restore_side_t R) {
  const size_t block_base = (size_t)blockIdx.x * NPB_WAVE;
  NPD_SEGMENT(f64, N, block_base);
  const size_t p = block_base + threadIdx.x;
  const bool reset = p < (size_t)lanes && (!mask || mask[p] != 0);
  if (reset && len) { len[p] = 0; ret[p] = 0.0; index[p] += 1; }
  if (!__any(reset)) return;
  const size_t s = reset && src.next_slot ? (size_t)npd_bank_take(src, p) : p;
  npd_restore_lanes(f64, N, p, reset, src, s, R);
}

/* construction-time state for every plant selected by mask (NULL = all): the state the reference's
 * constructors leave behind with the default SecondarySystemConfig (npd_init.h) */
__global__ __launch_bounds__(NPB_WAVE) void npb_init_kernel(npb_params_t P, size_t N, npd_real_t *__restrict__ f64,
                                                            const uint8_t *__restrict__ mask,
                                                            int n_plants) {
  const size_t p = (size_t)blockIdx.x * NPB_WAVE + threadIdx.x;
  NPD_SEGMENT(f64, N, p);
  if (mask && p < (size_t)n_plants && !mask[p]) return;
  if (mask && p >= (size_t)n_plants) return;
  { npb_prim_t s; npd_prim_init(&s); NPD_STORE(PRIM, npb_prim_t, s, 0); }
#pragma unroll 1
  for (int i = 0; i < NPB_NUM_SG; i++) { npb_sg_t g; npd_sg_init(&g); NPD_STORE(SG, npb_sg_t, g, i); }
#pragma unroll 1
  for (int i = 0; i < NPB_NUM_PUMPS; i++) { npb_pump_t pm; npd_pump_init(&pm, i); NPD_STORE(PUMP, npb_pump_t, pm, i); }
  { npb_fw_t fw; npd_fw_init(&fw); NPD_STORE(FW, npb_fw_t, fw, 0); }
  { npb_turb_t t; npb_tstg_t g; npd_turb_init(&t, &g); NPD_STORE(TURB, npb_turb_t, t, 0); NPD_STORE(TSTG, npb_tstg_t, g, 0); }
#pragma unroll 1
  for (int i = 0; i < 2; i++) { npb_chem_t ch; npd_chem_init(&ch, i); NPD_STORE(CHEM, npb_chem_t, ch, i); }
  { npb_ph_t ph; npd_ph_init(&ph); NPD_STORE(PH, npb_ph_t, ph, 0); }
  { npb_cond_t cd; npd_cond_init(&cd); NPD_STORE(COND, npb_cond_t, cd, 0); }
  { npb_sec_t sec; npd_sec_init(&sec); NPD_STORE(SEC, npb_sec_t, sec, 0); }
  { npb_maint_t m; npd_maint_init(&m); NPD_STORE(MAINT, npb_maint_t, m, 0); }
#pragma unroll 1
  for (int i = 0; i < NPB_NUM_PUMPS; i++) { npb_mpump_t mp; npd_mpump_init(&mp); NPD_STORE(MPUMP, npb_mpump_t, mp, i); }
  (void)P;
}

/* NuclearPlantSimulator.reset(start_at_steady_state)  sim.py:546-581 for every plant selected by mask (NULL = all):
 * the reference's own reset semantics (npd_reset.h), which keep part of the plant's history -- unlike
 * npb_init_kernel, which stands in for constructing a new simulator.  The maint.* section is left alone (the
 * maintenance system is not reset; only the state manager's log is cleared, sim.py:573-574). */
__global__ __launch_bounds__(NPB_WAVE) void npb_reset_kernel(npb_params_t P, size_t N, npd_real_t *__restrict__ f64,
                                                             const uint8_t *__restrict__ mask, int n_plants, int steady) {
  const size_t p = (size_t)blockIdx.x * NPB_WAVE + threadIdx.x;
  NPD_SEGMENT(f64, N, p);
  if (mask && (p >= (size_t)n_plants || !mask[p])) return;
  { npb_prim_t s; NPD_LOAD(PRIM, npb_prim_t, s, 0); npd_prim_reset(&s); NPD_STORE(PRIM, npb_prim_t, s, 0); }
  npb_sec_t sec;
  NPD_LOAD(SEC, npb_sec_t, sec, 0);
  npd_sec_reset(&sec);
  npb_sg_t sg[NPB_NUM_SG];
  for (int i = 0; i < NPB_NUM_SG; i++) { NPD_LOAD(SG, npb_sg_t, sg[i], i); npd_sg_reset(&sg[i]); }
  npd_equilibrium_t eq;
  if (steady) {
    /* sim.py:558-563: primary_physics.thermal_power_mw was zeroed by reset_system, so the rated power is used */
    npd_steady_state_equilibrium(sg, &sec, &P, P.rated_power_mw, &eq);
    npd_sec_steady_state(&sec, &eq);
  }
  for (int i = 0; i < NPB_NUM_SG; i++) NPD_STORE(SG, npb_sg_t, sg[i], i);
  NPD_STORE(SEC, npb_sec_t, sec, 0);
#pragma unroll 1
  for (int i = 0; i < NPB_NUM_PUMPS; i++) {
    npb_pump_t pm;
    NPD_LOAD(PUMP, npb_pump_t, pm, i);
    npd_pump_reset(&pm, i);
    if (steady) npd_pump_steady_state(&pm, i, eq.steam_pressure, eq.feedwater_flow, eq.pumps_needed, eq.pump_speed);
    NPD_STORE(PUMP, npb_pump_t, pm, i);
  }
  { npb_fw_t fw; npd_fw_reset(&fw); NPD_STORE(FW, npb_fw_t, fw, 0); }
  {
    npb_turb_t t; npb_tstg_t g;
    NPD_LOAD(TURB, npb_turb_t, t, 0); NPD_LOAD(TSTG, npb_tstg_t, g, 0);
    npd_turb_reset(&t, &g, steady, steady ? eq.load_demand : 0.0, steady ? eq.electrical_power : 0.0);
    NPD_STORE(TURB, npb_turb_t, t, 0); NPD_STORE(TSTG, npb_tstg_t, g, 0);
  }
#pragma unroll 1
  for (int i = 0; i < 2; i++) { npb_chem_t ch; npd_chem_reset(&ch); NPD_STORE(CHEM, npb_chem_t, ch, i); }
  { npb_cond_t cd; NPD_LOAD(COND, npb_cond_t, cd, 0); npd_cond_reset(&cd); NPD_STORE(COND, npb_cond_t, cd, 0); }
  /* the pH controller and its pending doses are not reset (secondary/__init__.py:1041-1072 never touches them) */
}

/* operator-ordered maintenance (npb_perform_maintenance): FeedwaterPump.perform_maintenance(type, **kwargs) called by the user between
 * two steps (feedwater/pump_system.py:750 -> the lubrication system's dispatcher, pump_lubrication.py:625-674), for every plant whose
 * lane of the caller's columns orders one.  One wave per 64 plants.  The expected use is sparse -- a policy orders service for a
 * small share of the plants per step -- so a wave first reads its 64 orders (8 B per plant) and leaves when none can succeed; a wave
 * that stays visits the pumps somebody ordered, and only the ordering lanes load, change and store their pump section: a plant
 * without a successful order keeps its exact bits under either storage type because nothing is stored to it.  The work-order queue,
 * the maint.* / mpump.* sections and the counters are not touched (a direct call bypasses AutoMaintenanceSystem in the reference too). */
struct npd_operator_orders_t {
  const int32_t *action, *pump, *bearing;     /* the caller's [n_plants] columns; bearing NULL = NPB_BEARING_ALL */
  const double *target_level;                 /* [n_plants], NULL = 95.0: _perform_oil_top_off's default argument (pump_lubrication.py:710) */
  uint8_t *success;                           /* [n_plants] or NULL */
  int n_plants;
};
__global__ __launch_bounds__(NPB_WAVE) void npb_operator_maint_kernel(npd_operator_orders_t O, npd_maint_log_t L, size_t N, npd_real_t *__restrict__ f64) {
  const size_t p = (size_t)blockIdx.x * NPB_WAVE + threadIdx.x;
  const bool live = p < (size_t)O.n_plants;      /* the columns have n_plants elements, not the pitch */
  int action = -1, pump = 0;
  if (live) { action = O.action[p]; pump = O.pump[p]; }
  /* "Unknown maintenance type" (pump_lubrication.py:661-668): an action outside the catalog or without a handler; a pump that is none */
  bool ok = action >= 0 && action < NPB_MAINT_NACT && ((NPD_MA_HANDLER_MASK >> (action & 31)) & 1u) && pump >= 0 && pump < NPB_NUM_PUMPS;
  if (!__any(ok)) {
    if (live && O.success) O.success[p] = 0;
    return;
  }
  int bearing = NPB_BEARING_ALL;
  double target_level = 95.0;
  if (ok && O.bearing) bearing = O.bearing[p];
  if (ok && O.target_level) target_level = O.target_level[p];
  /* "Invalid bearing component" (:789-797); the other handlers take no component_id and ignore it */
  if (action == NPB_MA_BEARING_REPLACEMENT && (bearing < NPB_BEARING_ALL || bearing > NPB_BEARING_THRUST)) ok = false;
  if (live && O.success) O.success[p] = ok ? 1 : 0;
  NPD_SEGMENT(f64, N, (size_t)blockIdx.x * NPB_WAVE);
#pragma unroll 1
  for (int k = 0; k < NPB_NUM_PUMPS; k++) {
    const bool mine = ok && pump == k;
    if (!__any(mine)) continue;
    if (mine) {
      npb_pump_t pm;
      NPD_LOAD(PUMP, npb_pump_t, pm, k);
      npb_params_t P = {};      /* the handlers read one parameter: the top-off target, which here is the caller's argument */
      P.maint_top_off_target = target_level;
      npd_maint_execute(&pm, &P, action, bearing);
      NPD_STORE(PUMP, npb_pump_t, pm, k);
    }
  }
  if (L.cursor)
    npd_maint_log_operator(L, ok, p, NPD_F64_COL(PRIM, npb_prim_t, sim_time, 0), pump, action, NPB_MAINT_EVENT_OPERATOR,
                           action == NPB_MA_BEARING_REPLACEMENT ? bearing : 0);
}

/* operator-ordered maintenance of steam generators and condenser (npb_perform_component_maintenance): perform_maintenance(type, **kwargs)
 * of a steam generator, the steam-generator system, the condenser or a steam-jet ejector, called by the user between two steps
 * (npd_component_maintenance.h), for every plant whose lane of the caller's columns orders one.  The design of the pump kernel above:
 * one wave per 64 plants reads its 64 orders, writes success and leaves when none can succeed; a wave that stays visits the component
 * kinds and units somebody in it ordered, and only the ordering lanes load, change and store the sections their action touches --
 * one generator; the three generators one after the other (a system action) or the system's flags alone; the condenser, with its
 * chemistry for the water treatment.  Nothing is stored to a plant without a successful order. */
struct npd_component_orders_t {
  const int32_t *action, *unit, *option;      /* the caller's [n_plants] columns; unit NULL = 0, option NULL = NPB_CLEANING_DEFAULT */
  const double *amount;                       /* [n_plants] or NULL: tubes_to_plug; no handler of the catalog reads it */
  uint8_t *success;                           /* [n_plants] or NULL */
  int n_plants;
  unsigned kinds;                             /* bit k: the handle's mode carries component kind k (NPB_COMPONENT_*) */
};
__global__ __launch_bounds__(NPB_WAVE) void npb_operator_component_maint_kernel(npd_component_orders_t O, npd_maint_log_t L, size_t N, npd_real_t *__restrict__ f64) {
  const size_t p = (size_t)blockIdx.x * NPB_WAVE + threadIdx.x;
  const bool live = p < (size_t)O.n_plants;      /* the columns have n_plants elements, not the pitch */
  int action = -1, unit = 0;
  if (live) { action = O.action[p]; if (action >= 0 && O.unit) unit = O.unit[p]; }
  const int kind = npd_component_kind(action);
  if (kind == NPB_COMPONENT_SGSYS || kind == NPB_COMPONENT_COND) unit = 0;      /* one of each: the unit is ignored */
  /* "Unknown maintenance type": an index outside the catalog; a generator or ejector that is none; a component the mode does not carry */
  const bool ok = kind >= 0 && ((O.kinds >> kind) & 1u) && unit >= 0 && unit < NPB_COMPONENT_UNITS(kind);
  if (live && O.success) O.success[p] = ok ? 1 : 0;
  if (!__any(ok)) return;
  int option = NPB_CLEANING_DEFAULT;
  if (ok && O.option) option = O.option[p];
  NPD_SEGMENT(f64, N, (size_t)blockIdx.x * NPB_WAVE);
  const bool on_sg = ok && kind == NPB_COMPONENT_SG;
  const bool on_sgsys = ok && kind == NPB_COMPONENT_SGSYS;
  const bool on_sgs = on_sgsys && npd_sgsys_touches_generators(action);
  if (__any(on_sg || on_sgs)) {
    int cleaned = 0;
#pragma unroll 1
    for (int k = 0; k < NPB_NUM_SG; k++) {
      const bool mine = (on_sg && unit == k) || on_sgs;
      if (!__any(mine)) continue;
      if (mine) {
        npb_sg_t g;
        NPD_LOAD(SG, npb_sg_t, g, k);
        if (on_sg) npd_sg_maintenance(&g, action, option);
        else npd_sgsys_maintenance_sg(&g, action, &cleaned);
        NPD_STORE(SG, npb_sg_t, g, k);
      }
    }
  }
  if (__any(on_sgsys && !on_sgs)) {
    if (on_sgsys && !on_sgs) {
      npb_sec_t sec;
      NPD_LOAD(SEC, npb_sec_t, sec, 0);
      npd_sgsys_maintenance_sec(&sec, action);
      NPD_STORE(SEC, npb_sec_t, sec, 0);
    }
  }
  const bool on_cond = ok && (kind == NPB_COMPONENT_COND || kind == NPB_COMPONENT_EJECTOR);
  if (__any(on_cond)) {
    if (on_cond) {
      npb_cond_t cd;
      NPD_LOAD(COND, npb_cond_t, cd, 0);
      if (kind == NPB_COMPONENT_EJECTOR) {
#pragma unroll
        for (int e = 0; e < NPB_NUM_EJECTORS; e++)      /* a constant index: the section stays in registers */
          if (unit == e) npd_ejector_maintenance(&cd, e, action, option);
      } else if (npd_cond_touches_chemistry(action)) {
        npb_chem_t ch;      /* chem[1]: the condenser-owned WaterChemistry (include/npb_fields.h) */
        NPD_LOAD(CHEM, npb_chem_t, ch, 1);
        npd_cond_maintenance(&cd, &ch, action, option);
        NPD_STORE(CHEM, npb_chem_t, ch, 1);
      } else {
        npd_cond_maintenance(&cd, nullptr, action, option);
      }
      NPD_STORE(COND, npb_cond_t, cd, 0);
    }
  }
  if (L.cursor) npd_maint_log_operator(L, ok, p, NPD_F64_COL(PRIM, npb_prim_t, sim_time, 0), unit, action, NPB_MAINT_EVENT_OPERATOR_COMPONENT);
}

/* operator-ordered maintenance of the turbine (npb_perform_turbine_maintenance): perform_maintenance(type) of the turbine, one of its
 * bearings, its bearing-lubrication system or one of its stages, called by the user between two steps (npd_turbine_maintenance.h), for
 * every plant whose lane of the caller's columns orders one.  The design of the component kernel above: one wave per 64 plants reads
 * its 64 orders, writes success and leaves when none can succeed.  Orders on the turbine, a bearing and the lubrication system load,
 * change and store the turb section of the ordering lanes; an order on a stage touches that stage's three tstg columns and nothing else
 * (the section's other 67 columns are never loaded), the wave skipping the stages nobody in it ordered.  Nothing is stored to a plant
 * without a successful order. */
struct npd_turbine_orders_t {
  const int32_t *action, *unit;               /* the caller's [n_plants] columns; unit NULL = 0 */
  uint8_t *success;                           /* [n_plants] or NULL */
  int n_plants;
  int turbine;                                /* the handle's mode steps the turbine */
};
__global__ __launch_bounds__(NPB_WAVE) void npb_operator_turbine_maint_kernel(npd_turbine_orders_t O, npd_maint_log_t L, size_t N, npd_real_t *__restrict__ f64) {
  const size_t p = (size_t)blockIdx.x * NPB_WAVE + threadIdx.x;
  const bool live = p < (size_t)O.n_plants;      /* the columns have n_plants elements, not the pitch */
  int action = -1, unit = 0;
  if (live) { action = O.action[p]; if (action >= 0 && O.unit) unit = O.unit[p]; }
  const int kind = npd_turbine_kind(action);
  if (kind == NPB_TURBINE_SYSTEM || kind == NPB_TURBINE_LUBE) unit = 0;      /* one of each: the unit is ignored */
  /* "Unknown maintenance type": an index outside the catalog; a bearing or stage that is none; a thrust adjustment of a journal bearing;
   * a mode that steps no turbine */
  const bool ok = O.turbine && npd_turbine_order_ok(kind, action, unit);
  if (live && O.success) O.success[p] = ok ? 1 : 0;
  if (!__any(ok)) return;
  NPD_SEGMENT(f64, N, (size_t)blockIdx.x * NPB_WAVE);
  const bool on_turb = ok && kind != NPB_TURBINE_STAGE;
  if (__any(on_turb)) {
    if (on_turb) {
      npb_turb_t t;
      NPD_LOAD(TURB, npb_turb_t, t, 0);
      if (kind == NPB_TURBINE_SYSTEM) npd_turbine_system_maintenance(&t, action);
      else if (kind == NPB_TURBINE_LUBE) npd_turbine_lube_maintenance(&t, action);
      else {
#pragma unroll
        for (int b = 0; b < 4; b++)      /* a constant index: the section stays in registers */
          if (unit == b) npd_turbine_bearing_maintenance(&t, b, action);
      }
      NPD_STORE(TURB, npb_turb_t, t, 0);
    }
  }
  const bool on_stage = ok && kind == NPB_TURBINE_STAGE;
  if (__any(on_stage)) {
#pragma unroll 1
    for (int k = 0; k < 14; k++) {
      const bool mine = on_stage && unit == k;
      if (!__any(mine)) continue;
      if (mine) {      /* tstg has carried reals only: member slot = column within the section */
        npd_real_t *deg = (npd_real_t *)npd_gaddr(f64, N, p, NPD_SEC_COL(TSTG, 0) + NPB_F64_SLOT(npb_tstg_t, stage_efficiency_degradation) + k);
        npd_real_t *dep = (npd_real_t *)npd_gaddr(f64, N, p, NPD_SEC_COL(TSTG, 0) + NPB_F64_SLOT(npb_tstg_t, stage_deposit_thickness) + k);
        npd_real_t *wear = (npd_real_t *)npd_gaddr(f64, N, p, NPD_SEC_COL(TSTG, 0) + NPB_F64_SLOT(npb_tstg_t, stage_blade_wear_factor) + k);
        double efficiency_degradation = (double)*deg, deposit_thickness = (double)*dep, blade_wear_factor = (double)*wear;
        npd_turbine_stage_maintenance(&efficiency_degradation, &deposit_thickness, &blade_wear_factor, action);
        *deg = (npd_real_t)efficiency_degradation; *dep = (npd_real_t)deposit_thickness; *wear = (npd_real_t)blade_wear_factor;
      }
    }
  }
  if (L.cursor) npd_maint_log_operator(L, ok, p, NPD_F64_COL(PRIM, npb_prim_t, sim_time, 0), unit, action, NPB_MAINT_EVENT_OPERATOR_TURBINE);
}

/* ---- automatic maintenance of the feedwater pumps, the steam generators and the condenser in ONE queue (npb_set_component_maintenance;
 * npd_component_auto.h): a launch of its own behind the PLAIN step kernel, which is the step kernel of a handle without any automatic
 * maintenance -- the step kernels do not know this rule.  One wave = 64 plants.  The wave first screens: is a check due on open orders,
 * is a pump's threshold crossed outside its cooldown (npd_maint_second_look), is a component's; a wave with none of that moves
 * last_check_time where a check fell due and leaves.  Otherwise the reference's order: AutoMaintenanceSystem.update carries out one due
 * order, the earliest created of any component; then the scan in the order of StateManager.maintenance_thresholds, FWP-1..4, SG-0..2,
 * the condenser, every created order numbered from the one counter maint.work_orders_created. */
__device__ __forceinline__ void npd_cmaint_values(const npd_real_t *f64c, size_t N, size_t p, int c, double dt, double *v) {
  npd_real_t *f64 = const_cast<npd_real_t *>(f64c);
  if (c == NPB_CMAINT_COND) {
    v[0] = NPD_F64_COL(COND, npb_cond_t, total_fouling_resistance, 0);
    v[1] = npd_cond_tube_leak_rate(NPD_F64_COL(COND, npb_cond_t, vibration_damage, 0), NPD_F64_COL(COND, npb_cond_t, corrosion_damage, 0),
                                   NPD_F64_COL(CHEM, npb_chem_t, water_aggressiveness, 1), NPD_F64_COL(COND, npb_cond_t, active_tube_count, 0),
                                   dt / 60.0);      /* the condenser's dt: hours (npd_step1.h) */
    v[2] = 0.0;
    return;
  }
  v[0] = NPD_F64_COL(SG, npb_sg_t, tsp_fouling_fraction, c);
  v[1] = NPD_F64_COL(SG, npb_sg_t, tube_wall_temp, c);
  v[2] = NPD_F64_COL(SG, npb_sg_t, steam_quality, c);
}
/* everything behind the screen, as a real function call (noinline), so that the screen -- what nearly every wave of nearly every step
 * runs and leaves from -- is allocated for itself, not for the rule's registers and scratch: the pattern of npd_maint_rule_for_wave.
 * work: this lane's check is due on open orders; scan_bits: bit k = pump k, bit 4 + c = component c has something new for some lane */
__device__ __attribute__((noinline)) void npd_maint_all_rule(const npd_maint_rule_consts_t *RC, npd_cmaint_side_t side, npd_maint_cache_t MC, npd_real_t *f64,
                                                             size_t N, size_t p, double t, bool work, unsigned scan_bits) {
  const npb_params_t &P = RC->P; const npb_maint_table_t &T = RC->T;
  npb_maint_t m;
  NPD_LOAD(MAINT, npb_maint_t, m, 0);
  int dirty = 0, executed = -1, executed_comp = -1;
  const bool log_on = RC->L.cursor != nullptr, live = p < (size_t)MC.n_plants;    /* padding lanes never log */
  npb_maint_event_t ev = {};
  ev.time = t; ev.plant = (int32_t)p;
  /* ---- AutoMaintenanceSystem.update: one due order, the earliest created of pumps and components, is carried out.  (A lane whose
   * check fell due with nothing open has had its last_check_time moved by the screen; m holds that.) */
  if (work) {
    m.last_check_time = t;
    dirty = 1;
    double best = 0.0; int pick = -1, pick_action = -1;
#pragma unroll 1
    for (int k = 0; k < NPB_NUM_PUMPS; k++) {
      npb_mpump_t mp;
      NPD_MP_LOAD(k, wo_order, NPB_MAINT_NACT); NPD_MP_LOAD(k, wo_planned_start, NPB_MAINT_NACT);
      int a; const double o = npd_maint_first_due(&mp, t, &a);
      if (o > 0.0 && (best == 0.0 || o < best)) { best = o; pick = k; pick_action = a; }
    }
    int cslot; const double co = npd_cmaint_first_due(side, p, t, &cslot);
    if (co > 0.0 && (best == 0.0 || co < best)) { best = co; pick = -1; executed_comp = cslot / NPB_CMAINT_NROW; } else cslot = -1;
    if (pick >= 0) {      /* a pump's order */
      npd_maint_carry_out_pump_order(P, MC, f64, N, p, pick, pick_action, best, log_on, m, ev);
      ev.pump = (uint8_t)pick; ev.kind = NPB_MAINT_EVENT_COMPLETED;
      executed = pick;
    } else if (cslot >= 0) {      /* a component's: perform_maintenance(maintenance_type=action) with its default arguments */
      const int c = executed_comp;
      const int action = side.C->T.action[npd_cmaint_param0(c) + cslot % NPB_CMAINT_NROW];
      ev.created = NPD_CMS(side, NPB_CMS_WO_CREATED, cslot, p);
      ev.planned_start = NPD_CMS(side, NPB_CMS_WO_PLANNED_START, cslot, p);
      ev.priority = (uint8_t)NPD_CMS(side, NPB_CMS_WO_PRIORITY, cslot, p);
      ev.order = (int32_t)best; ev.action = (uint8_t)action; ev.pump = (uint8_t)(c == NPB_CMAINT_COND ? 0 : c);
      ev.bearing = (uint8_t)(c == NPB_CMAINT_COND ? NPB_COMPONENT_COND : NPB_COMPONENT_SG);
      ev.reserved = action == NPB_CA_AUTO_CONDENSER_TUBE_PLUGGING ? 0 : 1;      /* the one handler that raises: success = false */
      ev.kind = NPB_MAINT_EVENT_COMPONENT_COMPLETED;
      NPD_CMS(side, NPB_CMS_WO_ORDER, cslot, p) = 0.0; NPD_CMS(side, NPB_CMS_WO_CREATED, cslot, p) = 0.0;
      NPD_CMS(side, NPB_CMS_WO_PLANNED_START, cslot, p) = 0.0; NPD_CMS(side, NPB_CMS_WO_PRIORITY, cslot, p) = 0.0;
      m.maintenance_actions_performed += 1;      /* maint.executed[] counts the pumps' orders only (include/npb_fields.h) */
      if (c == NPB_CMAINT_COND) {
        npb_cond_t cd;
        NPD_LOAD(COND, npb_cond_t, cd, 0);
        if (action == NPB_CA_AUTO_CONDENSER_TUBE_PLUGGING) {      /* what the handler has done when it raises (condenser/physics.py:1236-1240, tubes_to_plug = 10) */
          const double old_active_count = cd.active_tube_count;
          cd.plugged_tube_count += 10;
          cd.active_tube_count = npd_pymax(1000.0, old_active_count - 10);
        } else if (npd_cond_touches_chemistry(action)) {
          npb_chem_t ch;
          NPD_LOAD(CHEM, npb_chem_t, ch, 1);
          npd_cond_maintenance(&cd, &ch, action, NPB_CLEANING_DEFAULT);
          NPD_STORE(CHEM, npb_chem_t, ch, 1);
        } else {
          npd_cond_maintenance(&cd, nullptr, action, NPB_CLEANING_DEFAULT);
        }
        NPD_STORE(COND, npb_cond_t, cd, 0);
      } else {
#pragma unroll 1
        for (int k = 0; k < NPB_NUM_SG; k++) {
          if (c != k) continue;
          npb_sg_t g;
          NPD_LOAD(SG, npb_sg_t, g, k);
          npd_sg_maintenance(&g, action, NPB_CLEANING_DEFAULT);
          NPD_STORE(SG, npb_sg_t, g, k);
        }
      }
    }
  }
  if (log_on) npd_maint_log(RC->L, live && (executed >= 0 || executed_comp >= 0), ev);      /* at most one completion per plant and step */
  ev.reserved = 0; ev.priority = 0;      /* (a component completion's success and priority: not the next records') */
  /* ---- StateManager.collect_states: the pumps ... */
#pragma unroll 1
  for (int k = 0; k < NPB_NUM_PUMPS; k++) {
    if (!((scan_bits >> k) & 1u) && !__any(executed == k)) continue;
    npd_maint_scan_pump_logged(RC, f64, N, p, k, t, log_on, live, m, ev, dirty);
  }
  /* ---- ... then the generators and the condenser */
#pragma unroll 1
  for (int c = 0; c < NPB_CMAINT_NCOMP; c++) {
    if (!((scan_bits >> (4 + c)) & 1u) && !__any(executed_comp == c)) continue;
    double v[NPB_CMAINT_NROW];
    npd_cmaint_values(f64, N, p, c, P.dt, v);
    const uint32_t viol = npd_cmaint_violations(side, p, c, v, t);
    int slot = -1, action = 0, priority = 0;
    if (viol) {
      slot = npd_cmaint_scan(side, p, c, viol, &m, &P, t, &action, &priority);
      if (slot >= 0) dirty = 1;
    }
    if (log_on) {
      ev = npb_maint_event_t{};
      ev.time = t; ev.plant = (int32_t)p; ev.created = t; ev.order = m.work_orders_created; ev.trigger = (uint16_t)viol;
      ev.planned_start = slot >= 0 ? NPD_CMS(side, NPB_CMS_WO_PLANNED_START, slot, p) : 0.0;
      ev.action = (uint8_t)action; ev.priority = (uint8_t)priority; ev.pump = (uint8_t)(c == NPB_CMAINT_COND ? 0 : c);
      ev.bearing = (uint8_t)(c == NPB_CMAINT_COND ? NPB_COMPONENT_COND : NPB_COMPONENT_SG);
      ev.kind = NPB_MAINT_EVENT_COMPONENT_CREATED;
      npd_maint_log(RC->L, live && slot >= 0, ev);
    }
  }
  if (dirty) {
    NPD_STORE(MAINT, npb_maint_t, m, 0);
    if (MC.counts && p < (size_t)MC.n_plants) MC.counts[p] = m.maintenance_actions_performed;
  }
}
__global__ __launch_bounds__(NPB_WAVE) void npb_maint_all_kernel(const npd_maint_rule_consts_t *RC, npd_cmaint_side_t side, npd_maint_cache_t MC, size_t N,
                                                                 npd_real_t *__restrict__ f64) {
  NPD_SEGMENT(f64, N, (size_t)blockIdx.x * NPB_WAVE);
  const size_t p = (size_t)blockIdx.x * NPB_WAVE + threadIdx.x;
  const npb_params_t &P = RC->P; const npb_maint_table_t &T = RC->T; const npd_maint_screen_t &S = RC->S;
  const double t = NPD_F64_COL(PRIM, npb_prim_t, sim_time, 0);
  /* ---- the screen */
  npd_maint_due_t due;
  npd_maint_due_load(&due, f64, N, p);
  const bool work = npd_maint_due_decide(&due, t, P.maint_check_interval_hours * 60);      /* moves last_check_time where due with nothing open */
  unsigned scan_bits = 0;      /* bit k: pump k, bit 4 + c: component c -- somebody in the wave has something new there */
  {
    /* every value first, in straight-line code, so that the loads are in flight together (a lone wave that uses each load at once waits
     * out a memory latency per pump); then, per crossed row, that row's stamp alone, for the lanes that crossed it: a running pump's oil
     * temperature sits above its row for the whole run, and its fifteen other stamps are not worth reading at every step */
    uint32_t hits[NPB_NUM_PUMPS];
    double cv[NPB_CMAINT_NCOMP][NPB_CMAINT_NROW];
#pragma unroll
    for (int k = 0; k < NPB_NUM_PUMPS; k++) hits[k] = npd_maint_crossed_rows(S, f64, N, p, k);
#pragma unroll
    for (int c = 0; c < NPB_CMAINT_NCOMP; c++) npd_cmaint_values(f64, N, p, c, P.dt, cv[c]);
#pragma unroll
    for (int k = 0; k < NPB_NUM_PUMPS; k++) {
      bool fresh = false;
#pragma unroll
      for (int q = 0; q < NPB_MAINT_NPARAM; q++) {
        const bool mine = ((hits[k] >> q) & 1u) != 0;
        if (!__any(mine)) continue;
        if (mine) {
          const double lv = (double)*(const npd_real_t *)npd_gaddr(f64, N, p, NPD_MP_COL(k, last_violation_time, q));
          fresh |= !((lv >= 0.0) & (t - lv < S.cooldown_minutes[q]));      /* _is_threshold_in_cooldown */
        }
      }
      if (__any(fresh)) scan_bits |= 1u << k;
    }
#pragma unroll
    for (int c = 0; c < NPB_CMAINT_NCOMP; c++)
      if (__any(npd_cmaint_violations(side, p, c, cv[c], t) != 0)) scan_bits |= 16u << c;
  }
  if (!__any(work) && !scan_bits) return;
  npd_maint_all_rule(RC, side, MC, f64, N, p, t, work, scan_bits);
}

/* ---- host-side launchers: one table per storage type (npb_launchers_t), which npb_api.hip calls through */
/* field access of the C ABI: one member of every plant <-> a contiguous buffer of double (real members) or
 * int32 (int members).  where = arena column, sub = narrow position inside the column, kind: 0 carried real,
 * 1 output real (stored as float), 2 int32 */
__global__ void npb_field_get_kernel(const npd_real_t *__restrict__ arena, size_t N, int col, int sub, int kind, void *__restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  NPD_SEGMENT(arena, N, i);
  const char *e = (const char *)(arena + (size_t)col * N + i);
  if (kind == 0) ((double *)out)[i] = (double)*(const npd_real_t *)e;
  else if (kind == 1) ((double *)out)[i] = (double)*(const float *)(e + sub * 4);
  else ((int32_t *)out)[i] = *(const int32_t *)(e + sub * 4);
}
__global__ void npb_field_set_kernel(npd_real_t *__restrict__ arena, size_t N, int col, int sub, int kind, const void *__restrict__ in, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  NPD_SEGMENT(arena, N, i);
  char *e = (char *)(arena + (size_t)col * N + i);
  if (kind == 0) *(npd_real_t *)e = (npd_real_t)((const double *)in)[i];
  else if (kind == 1) *(float *)(e + sub * 4) = (float)((const double *)in)[i];
  else *(int32_t *)(e + sub * 4) = ((const int32_t *)in)[i];
}
/* many members at once, every value widened to double: out[f * n + plant]; plan[f] = {column, sub, kind} (the state
 * log's sampling step, nuclear_sim_amd/statelog.py) */
__global__ void npb_gather_kernel(const npd_real_t *__restrict__ arena, size_t N, const int *__restrict__ plan, double *__restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
  if (i >= n) return;
  const int col = plan[3 * f], sub = plan[3 * f + 1], kind = plan[3 * f + 2];
  NPD_SEGMENT(arena, N, i);
  const char *e = (const char *)(arena + (size_t)col * N + i);
  double v;
  if (kind == 0) v = (double)*(const npd_real_t *)e;
  else if (kind == 1) v = (double)*(const float *)(e + sub * 4);
  else v = (double)*(const int32_t *)(e + sub * 4);
  out[(size_t)f * n + i] = v;
}
static void NPB_LAUNCHER(gather)(const void *arena, size_t npad, const int *plan_dev, int n_fields, double *out, int n, hipStream_t stream) {
  hipLaunchKernelGGL(npb_gather_kernel, dim3((n + 255) / 256, n_fields), dim3(256), 0, stream, (const npd_real_t *)arena, npad, plan_dev, out, n);
}
static void NPB_LAUNCHER(field_get)(const void *arena, size_t npad, int col, int sub, int kind, void *out, int n, hipStream_t stream) {
  hipLaunchKernelGGL(npb_field_get_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const npd_real_t *)arena, npad, col, sub, kind, out, n);
}
static void NPB_LAUNCHER(field_set)(void *arena, size_t npad, int col, int sub, int kind, const void *in, int n, hipStream_t stream) {
  hipLaunchKernelGGL(npb_field_set_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (npd_real_t *)arena, npad, col, sub, kind, in, n);
}
/* fp64-storage plants above which the sweep of a step (4 221 B per plant) is so far past the 256 MB Infinity Cache that streaming
 * state stores win (measured: even at 81 920, -5 % at 98 304, -10 % at 131 072); fp32 storage moves half the bytes */
#define NPB_NT_STORE_ABOVE ((size_t)90112)
/* plants (of either storage type) from which on npb_create segments the arena ("segmented arena", npd_arena.h), and between which npb_step gives
 * the batch to the four-wave kernel although its groups no longer fit at once.  Measured
 * (profiles/r3_segment_sweep.txt, r3_segment_size.txt): 65 536 plants 0.0906 ms against the one-wave kernel's 0.0956 on a one-block arena
 * (the four-wave kernel there: 0.0975); 49 152 0.0784 against the two-wave kernel's 0.0792, 40 960 level; 81 920 0.122 against 0.166;
 * 106 496 0.169 against the streaming build's 0.175, 131 072 0.202 against 0.193; the streaming build itself gains 2 % at 131 072 plants
 * and 10 % at 262 144 from the segments (profiles/r3_segment_size.txt) */
#define NPB_SEGMENTED_FROM ((size_t)45056)
#define NPB_SEGMENTED_UP_TO ((size_t)114688)
/* the table as the step kernels' pump phase evaluates it (npd_maintenance.h): a strict comparison as the sign of fma(value, sgn, c);
 * any other comparison kind in the scan makes every (wave, pump) "look properly" */
static void npd_maint_fold_table(const npb_params_t *P, const npb_maint_table_t *T, npd_maint_hot_t *H) {
  bool always = false;
  for (int q = 0; q < NPB_MAINT_NPARAM; q++) {
    H->tab[q] = 0.0; H->tab[NPB_MAINT_NPARAM + q] = -1.0;
    if (!T || T->rank[q] < 0) continue;
    if (T->comparison[q] == NPB_CMP_GREATER_THAN) { H->tab[q] = 1.0; H->tab[NPB_MAINT_NPARAM + q] = -T->threshold[q]; }
    else if (T->comparison[q] == NPB_CMP_LESS_THAN) { H->tab[q] = -1.0; H->tab[NPB_MAINT_NPARAM + q] = T->threshold[q]; }
    else always = true;
    if (!(T->threshold[q] == T->threshold[q]) || T->threshold[q] - T->threshold[q] != 0.0) always = true;   /* a NaN or infinite threshold: leave it to the real comparison */
  }
  H->tab[2 * NPB_MAINT_NPARAM] = always ? 1.0 : 0.0;
  H->tab[2 * NPB_MAINT_NPARAM + 1] = P->maint_check_interval_hours * 60;
}
static npd_maint_cache_t npd_maint_cache_of(void *maint_side, int32_t *counts, int n_plants, double *diag = nullptr, size_t diag_pitch = 0) {
  npd_maint_cache_t C;
  C.counts = counts; C.n_plants = n_plants; C.diag = diag; C.diag_pitch = diag_pitch;
  C.entry = maint_side ? (npd_u32x4 *)((char *)maint_side + NPD_MAINT_CONSTS_BYTES) : nullptr;
  return C;
}
/* maint_table / maint_side (the handle's maintenance side buffer, rule constants uploaded): NULL unless the automatic maintenance is on (npb_step) */
static int NPB_LAUNCHER(step)(const npb_params_t *P, int n_plants, size_t npad_seg, void *arena,
                              const int32_t *action, const double *magnitude, const double *setpoint,
                              const double *noise_z, const double *cw_temp, double *obs, double *reward, uint8_t *done,
                              uint32_t *trip_flags, double *info, int variant, double *diag, size_t diag_pitch,
                              const npb_maint_table_t *maint_table, void *maint_side, int32_t *maint_counts, hipStream_t stream) {
  const size_t npad = NPD_NPAD(npad_seg), seg = NPD_SEG_OF(npad_seg);   /* column pitch in plants / plants per arena segment (0: one segment) */
  npd_maint_hot_t MH;
  npd_maint_fold_table(P, maint_side ? maint_table : nullptr, &MH);
  const npd_maint_cache_t MC = npd_maint_cache_of(maint_side, maint_counts, n_plants, diag, diag_pitch);
  const npd_maint_rule_consts_t *maint_rc = (const npd_maint_rule_consts_t *)maint_side;     /* NULL = off */
  dim3 grid((unsigned)(npad / NPB_WAVE)), block(NPB_WAVE);
  if (diag && P->mode == NPB_MODE_FULL) {   /* npb_set_diagnostics: the diagnostics build of the one-wave kernel at any size */
    hipLaunchKernelGGL(npb_step_diag_kernel, grid, block, 0, stream, *P, n_plants, npad_seg, (npd_real_t *)arena, action, magnitude, setpoint,
                       noise_z, cw_temp, obs, reward, done, trip_flags, info, MH, maint_rc, MC, diag, diag_pitch);
    return NPB_KERNEL_STEP_DIAG;
  }
  /* two kernels, one result (the same device functions in the same order per plant; tests/test_gpu_parity.py,
   * test_the_two_step_kernels_agree).  The more waves share a plant, the shorter the critical path of a step and the more of
   * the chip a small batch fills: four waves (npd_step4.h) while they are all resident, two (npd_step2.h) up to ~57 k plants;
   * once the one-wave kernel has a wave for every SIMD its LDS-DMA pipeline wins (measured crossovers).
   * variant: 0 = by batch size, 1 = one wave per 64 plants, 2 = two waves, 3 = their two-per-SIMD build, 4 = one wave with
   * streaming state stores (what 0 picks once the sweep is far past the Infinity Cache), 5 = four waves (npd_step4.h: what 0
   * picks while all its waves are resident at once, up to 32 768 plants, and again on the segmented arenas of 45 057 .. 114 688
   * plants).  The primary + steam-generator
   * mode always takes a one-wave kernel.  The return value names the kernel that was launched (npb_debug_last_step_kernel). */
  if (P->mode == NPB_MODE_PRIMARY) {
    hipLaunchKernelGGL(npb_step_primary_kernel, grid, block, 0, stream, *P, n_plants, npad_seg, (npd_real_t *)arena, action, magnitude, setpoint,
                       noise_z, obs, reward, done, trip_flags, info);
    return NPB_KERNEL_STEP_PRIMARY;
  }
  if (variant == 0) variant = npad <= 32768 ? 5 : (npad <= NPB_SEGMENTED_FROM ? 2 : (npad <= NPB_SEGMENTED_UP_TO ? 5 : (npad * sizeof(npd_real_t) > NPB_NT_STORE_ABOVE * 8 ? 4 : 1)));
  const bool with_maint = maint_rc != nullptr;     /* the builds with the automatic maintenance compiled in */
  if (variant == 4) {
    hipLaunchKernelGGL(with_maint ? npb_step_nt_maint_kernel : npb_step_nt_kernel, grid, block, 0, stream, *P, n_plants, npad_seg, (npd_real_t *)arena, action, magnitude, setpoint,
                       noise_z, cw_temp, obs, reward, done, trip_flags, info, MH, maint_rc, MC);
    return with_maint ? NPB_KERNEL_STEP_NT_MAINT : NPB_KERNEL_STEP_NT;
  }
  if (variant == 5 && P->mode == NPB_MODE_FULL) {     /* four waves per 64 plants (npd_step4.h) */
    hipLaunchKernelGGL(with_maint ? npb_step4_maint_kernel : npb_step4_kernel, grid, dim3(NPD4_THREADS), 0, stream, *P, n_plants, npad_seg, (npd_real_t *)arena, action, magnitude,
                       setpoint, noise_z, cw_temp, obs, reward, done, trip_flags, info, MH, maint_rc, MC);
    return with_maint ? NPB_KERNEL_STEP4_MAINT : NPB_KERNEL_STEP4;
  }
  const bool two_wave = (variant == 2 || variant == 3) && P->mode == NPB_MODE_FULL;
  const bool wide = two_wave && variant == 2 && npad <= 32768;   /* the whole register file while one wave per SIMD is all there is; variant 3 = never */
  if (wide) {
    hipLaunchKernelGGL(with_maint ? npb_step2_wide_maint_kernel : npb_step2_wide_kernel, grid, dim3(NPD2_THREADS), 0, stream, *P, n_plants, npad_seg, (npd_real_t *)arena, action, magnitude,
                       setpoint, noise_z, cw_temp, obs, reward, done, trip_flags, info, MH, maint_rc, MC);
    return with_maint ? NPB_KERNEL_STEP2_WIDE_MAINT : NPB_KERNEL_STEP2_WIDE;
  }
  if (two_wave) {
    hipLaunchKernelGGL(with_maint ? npb_step2_maint_kernel : npb_step2_kernel, grid, dim3(NPD2_THREADS), 0, stream, *P, n_plants, npad_seg, (npd_real_t *)arena, action, magnitude,
                       setpoint, noise_z, cw_temp, obs, reward, done, trip_flags, info, MH, maint_rc, MC);
    return with_maint ? NPB_KERNEL_STEP2_MAINT : NPB_KERNEL_STEP2;
  }
  hipLaunchKernelGGL(with_maint ? npb_step_maint_kernel : npb_step_kernel, grid, block, 0, stream, *P, n_plants, npad_seg, (npd_real_t *)arena, action, magnitude, setpoint,
                     noise_z, cw_temp, obs, reward, done, trip_flags, info, MH, maint_rc, MC);
  return with_maint ? NPB_KERNEL_STEP_MAINT : NPB_KERNEL_STEP;
}
/* the rule as a launch of its own (modes that do not step the pumps) */
static void NPB_LAUNCHER(maint)(size_t npad, void *arena, void *maint_side, int32_t *counts, int n_plants, hipStream_t stream) {
  hipLaunchKernelGGL(npb_maint_kernel, dim3((unsigned)(NPD_NPAD(npad) / NPB_WAVE)), dim3(NPB_WAVE), 0, stream, (const npd_maint_rule_consts_t *)maint_side,
                     npd_maint_cache_of(maint_side, counts, n_plants), npad, (npd_real_t *)arena);
}
/* the whole rule, pumps and components in one queue, behind the plain step kernel (npb_set_component_maintenance): cm_side = the handle's
 * component side buffer (npb_launch_cmaint_side_bytes), its table uploaded */
static void NPB_LAUNCHER(maint_all)(size_t npad, void *arena, void *maint_side, void *cm_side, int32_t *counts, int n_plants, double *diag, size_t diag_pitch,
                                    hipStream_t stream) {
  npd_cmaint_side_t side;
  side.C = (const npd_cmaint_consts_t *)cm_side; side.state = (double *)((char *)cm_side + (sizeof(npd_cmaint_consts_t) + 255) / 256 * 256); side.pitch = NPD_NPAD(npad);
  hipLaunchKernelGGL(npb_maint_all_kernel, dim3((unsigned)(NPD_NPAD(npad) / NPB_WAVE)), dim3(NPB_WAVE), 0, stream, (const npd_maint_rule_consts_t *)maint_side, side,
                     npd_maint_cache_of(maint_side, counts, n_plants, diag, diag_pitch), npad, (npd_real_t *)arena);
}
static void NPB_LAUNCHER(observe)(int mode, int n_plants, size_t npad, const void *arena, double *obs, hipStream_t stream) {
  dim3 grid((unsigned)(NPD_NPAD(npad) / NPB_WAVE)), block(NPB_WAVE);
  hipLaunchKernelGGL(npb_observe_kernel, grid, block, 0, stream, mode, n_plants, npad, (const npd_real_t *)arena, obs);
}
static void NPB_LAUNCHER(reset)(const npb_params_t *P, int n_plants, size_t npad, void *arena, const uint8_t *mask, int steady, hipStream_t stream) {
  dim3 grid((unsigned)(NPD_NPAD(npad) / NPB_WAVE)), block(NPB_WAVE);
  hipLaunchKernelGGL(npb_reset_kernel, grid, block, 0, stream, *P, npad, (npd_real_t *)arena, mask, n_plants, steady);
}
static void NPB_LAUNCHER(init)(const npb_params_t *P, int n_plants, size_t npad, void *arena, const uint8_t *mask, hipStream_t stream) {
  dim3 grid((unsigned)(NPD_NPAD(npad) / NPB_WAVE)), block(NPB_WAVE);
  hipLaunchKernelGGL(npb_init_kernel, grid, block, 0, stream, *P, npad, (npd_real_t *)arena, mask, n_plants);
}
/* episodes (npb_snapshot / npb_restore / npb_set_autoreset): maint_side / maint_counts NULL unless params.maint_enabled */
static npd_restore_side_t npd_restore_side_of(void *maint_side, int32_t *maint_counts, int n_plants, const npb_side_restores_t &side) {
  npd_restore_side_t R;
  R.maint_entry = npd_maint_cache_of(maint_side, maint_counts, n_plants).entry; R.maint_counts = maint_counts; R.n_plants = n_plants;
  R.cm = side.block[NPB_SIDE_CMAINT]; R.dg = side.block[NPB_SIDE_DIAG];
  return R;
}
/* src: the snapshot (npb_restore, the snapshot autoreset) or a bank with its slots (npb_restore_bank, the bank autoreset).  mask NULL
 * restores every lane of the pitch from the snapshot, the plants only from a bank (its slot columns have n entries) */
static void NPB_LAUNCHER(restore)(int n_plants, size_t npad, void *arena, npb_source_t src, const uint8_t *mask, npb_episode_counters_t C,
                                  void *maint_side, int32_t *maint_counts, npb_side_restores_t side, hipStream_t stream) {
  const int lanes = mask || src.next_slot ? n_plants : (int)NPD_NPAD(npad);
  hipLaunchKernelGGL(npb_restore_kernel, dim3((unsigned)(NPD_NPAD(npad) / NPB_WAVE)), dim3(NPB_WAVE), 0, stream, lanes, npad, (npd_real_t *)arena,
                     src, mask, C.len, C.ret, C.index, npd_restore_side_of(maint_side, maint_counts, n_plants, side));
}
static void NPB_LAUNCHER(episode)(int mode, int n_plants, size_t npad, void *arena, npb_source_t src, const uint8_t *done, const double *reward,
                                  double *obs, npb_episode_counters_t C, int32_t *out_len, double *out_ret, uint8_t *out_truncated,
                                  double *final_obs, int max_steps, void *maint_side, int32_t *maint_counts, npb_side_restores_t side, hipStream_t stream) {
  npd_episode_t E;
  E.len = C.len; E.ret = C.ret; E.index = C.index; E.out_index = C.out_index; E.out_len = out_len; E.out_ret = out_ret; E.out_truncated = out_truncated; E.final_obs = final_obs; E.max_steps = max_steps;
  hipLaunchKernelGGL(npb_episode_kernel, dim3((unsigned)(NPD_NPAD(npad) / NPB_WAVE)), dim3(NPB_WAVE), 0, stream, mode, n_plants, npad, (npd_real_t *)arena,
                     src, done, reward, obs, E, npd_restore_side_of(maint_side, maint_counts, n_plants, side));
}
/* npb_perform_maintenance: the caller's order columns; L = the maintenance event log (npb_set_maintenance_log) */
static void NPB_LAUNCHER(operator_maint)(int n_plants, size_t npad, void *arena, const int32_t *action, const int32_t *pump, const int32_t *bearing,
                                         const double *target_level, uint8_t *success, npd_maint_log_t L, hipStream_t stream) {
  npd_operator_orders_t O;
  O.action = action; O.pump = pump; O.bearing = bearing; O.target_level = target_level; O.success = success; O.n_plants = n_plants;
  hipLaunchKernelGGL(npb_operator_maint_kernel, dim3((unsigned)(NPD_NPAD(npad) / NPB_WAVE)), dim3(NPB_WAVE), 0, stream, O, L, npad, (npd_real_t *)arena);
}
/* npb_perform_component_maintenance: the caller's order columns; kinds = the component kinds the handle's mode carries; L as above */
static void NPB_LAUNCHER(operator_component_maint)(int n_plants, size_t npad, void *arena, const int32_t *action, const int32_t *unit, const int32_t *option,
                                                   const double *amount, uint8_t *success, unsigned kinds, npd_maint_log_t L, hipStream_t stream) {
  npd_component_orders_t O;
  O.action = action; O.unit = unit; O.option = option; O.amount = amount; O.success = success; O.n_plants = n_plants; O.kinds = kinds;
  hipLaunchKernelGGL(npb_operator_component_maint_kernel, dim3((unsigned)(NPD_NPAD(npad) / NPB_WAVE)), dim3(NPB_WAVE), 0, stream, O, L, npad, (npd_real_t *)arena);
}
/* npb_perform_turbine_maintenance: the caller's order columns; turbine = the handle's mode steps the turbine; L as above */
static void NPB_LAUNCHER(operator_turbine_maint)(int n_plants, size_t npad, void *arena, const int32_t *action, const int32_t *unit, uint8_t *success,
                                                 int turbine, npd_maint_log_t L, hipStream_t stream) {
  npd_turbine_orders_t O;
  O.action = action; O.unit = unit; O.success = success; O.n_plants = n_plants; O.turbine = turbine;
  hipLaunchKernelGGL(npb_operator_turbine_maint_kernel, dim3((unsigned)(NPD_NPAD(npad) / NPB_WAVE)), dim3(NPB_WAVE), 0, stream, O, L, npad, (npd_real_t *)arena);
}
/* not const: clang emits a namespace-scope const into the device code too, where these host functions do not exist */
extern "C" npb_launchers_t NPB_LAUNCHER(table) = {
  NPB_LAUNCHER(step), NPB_LAUNCHER(maint), NPB_LAUNCHER(observe), NPB_LAUNCHER(init), NPB_LAUNCHER(reset),
  NPB_LAUNCHER(field_get), NPB_LAUNCHER(field_set), NPB_LAUNCHER(gather), NPB_LAUNCHER(restore), NPB_LAUNCHER(episode),
  NPB_LAUNCHER(operator_maint), NPB_LAUNCHER(operator_component_maint), NPB_LAUNCHER(operator_turbine_maint), NPB_LAUNCHER(maint_all),
};
