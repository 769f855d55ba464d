/*
 * npb_storage_free.hip -- the kernels and host functions of the handle that never see an arena element type ("The
 * translation units of libnpb.so"): the traffic counters' calibration sweep (fp64 columns by definition), the rule constants and the
 * side buffers' sizes, the episode counters' clear, the component maintenance's side state, the carried diagnostics rows, the
 * work-order summary, the clear kernels of the column statistics and the event windows, the normaliser's reward kernel, the unprime
 * kernel and the whole rollout.  Compiled once, with the step kernels' flags: both storage types call the same extern "C" launchers
 * (npb_kernels.h), so there is no table here.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "npd_common.h"
#include "npd_arena.h"              /* NPD_NPAD: a launcher's pitch out of a packed N */
#include "npd_primary.h"            /* npd_coupling_t, for the two below */
#include "npd_maintenance.h"        /* npd_maint_rule_consts_t */
#include "npd_component_auto.h"     /* npd_cmaint_consts_t, npd_cmaint_init */
#include "npb_kernels.h"
#include "npd_attach.h"

/* calibration aid for the HBM traffic counters: reads every arena column and writes it back unchanged,
 * with exactly the access shape of the step kernel (8 B per lane, one 512-B line per wave and column),
 * so that FETCH_SIZE / WRITE_SIZE can be scaled against a known byte count (2 * state_bytes * pitch) */
__global__ __launch_bounds__(NPB_WAVE) void npb_touch_kernel(size_t N, double *__restrict__ f64) {
  const size_t p = (size_t)blockIdx.x * NPB_WAVE + threadIdx.x;
  { const size_t seg = N >> 32; N &= 0xffffffffu; if (seg) { f64 += (p / seg) * seg * (size_t)(NPB_TOTAL_COL64 - 1); N = seg; } }
#pragma unroll 8
  for (int k = 0; k < NPB_TOTAL_COL64; k++) { double v = f64[(size_t)k * N + p]; f64[(size_t)k * N + p] = v + 0.0; }
}
extern "C" void npb_launch_touch(size_t npad_seg, double *f64, hipStream_t stream) {
  const size_t npad = NPD_NPAD(npad_seg);
  dim3 grid((unsigned)(npad / NPB_WAVE)), block(NPB_WAVE);
  hipLaunchKernelGGL(npb_touch_kernel, grid, block, 0, stream, npad_seg, f64);
}

/* the maintenance side buffer does not depend on the storage type (npd_maint_rule_consts_t, npd_maintenance.h, holds no npd_real_t).
 * The rule's constants as the device reads them: host_out = npb_launch_maint_consts_bytes() bytes */
extern "C" void npb_launch_maint_consts(const npb_params_t *P, const npb_maint_table_t *T, npd_maint_log_t log, void *host_out) {
  npd_maint_rule_consts_t *RC = (npd_maint_rule_consts_t *)host_out;
  memset(RC, 0, sizeof(*RC));
  RC->P = *P; RC->T = *T; RC->L = log;
  npd_maint_screen_t &S = RC->S;
  for (int q = 0; q < NPB_MAINT_NPARAM; q++) {
    S.threshold[q] = T->threshold[q];
    S.cooldown_minutes[q] = T->cooldown_hours[q] * 60;
    if (T->rank[q] < 0) continue;             /* not in the scan: no mask bit, never fires */
    const int c = T->comparison[q];
    const uint32_t bit = 1u << q;
    if (c == NPB_CMP_GREATER_THAN || c == NPB_CMP_GREATER_EQUAL) S.want_gt |= bit;
    if (c == NPB_CMP_LESS_THAN || c == NPB_CMP_LESS_EQUAL) S.want_lt |= bit;
    if (c == NPB_CMP_GREATER_EQUAL || c == NPB_CMP_LESS_EQUAL) S.want_eq |= bit;
    if (c == NPB_CMP_EQUALS) S.want_near |= bit;
    if (c != NPB_CMP_GREATER_THAN && c != NPB_CMP_GREATER_EQUAL && c != NPB_CMP_LESS_THAN && c != NPB_CMP_LESS_EQUAL && c != NPB_CMP_EQUALS) S.want_far |= bit;
  }
}
extern "C" size_t npb_launch_maint_consts_bytes(void) { return sizeof(npd_maint_rule_consts_t); }
/* rule constants + cooldown cache (npd_maint_cache_of); a zeroed cache = "nothing known: look" */
extern "C" size_t npb_launch_maint_side_bytes(size_t npad) { return NPD_MAINT_CONSTS_BYTES + (size_t)NPB_NUM_PUMPS * NPD_NPAD(npad) * (sizeof(float) + sizeof(uint32_t)); }
extern "C" size_t npb_launch_maint_cache_offset(void) { return NPD_MAINT_CONSTS_BYTES; }

/* npb_reset / npb_reset_reference / npb_restore: the episode counters (len, ret) and the carried start entries (start: -1, not from
 * the bank) of the plants of mask (NULL = every lane of the pitch); each column may be NULL */
__global__ void npb_episode_clear_kernel(const uint8_t *__restrict__ mask, int32_t *__restrict__ len, double *__restrict__ ret, int32_t *__restrict__ index,
                                         int32_t *__restrict__ start, int n_plants, int npad) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npad || (mask && (p >= n_plants || !mask[p]))) return;
  if (len) { len[p] = 0; index[p] += 1; }      /* (the index is allocated with the length) */
  if (ret) ret[p] = 0.0;
  if (start) start[p] = -1;
}
/* the component maintenance's side state (npd_component_auto.h) of the plants of mask (NULL = every lane of the pitch) as a freshly
 * constructed plant has it (npb_set_component_maintenance, npb_reset) */
__global__ void npb_cmaint_init_kernel(double *state, size_t pitch, const uint8_t *__restrict__ mask, int n_plants) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pitch || (mask && (p >= (size_t)n_plants || !mask[p]))) return;
  npd_cmaint_init(state, pitch, p);
}
/* the side buffer of one handle: [the table as the device reads it, a 256-byte slot][NPB_CMAINT_SIDE_DOUBLES][pitch] doubles */
#define NPD_CMAINT_CONSTS_BYTES ((sizeof(npd_cmaint_consts_t) + 255) / 256 * 256)
extern "C" size_t npb_launch_cmaint_side_bytes(size_t pitch) { return NPD_CMAINT_CONSTS_BYTES + (size_t)NPB_CMAINT_SIDE_DOUBLES * pitch * sizeof(double); }
extern "C" size_t npb_launch_cmaint_state_offset(void) { return NPD_CMAINT_CONSTS_BYTES; }
extern "C" void npb_launch_cmaint_init(void *cm_side, size_t pitch, const uint8_t *mask, int n_plants, hipStream_t stream) {
  hipLaunchKernelGGL(npb_cmaint_init_kernel, dim3((unsigned)((pitch + 255) / 256)), dim3(256), 0, stream,
                     (double *)((char *)cm_side + NPD_CMAINT_CONSTS_BYTES), pitch, mask, n_plants);
}
extern "C" void npb_launch_episode_clear(const uint8_t *mask, int32_t *len, double *ret, int32_t *index, int32_t *start, int n_plants, size_t npad,
                                         hipStream_t stream) {
  const int n = (int)NPD_NPAD(npad);
  hipLaunchKernelGGL(npb_episode_clear_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, mask, len, ret, index, start, n_plants, n);
}
/* the carried diagnostics rows (include/npb.h NPB_DIAG_CARRIED) of a diagnostics buffer into a packed [NPB_DIAG_NUM_CARRIED][pitch] copy in
 * table order: npb_snapshot, npb_set_start_bank */
__global__ void npb_diag_carried_pack_kernel(const double *__restrict__ live, size_t live_pitch, double *__restrict__ packed, size_t packed_pitch,
                                             size_t lanes) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= lanes) return;
  int k = 0;
#define NPB__X(row, fresh) packed[(size_t)(k++) * packed_pitch + p] = live[(size_t)(row) * live_pitch + p];
  NPB_DIAG_CARRIED(NPB__X)
#undef NPB__X
}
/* npb_reset / npb_reset_reference: the carried rows of the plants of mask (NULL = every lane below `lanes`) to values.v[k]; NaN = kept */
__global__ void npb_diag_carried_put_kernel(double *__restrict__ live, size_t live_pitch, const uint8_t *__restrict__ mask, int n_plants, size_t lanes,
                                            npb_diag_carried_values_t values) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= lanes || (mask && (p >= (size_t)n_plants || !mask[p]))) return;
  int k = 0;
#define NPB__X(row, fresh) { const double v = values.v[k++]; if (v == v) live[(size_t)(row) * live_pitch + p] = v; }
  NPB_DIAG_CARRIED(NPB__X)
#undef NPB__X
}
extern "C" void npb_launch_diag_carried_pack(const double *live, size_t live_pitch, double *packed, size_t packed_pitch, size_t lanes, hipStream_t stream) {
  hipLaunchKernelGGL(npb_diag_carried_pack_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, live, live_pitch, packed, packed_pitch, lanes);
}
extern "C" void npb_launch_diag_carried_put(double *live, size_t live_pitch, const uint8_t *mask, int n_plants, size_t lanes,
                                            npb_diag_carried_values_t values, hipStream_t stream) {
  hipLaunchKernelGGL(npb_diag_carried_put_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, live, live_pitch, mask, n_plants, lanes,
                     values);
}
/* the per-plant work-order summary folded from the event log (npb_set_maintenance_summary): its kernels and launchers */
#include "npd_maint_summary.h"

/* npb_column_stats_clear: the cells of the plants of mask (NULL = all) back to the empty values, over the fold's grid
 * (npd_column_stats.h) */
__global__ __launch_bounds__(NPD_COLSTAT_BLOCK) void npb_column_stats_clear_kernel(npb_column_stats_t S, const uint8_t *__restrict__ mask, int n_plants) {
  const int c = blockIdx.y;
  const size_t p = (size_t)blockIdx.x * NPD_COLSTAT_BLOCK + threadIdx.x;
  if (p >= (size_t)n_plants || (mask && !mask[p])) return;
  const size_t cell = (size_t)c * (size_t)n_plants + p;
  if (S.min) S.min[cell] = NPD_COLSTAT_POS_INF;
  if (S.max) S.max[cell] = NPD_COLSTAT_NEG_INF;
  if (S.sum) S.sum[cell] = 0.0;
  if (S.sumsq) S.sumsq[cell] = 0.0;
  if (S.last) S.last[cell] = NPD_COLSTAT_NAN;
  if (S.first_beyond) S.first_beyond[cell] = NPD_COLSTAT_POS_INF;
  if (S.n_beyond) S.n_beyond[cell] = 0;
  if (c == 0) S.n_samples[p] = 0;
}
extern "C" void npb_launch_column_stats_clear(const npb_column_stats_t *S, const uint8_t *mask, int n_plants, hipStream_t stream) {
  hipLaunchKernelGGL(npb_column_stats_clear_kernel, dim3((unsigned)((n_plants + NPD_COLSTAT_BLOCK - 1) / NPD_COLSTAT_BLOCK), (unsigned)S->n_cols),
                     dim3(NPD_COLSTAT_BLOCK), 0, stream, *S, mask, n_plants);
}

/* npb_event_windows_clear, and the start of npb_set_event_windows: the plants of mask (NULL = all) unprimed, their rings empty, an armed
 * capture dropped (npd_event_windows.h) */
__global__ __launch_bounds__(256) void npb_event_windows_clear_kernel(npb_event_windows_t W, const uint8_t *__restrict__ mask, int n_plants) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)n_plants || (mask && !mask[p])) return;
  W.valid[p] = 0;
  W.due[p] = -1;
}
extern "C" void npb_launch_event_windows_clear(const npb_event_windows_t *W, const uint8_t *mask, int n_plants, hipStream_t stream) {
  hipLaunchKernelGGL(npb_event_windows_clear_kernel, dim3((unsigned)((n_plants + 255) / 256)), dim3(256), 0, stream, *W, mask, n_plants);
}

/* npb_set_normalizer's reward kernel, behind the finish (npd_normalizer.h says what it does): nothing of the arena */
__global__ __launch_bounds__(256) void npb_normalizer_reward_kernel(npb_normalizer_t Z, int n_plants, const int32_t *__restrict__ index,
                                                                    const double *__restrict__ reward, const uint8_t *__restrict__ done, int carry) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)n_plants) return;
  const double r = reward[p];
  if (carry) Z.ret[p] = npd_normalizer_return(Z, p, index, r);
  double y = r * Z.scale[Z.n_streams - 1];
  const double lo = -Z.clip;
  y = y < lo ? lo : y;
  y = y > Z.clip ? Z.clip : y;
  Z.norm_reward[p] = y;
  Z.ended[p] = done[p] != 0;
  Z.primed[p] = 1;
  if (index) Z.seen[p] = index[p];
}
extern "C" void npb_launch_normalizer_reward(const npb_normalizer_t *Z, int n_plants, const int32_t *index, const double *reward, const uint8_t *done,
                                             int carry, hipStream_t stream) {
  hipLaunchKernelGGL(npb_normalizer_reward_kernel, dim3((unsigned)((n_plants + 255) / 256)), dim3(256), 0, stream, *Z, n_plants, index, reward, done, carry);
}

/* npb_task_clear, npb_features_clear, npb_controls_clear: the plants of mask (NULL = all) unprimed in that attachment's `primed` column --
 * the task's next DELTA samples are 0, the features' next frame fills every slot, the controls' next step starts a new hold */
__global__ __launch_bounds__(256) void npb_unprime_kernel(int32_t *__restrict__ primed, const uint8_t *__restrict__ mask, int n_plants) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)n_plants || (mask && !mask[p])) return;
  primed[p] = 0;
}
extern "C" void npb_launch_unprime(int32_t *primed, const uint8_t *mask, int n_plants, hipStream_t stream) {
  hipLaunchKernelGGL(npb_unprime_kernel, dim3((unsigned)((n_plants + 255) / 256)), dim3(256), 0, stream, primed, mask, n_plants);
}

/* the rollout (npb_set_rollout): the two kernels around the step, the cut, the advantages and their launchers */
#include "npd_rollout.h"
