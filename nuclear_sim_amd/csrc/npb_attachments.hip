/*
 * npb_attachments.hip -- the per-step attachments that read the arena ("The translation units of libnpb.so"): the state
 * log's sampler, the episode records, the reader of a per-plant column and what is built on it -- column statistics, event windows,
 * the task, the features, the controls, the order rules on their axes and the normaliser's partials.  Each is a launch of its own beside the step kernels of
 * npb_kernels.hip and shares no device code with them beyond the headers below.  Compiled once per storage type, with the step
 * kernels' flags; its launchers make up npb_launch_attach_table / npb32_launch_attach_table (npb_attach_launchers_t, npb_kernels.h).  The halves of
 * these attachments that never see an arena element -- their clear kernels, the normaliser's reward kernel -- are in
 * npb_storage_free.hip.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "npd_common.h"
#include "npd_primary.h"      /* npd_apply_control_actions: the controls move the actuators as the step does */
#include "npd_arena.h"
#include "npd_record_log.h"
#include "npb_kernels.h"
#include "npd_attach.h"
#include "npd_maintenance.h"             /* the handlers the order rules call, as the operator kernels of npb_kernels.hip call them */
#include "npd_component_maintenance.h"
#include "npd_turbine_maintenance.h"

/* the state log's sampling step for a watch list (npb_sampler_sample): one grid row per output row, lanes over the watched plants.
 * Row r < n_fields is an arena member, addressed as npb_gather_kernel addresses it with the plant ids[j] in place of the lane; the rows
 * behind are side rows (npb_sample_row_t): caller-owned buffers beside the arena.  Every value is widened to double: out[r * n_watched + j].
 * The row's descriptor is uniform over the block (scalar loads); consecutive ids read consecutive elements */
__global__ void npb_sample_kernel(const npd_real_t *__restrict__ arena, size_t N, const int *__restrict__ plan, int n_fields,
                                  const npb_sample_row_t *__restrict__ side, const int32_t *__restrict__ ids, double *__restrict__ out, int n_watched) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (j >= n_watched) return;
  const size_t p = (size_t)ids[j];
  double v;
  if (r < n_fields) {
    const int col = plan[3 * r], sub = plan[3 * r + 1], kind = plan[3 * r + 2];
    NPD_SEGMENT(arena, N, p);
    const char *e = (const char *)(arena + (size_t)col * N + p);
    if (kind == 0) v = (double)*(const npd_real_t *)e;
    else if (kind == 1) v = (double)*(const float *)(e + sub * 4);
    else v = (double)*(const int32_t *)(e + sub * 4);
  } else {
    const npb_sample_row_t S = side[r - n_fields];
    const int64_t e = (int64_t)p * S.plant_stride;
    if (S.type == NPB_SAMPLE_F64) v = ((const double *)S.row)[e];
    else if (S.type == NPB_SAMPLE_F32) v = (double)((const float *)S.row)[e];
    else if (S.type == NPB_SAMPLE_I32) v = (double)((const int32_t *)S.row)[e];
    else v = (double)((const uint8_t *)S.row)[e];
  }
  out[(size_t)r * n_watched + j] = v;
}
static void NPB_LAUNCHER(sample)(const void *arena, size_t npad, const int *plan_dev, int n_fields, const npb_sample_row_t *side_dev, int n_rows,
                                 const int32_t *ids_dev, int n_watched, double *out, hipStream_t stream) {
  const int block = n_watched <= 64 ? 64 : 256;      /* a short watch list: one wave per row, no idle waves */
  hipLaunchKernelGGL(npb_sample_kernel, dim3((n_watched + block - 1) / block, n_rows), dim3(block), 0, stream, (const npd_real_t *)arena, npad, plan_dev,
                     n_fields, side_dev, ids_dev, out, n_watched);
}
/* THE reader of a per-plant column (npb_colstat_col_t, npb_kernels.h): one value of plant p, widened to double as npb_sample_kernel widens
 * it.  f64 / N: the arena and its pitch AFTER NPD_SEGMENT (the fold applies it per thread, the windows and the task per wave: that stays
 * with the kernels).  The call site names how the descriptor arrives, because this compiler's code depends on it: a copy of the fold's
 * (D = npb_colstat_col_t) keeps its side-row loads global_load_*, where a reference makes them flat_load_* with lgkmcnt waits; a reference
 * into the kernel's argument (D = const npb_colstat_col_t &) keeps the windows' and the task's loads where they are, where a copy
 * reorders them (tools/compare_step_kernels.py shows either) */
template <class D> __device__ __forceinline__ double npd_column_read(const npd_real_t *f64, size_t N, size_t p, D C) {
  if (C.kind < 3) {
    const char *e = (const char *)(f64 + (size_t)C.col * N + p);
    if (C.kind == 0) return (double)*(const npd_real_t *)e;
    if (C.kind == 1) return (double)*(const float *)(e + C.sub * 4);
    return (double)*(const int32_t *)(e + C.sub * 4);
  }
  const int64_t e = (int64_t)p * C.plant_stride;
  const int type = C.kind - 3;
  if (type == NPB_SAMPLE_F64) return ((const double *)C.row)[e];
  if (type == NPB_SAMPLE_F32) return (double)((const float *)C.row)[e];
  if (type == NPB_SAMPLE_I32) return (double)((const int32_t *)C.row)[e];
  return (double)((const uint8_t *)C.row)[e];
}

/* npb_set_episode_records: the record of every episode that ends on this step, behind the step kernel, the rule and the summary fold and
 * BEFORE the episode kernel, which then does the bookkeeping and the restore as it always does: here the arena, the step's output columns
 * and the carried counters still describe the episode that ended.  Nothing of them is written */
struct npd_episode_records_t {
  npb_episode_records_desc_t D;                               /* the caller's columns and cursor */
  const int32_t *len; const double *ret; const int32_t *index; const int32_t *start;      /* carried [pitch]; start NULL = no bank */
  double *s_first_created, *s_first_completed; int32_t *s_n_created, *s_n_completed;      /* the handle's summary tables [n_keys][n_plants], or NULL */
  int n_keys;
  int max_steps;                                              /* 0 = no limit */
  int step;                                                   /* npb_step calls since the records were switched on */
  const npb_record_stats_t *stats;                            /* device: the handle's column statistics and the record-side columns that take them
                                                               * (npb_set_episode_record_stats), read by ended lanes only; NULL = not taken */
};
__global__ __launch_bounds__(NPB_WAVE) void npb_episode_records_kernel(int n_plants, size_t N, const npd_real_t *__restrict__ f64, const uint8_t *__restrict__ done,
                                                                       const double *__restrict__ reward, const double *__restrict__ obs,
                                                                       const uint32_t *__restrict__ trip_flags, npd_episode_records_t R) {
  const size_t block_base = (size_t)blockIdx.x * NPB_WAVE;
  NPD_SEGMENT(f64, N, block_base);
  const size_t p = block_base + threadIdx.x;
  bool terminated = false, truncated = false;
  int32_t len = 0;
  double ret = 0.0;
  if (p < (size_t)n_plants) {           /* the outcome as npb_episode_kernel decides it, behind this kernel on the same columns */
    terminated = done[p] != 0;
    len = R.len[p] + 1;
    ret = reward ? R.ret[p] + reward[p] : R.ret[p];
    truncated = R.max_steps > 0 && len >= R.max_steps && !terminated;     /* termination wins */
  }
  const bool ended = terminated || truncated;
  if (!__any(ended)) return;
  const npd_log_slots_t s = npd_log_reserve(R.D.cursor, ended);      /* the ended lanes' slots (npd_record_log.h) */
  const int lane = threadIdx.x;
  const uint32_t cap = (uint32_t)R.D.capacity;
  const uint32_t slot = npd_log_slot(s);
  const bool store = ended && slot < cap;
  if (store) {
    R.D.plant[slot] = (int32_t)p;
    R.D.episode[slot] = R.index[p];
    R.D.start[slot] = R.start ? R.start[p] : -1;
    R.D.length[slot] = len;
    R.D.flags[slot] = (terminated ? 1 : 0) | (truncated ? 2 : 0);
    R.D.trip_flags[slot] = trip_flags ? trip_flags[p] : 0u;
    R.D.step[slot] = R.step;
    R.D.ret[slot] = ret;
    R.D.end_time[slot] = NPD_F64_COL(PRIM, npb_prim_t, sim_time, 0);
  }
  if (R.D.final_obs && obs) {           /* the terminal observation: the wave's rows are consecutive in obs, and so are its slots */
#pragma unroll
    for (int k = 0; k < NPB_OBS_DIM; k++) {
      const int idx = k * NPB_WAVE + lane, r = idx / NPB_OBS_DIM, c = idx % NPB_OBS_DIM;
      const uint32_t slot_r = npd_log_slot(s, r);
      if (((s.rows >> r) & 1u) && slot_r < cap) R.D.final_obs[(size_t)slot_r * NPB_OBS_DIM + c] = obs[block_base * NPB_OBS_DIM + idx];
    }
  }
  if (!ended) return;
  const bool copy = store && R.D.first_created;
  for (int j = 0; R.s_first_created && j < R.n_keys; j++) {  /* the plant's summary cells as of this step (the fold ran before this launch), then "never" and 0 again */
    const size_t cell = (size_t)j * (size_t)n_plants + p;
    if (copy) {
      const size_t out = (size_t)j * (size_t)cap + slot;
      R.D.first_created[out] = R.s_first_created[cell];
      R.D.first_completed[out] = R.s_first_completed[cell];
      R.D.n_created[out] = R.s_n_created[cell];
      R.D.n_completed[out] = R.s_n_completed[cell];
    }
    if (R.D.clear_summary) {
      ((uint64_t *)R.s_first_created)[cell] = 0x7ff0000000000000ull;
      ((uint64_t *)R.s_first_completed)[cell] = 0x7ff0000000000000ull;
      R.s_n_created[cell] = 0;
      R.s_n_completed[cell] = 0;
    }
  }
  if (!R.stats) return;
  if (store && R.stats->cause) R.stats->cause[slot] = (int32_t)R.stats->task_cause[p];      /* why it ended: the task's cause word (npb_set_episode_record_task) */
  /* the plant's column statistics as of this step (their fold ran before this launch), then the empty values again (npd_column_stats.h) */
  const npb_column_stats_t st = R.stats->st;
  const npb_episode_record_stats_desc_t rs = R.stats->rs;
  if (store && rs.n_samples) rs.n_samples[slot] = st.n_samples[p];
  if (rs.clear) st.n_samples[p] = 0;
#define NPD_RECORD_STAT(name, empty) \
    if (store && rs.name) rs.name[(size_t)c * (size_t)cap + slot] = st.name[cell]; \
    if (rs.clear && st.name) st.name[cell] = (empty);
  for (int c = 0; c < st.n_cols; c++) {
    const size_t cell = (size_t)c * (size_t)n_plants + p;
    NPD_RECORD_STAT(min, __longlong_as_double(0x7ff0000000000000ll))
    NPD_RECORD_STAT(max, __longlong_as_double((long long)0xfff0000000000000ull))
    NPD_RECORD_STAT(sum, 0.0)
    NPD_RECORD_STAT(sumsq, 0.0)
    NPD_RECORD_STAT(last, __longlong_as_double(0x7ff8000000000000ll))
    NPD_RECORD_STAT(first_beyond, __longlong_as_double(0x7ff0000000000000ll))
    NPD_RECORD_STAT(n_beyond, 0)
  }
#undef NPD_RECORD_STAT
}
/* C: the handle's carried counters; start: its carried bank entries or NULL; summary: the handle's summary while the records copy or clear it, else NULL;
 * record_stats: the handle's device copy of its column statistics and the record-side columns that take them, or NULL */
static void NPB_LAUNCHER(episode_records)(int n_plants, size_t npad, const void *arena, const uint8_t *done, const double *reward, const double *obs,
                                          const uint32_t *trip_flags, npb_episode_counters_t C, const int32_t *start, int max_steps, int step,
                                          const npb_episode_records_desc_t *D, const npb_maint_summary_desc_t *summary, const npb_record_stats_t *record_stats,
                                          hipStream_t stream) {
  npd_episode_records_t R;
  R.stats = record_stats;
  R.D = *D; R.len = C.len; R.ret = C.ret; R.index = C.index; R.start = start; R.max_steps = max_steps; R.step = step;
  R.s_first_created = summary ? summary->first_created : nullptr; R.s_first_completed = summary ? summary->first_completed : nullptr;
  R.s_n_created = summary ? summary->n_created : nullptr; R.s_n_completed = summary ? summary->n_completed : nullptr;
  R.n_keys = summary ? summary->n_keys : 0;
  hipLaunchKernelGGL(npb_episode_records_kernel, dim3((unsigned)(NPD_NPAD(npad) / NPB_WAVE)), dim3(NPB_WAVE), 0, stream, n_plants, npad,
                     (const npd_real_t *)arena, done, reward, obs, trip_flags, R);
}

/* the per-plant column statistics (npb_set_column_stats): the fold kernel and its launcher */
#include "npd_column_stats.h"

/* state windows around events (npb_set_event_windows): the per-step kernel and its launcher */
#include "npd_event_windows.h"

/* the caller's reward terms and termination rules (npb_set_task): the per-step kernel and its launcher */
#include "npd_task.h"

/* the caller's policy inputs (npb_set_features): the frame-stack kernel and its launcher */
#include "npd_features.h"

/* the caller's policy outputs (npb_set_controls): the decode kernel in front of the step and its launcher */
#include "npd_controls.h"

/* order rules on the controls' axes (npb_set_control_orders): the kernel behind the decode and its launcher */
#include "npd_control_orders.h"

/* running observation and reward normalisation (npb_set_normalizer): the partials kernel of a fold and its launcher */
#include "npd_normalizer.h"

/* not const: clang emits a namespace-scope const into the device code too, where these host functions do not exist */
extern "C" npb_attach_launchers_t NPB_LAUNCHER(attach_table) = {
  NPB_LAUNCHER(sample), NPB_LAUNCHER(episode_records), NPB_LAUNCHER(column_stats_fold), NPB_LAUNCHER(event_windows),
  NPB_LAUNCHER(task), NPB_LAUNCHER(features), NPB_LAUNCHER(controls), NPB_LAUNCHER(normalizer),
  NPB_LAUNCHER(control_orders),
};
