/* npb_kernels.h -- host-callable launchers of the device kernels (internal to libnpb.so).
 * npb_kernels.hip (the plant kernels: npb_launchers_t) and npb_attachments.hip (the per-step attachments that read the arena:
 * npb_attach_launchers_t) are compiled twice each: 8-byte arena columns (npb_launch_table, npb_launch_attach_table) and 4-byte columns for
 * fp32 storage (npb32_launch_table, npb32_launch_attach_table, -DNPB_BUILD_F32); the arena pointer is void* here and typed inside each
 * translation unit.  A handle picks its two tables once, by its storage type.  What never sees an arena element is compiled once
 * (npb_storage_free.hip) and declared behind the tables. */
#ifndef NPB_KERNELS_H
#define NPB_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/npb_params.h"
#include "../../include/npb_maint.h"
#include "../../include/npb.h"
#ifdef __cplusplus
extern "C" {
#endif
/* where a restore copies from: the snapshot (npb_snapshot), or a start bank (npb_set_start_bank) with its slot columns
 * (npb_set_start_slots).  Entry s of the source is lane s of an arena in a handle's own layout; a snapshot has the bank fields NULL */
typedef struct {
  const void *arena;        /* the snapshot arena, or the bank arena: M plants in the layout of the handle it was copied from */
  size_t N;                 /* its packed pitch: pitch | segment size << 32 (NPD_SEGMENT) */
  int M;                    /* a bank's entries */
  int32_t *next_slot;       /* the caller's [n], NULL for the snapshot: a restored plant takes entry ((next_slot % M) + M) % M, then next_slot = (s + advance) % M */
  int32_t *episode_start;   /* the caller's [n], or NULL: the entry a restored plant took */
  int advance;
  int32_t *start;           /* carried [pitch]: the entry of each plant's running episode, -1 = not from the bank */
  int32_t *out_start;       /* the caller's [n], or NULL: the episode kernel's copy of `start` as of each step */
} npb_source_t;
/* a side block: per-plant fp64 rows that belong to a plant's state and live beside the arena.  A restore takes each along: entry s of
 * src (a packed [rows][src_pitch] copy, recorded with the snapshot or the bank) -> plant p of the live rows; live NULL = the block is off.
 * NPB_SIDE_CMAINT: the side state of the component maintenance (npb_set_component_maintenance), live = [NPB_CMAINT_SIDE_DOUBLES][pitch], copied
 * member by member.  NPB_SIDE_DIAG: the carried diagnostics rows (include/npb.h NPB_DIAG_CARRIED, npb_carry_diagnostics), src in table order,
 * live = the caller's diagnostics buffer ([NPB_DIAG_DIM][pitch], indexed by the global plant number: that buffer is not segmented) */
enum { NPB_SIDE_CMAINT, NPB_SIDE_DIAG, NPB_SIDE_COUNT };
typedef struct { double *live; const double *src; size_t pitch, src_pitch; } npb_side_restore_t;
typedef struct { npb_side_restore_t block[NPB_SIDE_COUNT]; } npb_side_restores_t;
/* the maintenance event log (npb_set_maintenance_log): the caller's records and cursor; cursor NULL = off */
typedef struct npd_maint_log_t { npb_maint_event_t *records; uint32_t *cursor; int capacity; } npd_maint_log_t;
/* the episode counters a restore zeroes and the episode index it bumps with them (npb_set_autoreset), each [pitch] or NULL; out_index =
 * the caller's column the episode kernel fills (npb_set_episode_index_buffer) */
typedef struct { int32_t *len; double *ret; int32_t *index; int32_t *out_index; } npb_episode_counters_t;
/* one side row of a sampler (npb_sampler_create): watched plant p's value is element p * plant_stride of `row` (the source's base moved
 * to the row), of type NPB_SAMPLE_* */
typedef struct { const void *row; int64_t plant_stride; int type; int pad_; } npb_sample_row_t;
/* one column of npb_set_column_stats as the fold kernel reads it.  kind 0 / 1 / 2: an arena member (col, sub; 0 carried real, 1 output real
 * stored as float, 2 int32); kind 3 + NPB_SAMPLE_*: a side row, plant p's value is element p * plant_stride of `row`.  direction / limit:
 * the column's limit (0 = none) */
typedef struct { const void *row; int64_t plant_stride; int col, sub, kind, direction; double limit; } npb_colstat_col_t;
/* the handle's column statistics: the columns (device, n_cols of them; cols NULL = stats off) and the caller's tables as the descriptor
 * names them, [n_cols][n_plants] each or NULL, n_samples [n_plants] */
typedef struct {
  const npb_colstat_col_t *cols; int n_cols;
  double *min, *max, *sum, *sumsq, *last, *first_beyond; int32_t *n_beyond, *n_samples;
} npb_column_stats_t;
/* npb_set_episode_record_stats: what the records kernel needs of the statistics, kept in DEVICE memory by the handle and passed as one
 * pointer (NULL = off), so that the kernel's argument block, and with it the kernel without statistics, stays what it was */
typedef struct {
  npb_column_stats_t st; npb_episode_record_stats_desc_t rs;
  /* npb_set_episode_record_task: the task's cause column [n_plants] and the record-side column [capacity] that takes it; NULL = not taken.
   * Without npb_set_episode_record_stats st and rs are zero here: no column, no table, nothing cleared */
  const uint32_t *task_cause; int32_t *cause;
} npb_record_stats_t;
/* npb_set_task (npd_task.h): one reward term and one termination rule as the kernel reads them.  c: the column (direction / limit: those of
 * BEYOND and EXCESS); r: the second column of ABS_ERR / SQ_ERR where ref_col != 0, else `ref`; prev_row: the DELTA term's row of the
 * previous-sample table, -1 for every other kind */
typedef struct { npb_colstat_col_t c, r; double w, ref; int kind, ref_col; uint32_t mask; int prev_row; } npb_task_term_col_t;
typedef struct { npb_colstat_col_t c; double terminal; int mode; uint32_t mask; } npb_task_rule_col_t;
/* the handle's task: the terms and rules (device, one allocation with the state below; terms NULL = off), the caller's outputs, and the
 * state the handle owns -- prev double [n_delta][n_plants], and per plant the primed flag and the episode index last seen */
typedef struct {
  const npb_task_term_col_t *terms; const npb_task_rule_col_t *rules; int n_terms, n_rules, n_delta; double bias;
  double *reward; uint8_t *done; uint32_t *cause; double *terms_out;
  double *prev; int32_t *primed, *seen;
} npb_task_t;
/* npb_set_event_windows (npd_event_windows.h): one trigger as the kernel reads it -- its column (direction / limit: those of
 * NPB_TRIGGER_MODE_BEYOND), the mode and the mask of NPB_TRIGGER_MODE_BITS_RISE */
typedef struct { npb_colstat_col_t c; int mode; uint32_t mask; } npb_event_trigger_col_t;
/* the caller's record columns, `capacity` entries each (npb_event_windows_desc_t) */
typedef struct {
  int capacity;
  int32_t *plant, *episode, *trigger, *step, *n_pre, *n_post, *flags, *retriggers; uint32_t *fired;
  double *time, *times, *values; uint32_t *cursor;
} npb_event_window_records_t;
/* the handle's event windows: the recorded columns and the triggers (device, one allocation with everything below; cols NULL = off), the
 * window shape, and the state the handle owns -- the ring [H][n_cols + 1][n_plants] (the plant clock as the extra column), the previous
 * value of every trigger source [n_triggers][n_plants], and per plant: samples in the ring (0 = unprimed), the step a capture is due (-1 =
 * idle), the episode index last seen, and of an armed capture the trigger step, its n_pre, the lowest trigger, the fired set, the
 * triggers since, and the plant clock */
typedef struct {
  const npb_colstat_col_t *cols; const npb_event_trigger_col_t *triggers; int n_cols, n_triggers, pre, post;
  double *ring, *prev, *a_time;
  int32_t *valid, *due, *seen, *a_step, *a_n_pre, *a_trigger, *a_retriggers; uint32_t *a_fired;
  npb_event_window_records_t D;
} npb_event_windows_t;
/* npb_set_features (npd_features.h): one column as the kernel reads it.  c: the column; r: the second column where ref_col != 0 (a setpoint
 * error), else the constant `ref`; kind: NPB_FEATURE_KIND_*; live: bit 0 / bit 1 = c / r is read in a FRESH frame too (an arena member, or a
 * source the caller marked live), else c takes `fresh` and r takes `ref` there */
typedef struct { npb_colstat_col_t c, r; double scale, ref, lo, hi, nan_to, fresh; int kind, ref_col; uint32_t mask; int live; } npb_feature_col_t;
/* the handle's features: the columns (device, one allocation with the state below; cols NULL = off), the stack depth, the caller's out
 * [n_plants][stack][n_cols] and final (or NULL) of float or double, and per plant the primed flag and the episode index last seen */
typedef struct {
  const npb_feature_col_t *cols; int n_cols, stack, out_f64;
  void *out, *final;
  int32_t *primed, *seen;
} npb_features_t;
/* npb_set_controls (npd_controls.h): the axes as the caller wrote them (uniform over the launch: kernel arguments), the caller's input
 * tensor and held / prev [n_axes][n_plants], and of the handle's one allocation (age; NULL = off) the bookkeeping words and the two input
 * columns [n_plants] (column[input]; NULL where no axis fills that input) */
typedef struct {
  npb_control_axis_t axes[NPB_CONTROLS_AXES_MAX]; int n_axes, interval, in_f64;
  const void *in; double *held, *prev, *column[NPB_CONTROL_INPUT_COUNT];
  int32_t *age, *primed, *seen;
} npb_controls_t;
/* npb_set_control_orders (npd_control_orders.h): the rules as the check left them (uniform over the launch: kernel arguments; a unit or
 * option the family's call ignores is 0), the controls' held and age they read, the caller's fired [n_orders][n_plants], the handle's
 * since [n_orders][n_plants] (its one allocation; NULL = off) */
typedef struct {
  npb_control_order_t rule[NPB_CONTROL_ORDERS_MAX]; int n_orders, interval;
  const double *held; const int32_t *age;
  double *fired; int32_t *since;
} npb_control_orders_t;
/* npb_set_rollout (npd_rollout.h): the caller's buffers as the descriptor names them, the shapes they were bound with (cells = K * C of the
 * features, n_axes of the controls or 0, the element sizes of obs and act), and of the handle: n_final int32 [n_plants] (its one
 * allocation; NULL = off) and the host cursor t */
typedef struct {
  int32_t *n_final;
  npb_rollout_desc_t D;
  int cells, n_axes, obs_bytes, act_bytes, t;
} npb_rollout_t;
/* npb_set_normalizer (npd_normalizer.h, npb_minibatch.hip): one stream as the partials kernel and the finish kernel read it.  c: the
 * column whose raw samples are folded (unused by the return stream); ref0 / scale0: the column's own ref and scale (the return stream: 0.0
 * and 1.0), the shift of the first fold and what the table holds while count == 0; feat_col: the features' column whose table entry the
 * finish kernel rewrites, -1 for the return stream */
typedef struct { npb_colstat_col_t c; double ref0, scale0; int feat_col, pad_; } npb_norm_stream_t;
#define NPB_NORM_STREAMS_MAX (NPB_FEATURES_COLS_MAX + 1)
/* the handle's normaliser: the streams (device, one allocation with everything below but norm_reward and feat_cols; streams NULL = off);
 * the state count, mean, M2 [n_streams] and beside it scale [n_streams], what the table holds (the reward kernel reads the return
 * stream's); with the return stream ret [n_plants], primed, seen, ended [n_plants]; the partials, vector v = 3 * stream + {0: s1, 1: s2,
 * 2: the count as a double} at partial + v * ws_stride, every level of the tree one behind the other (npb_moments_workspace); the
 * caller's norm_reward; the features' device table */
typedef struct {
  const npb_norm_stream_t *streams; int n_streams, n_cols, reward_on;
  double eps, gamma, clip;
  double *count, *mean, *M2, *scale;
  double *ret; int32_t *primed, *seen, *ended;
  double *partial; size_t ws_stride;
  double *norm_reward;
  npb_feature_col_t *feat_cols;
} npb_normalizer_t;
typedef struct {
  int (*step)(const npb_params_t *P, int n_plants, size_t npad, void *arena, const int32_t *action,
              const double *magnitude, const double *setpoint, const double *noise_z, const double *cw_temp,
              double *obs, double *reward, uint8_t *done, uint32_t *trip_flags, double *info, int variant, double *diag, size_t diag_pitch,
              const npb_maint_table_t *maint_table, void *maint_side, int32_t *maint_counts, hipStream_t stream);
  void (*maint)(size_t npad, void *arena, void *maint_side, int32_t *counts, int n_plants, hipStream_t stream);
  void (*observe)(int mode, int n_plants, size_t npad, const void *arena, double *obs, hipStream_t stream);
  void (*init)(const npb_params_t *P, int n_plants, size_t npad, void *arena, const uint8_t *mask, hipStream_t stream);
  void (*reset)(const npb_params_t *P, int n_plants, size_t npad, void *arena, const uint8_t *mask, int steady, hipStream_t stream);
  /* kind: 0 carried real, 1 output real (float), 2 int32; buffers: double for reals, int32 for ints */
  void (*field_get)(const void *arena, size_t npad, int col, int sub, int kind, void *out, int n, hipStream_t stream);
  void (*field_set)(void *arena, size_t npad, int col, int sub, int kind, const void *in, int n, hipStream_t stream);
  void (*gather)(const void *arena, size_t npad, const int *plan_dev, int n_fields, double *out, int n, hipStream_t stream);
  /* episodes: src = the snapshot or a bank with slots (npb_source_t); maint_side / maint_counts NULL unless params.maint_enabled */
  void (*restore)(int n_plants, size_t npad, void *arena, npb_source_t src, const uint8_t *mask, npb_episode_counters_t C,
                  void *maint_side, int32_t *maint_counts, npb_side_restores_t side, hipStream_t stream);
  void (*episode)(int mode, int n_plants, size_t npad, void *arena, npb_source_t src, const uint8_t *done, const double *reward,
                  double *obs, npb_episode_counters_t C, int32_t *out_len, double *out_ret, uint8_t *out_truncated,
                  double *final_obs, int max_steps, void *maint_side, int32_t *maint_counts, npb_side_restores_t side, hipStream_t stream);
  /* npb_perform_maintenance: the caller's [n_plants] order columns (bearing / target_level / success may be NULL) and the maintenance
   * event log */
  void (*operator_maint)(int n_plants, size_t npad, void *arena, const int32_t *action, const int32_t *pump, const int32_t *bearing,
                         const double *target_level, uint8_t *success, npd_maint_log_t log, hipStream_t stream);
  /* npb_perform_component_maintenance: the caller's [n_plants] order columns (unit / option / amount / success may be NULL), the component
   * kinds the handle's mode carries (bit k = NPB_COMPONENT_* k) and the maintenance event log */
  void (*operator_component_maint)(int n_plants, size_t npad, void *arena, const int32_t *action, const int32_t *unit, const int32_t *option,
                                   const double *amount, uint8_t *success, unsigned kinds, npd_maint_log_t log, hipStream_t stream);
  /* npb_perform_turbine_maintenance: the caller's [n_plants] order columns (unit / success may be NULL), whether the handle's mode steps
   * the turbine, and the event log */
  void (*operator_turbine_maint)(int n_plants, size_t npad, void *arena, const int32_t *action, const int32_t *unit, uint8_t *success, int turbine,
                                 npd_maint_log_t log, hipStream_t stream);
  /* npb_set_component_maintenance: the whole automatic-maintenance rule, pumps, generators and condenser in one queue, as a launch of its own
   * behind the plain step kernel; maint_side = the rule's constants, cm_side = the component table and side state */
  void (*maint_all)(size_t npad, void *arena, void *maint_side, void *cm_side, int32_t *counts, int n_plants, double *diag, size_t diag_pitch,
                    hipStream_t stream);
} npb_launchers_t;
extern npb_launchers_t npb_launch_table, npb32_launch_table;
/* the per-step attachments that read the arena (npb_attachments.hip) */
typedef struct {
  /* npb_sampler_sample: rows = n_fields arena members (plan_dev as for gather) then the side rows, of the plants ids_dev[0 .. n_watched):
   * out[r * n_watched + j], one launch */
  void (*sample)(const void *arena, size_t npad, const int *plan_dev, int n_fields, const npb_sample_row_t *side_dev, int n_rows,
                 const int32_t *ids_dev, int n_watched, double *out, hipStream_t stream);
  /* npb_set_episode_records: one record per episode that ends on this step, before the episode kernel does its bookkeeping.  C / start: the
   * handle's carried counters and bank entries (start NULL = no bank); step: npb_step calls since the records were switched on; summary: the
   * handle's work-order summary while the records copy or clear it, else NULL; record_stats: the handle's device copy of its column
   * statistics and of the record-side columns that take them (npb_set_episode_record_stats), or NULL */
  void (*episode_records)(int n_plants, size_t npad, const void *arena, const uint8_t *done, const double *reward, const double *obs,
                          const uint32_t *trip_flags, npb_episode_counters_t C, const int32_t *start, int max_steps, int step,
                          const npb_episode_records_desc_t *D, const npb_maint_summary_desc_t *summary, const npb_record_stats_t *record_stats,
                          hipStream_t stream);
  /* npb_set_column_stats (npd_column_stats.h): one sample of every column of every plant folded into the tables, one launch */
  void (*column_stats_fold)(const void *arena, size_t npad, const npb_column_stats_t *S, int n_plants, hipStream_t stream);
  /* npb_set_event_windows (npd_event_windows.h): the sample of this step into every plant's ring, the triggers, and the windows that are
   * due.  step: npb_step calls since the windows were set; index: the handle's carried episode indices or NULL; len / done / max_steps:
   * the carried lengths and the step's done column while the autoreset is on (the episode kernel's rule), else len NULL */
  void (*event_windows)(const void *arena, size_t npad, const npb_event_windows_t *W, int n_plants, int step, const int32_t *index,
                        const int32_t *len, const uint8_t *done, int max_steps, hipStream_t stream);
  /* npb_set_task (npd_task.h): every plant's task reward, termination flag and cause word from the end-of-step state and the step's
   * outputs; index: the handle's carried episode indices or NULL */
  void (*task)(const void *arena, size_t npad, const npb_task_t *T, int n_plants, const int32_t *index, hipStream_t stream);
  /* npb_set_features (npd_features.h): mode 0 = this step's frame into every plant's stack (shift or fill), 1 = the plants the episode
   * kernel restarted (their stacks to `final`, then the fresh frame), 2 = the unprimed plants' fresh frame; index: the handle's carried
   * episode indices or NULL */
  void (*features)(const void *arena, size_t npad, const npb_features_t *F, int n_plants, int mode, const int32_t *index, hipStream_t stream);
  /* npb_set_controls (npd_controls.h): every plant's row of the caller's input decoded in front of the step -- the actuators moved, the
   * input columns filled, held / prev kept; index: the handle's carried episode indices or NULL */
  void (*controls)(void *arena, size_t npad, const npb_controls_t *C, const npb_params_t *P, int n_plants, const int32_t *index, hipStream_t stream);
  /* npb_set_normalizer (npd_normalizer.h): this step's raw samples of every stream as partial sums of the pinned tree, one workgroup per
   * 256 plants, and with the return stream every plant's discounted return carried; reward / done: the columns the episode kernel reads;
   * index: the handle's carried episode indices or NULL */
  void (*normalizer)(const void *arena, size_t npad, const npb_normalizer_t *Z, int n_plants, const int32_t *index, const double *reward,
                     hipStream_t stream);
  /* npb_set_control_orders (npd_control_orders.h): behind the controls kernel -- which rule fires on which plant, since / fired kept,
   * and the service of the firing plants, with its records in the maintenance event log */
  void (*control_orders)(void *arena, size_t npad, const npb_control_orders_t *O, npd_maint_log_t log, int n_plants, hipStream_t stream);
} npb_attach_launchers_t;
extern npb_attach_launchers_t npb_launch_attach_table, npb32_launch_attach_table;
/* the same for either storage type (npb_storage_free.hip) */
void npb_launch_maint_consts(const npb_params_t *P, const npb_maint_table_t *T, npd_maint_log_t log, void *host_out);
size_t npb_launch_maint_consts_bytes(void);
size_t npb_launch_maint_side_bytes(size_t npad);
size_t npb_launch_maint_cache_offset(void);
size_t npb_launch_cmaint_side_bytes(size_t pitch);
size_t npb_launch_cmaint_state_offset(void);
void npb_launch_cmaint_init(void *cm_side, size_t pitch, const uint8_t *mask, int n_plants, hipStream_t stream);
void npb_launch_touch(size_t npad, double *arena, hipStream_t stream);
void npb_launch_episode_clear(const uint8_t *mask, int32_t *len, double *ret, int32_t *index, int32_t *start, int n_plants, size_t npad, hipStream_t stream);
/* the carried diagnostics rows of a diagnostics buffer (`live`, [NPB_DIAG_DIM][live_pitch]) into `packed`, [NPB_DIAG_NUM_CARRIED][packed_pitch] in
 * table order, for the plants below `lanes` */
void npb_launch_diag_carried_pack(const double *live, size_t live_pitch, double *packed, size_t packed_pitch, size_t lanes, hipStream_t stream);
/* the plants of mask (NULL = every lane below `lanes`) to values[k] per carried row, a NaN = the row is kept */
typedef struct { double v[NPB_DIAG_NUM_CARRIED]; } npb_diag_carried_values_t;
void npb_launch_diag_carried_put(double *live, size_t live_pitch, const uint8_t *mask, int n_plants, size_t lanes, npb_diag_carried_values_t values,
                                 hipStream_t stream);
/* npb_set_maintenance_summary (npd_maint_summary.h): one fold of the log's records [*D->folded, min(*log.cursor, log.capacity)) into the
 * caller's tables, the bookkeeping words rewritten by the last block (ticket: the handle's device word, zero between folds); and the rows of
 * the plants of mask (NULL = all) back to +inf and 0 */
void npb_launch_maint_summary_fold(const npb_maint_summary_desc_t *D, npd_maint_log_t log, uint32_t *ticket, int n_plants, hipStream_t stream);
void npb_launch_maint_summary_clear(const npb_maint_summary_desc_t *D, const uint8_t *mask, int n_plants, hipStream_t stream);
/* npb_column_stats_clear (npd_column_stats.h): the cells of the plants of mask (NULL = all) back to the empty values in every table kept */
void npb_launch_column_stats_clear(const npb_column_stats_t *S, const uint8_t *mask, int n_plants, hipStream_t stream);
/* npb_event_windows_clear (npd_event_windows.h): the plants of mask (NULL = all) unprimed, their rings empty, an armed capture dropped */
void npb_launch_event_windows_clear(const npb_event_windows_t *W, const uint8_t *mask, int n_plants, hipStream_t stream);
/* npb_task_clear, npb_features_clear, npb_controls_clear: the plants of mask (NULL = all) unprimed in that attachment's `primed` column */
void npb_launch_unprime(int32_t *primed, const uint8_t *mask, int n_plants, hipStream_t stream);
/* npb_set_normalizer, the same for either storage type: neither touches the arena.
 * finish (npb_minibatch.hip, IEEE division and root): one workgroup ends the tree over the `groups` partials of every vector (0 = no batch:
 *   the state stays), merges, writes count, mean, M2 and scale, and ref and scale into the features' table entries.
 * reward (npd_normalizer.h): norm_reward, ended, primed and seen of every plant; carry != 0: the return is carried here (frozen: the partials
 *   kernel, which carries it otherwise, has not run) */
void npb_launch_normalizer_finish(const npb_normalizer_t *Z, int groups, hipStream_t stream);
/* one normaliser across shards (npb_minibatch.hip): base, device [3][n_streams], what the shards agreed on last.
 * delta: out [3][n_streams] = the population folded since the base.  combine: the base merged with deltas [n_shards][3][n_streams] in
 *   ascending order into the state AND the base; the caller follows it with npb_launch_normalizer_finish(Z, 0) for scale and the table */
void npb_launch_normalizer_delta(const npb_normalizer_t *Z, const double *base, double *out, hipStream_t stream);
void npb_launch_normalizer_combine(const npb_normalizer_t *Z, double *base, const double *deltas, int n_shards, hipStream_t stream);
void npb_launch_normalizer_reward(const npb_normalizer_t *Z, int n_plants, const int32_t *index, const double *reward, const uint8_t *done, int carry,
                                  hipStream_t stream);
/* npb_set_rollout (npd_rollout.h), the same for either storage type: none of them touches the arena.
 * pre: the three copies into slot R->t in front of the controls kernel, feat_out and ctl_in the tensors the features and the controls are
 *   bound to (ctl_in NULL without controls).
 * post: reward, ended, episode and the terminal stacks of slot R->t, behind features pass A; len / index: the carried lengths and episode
 *   indices while the autoreset is on, else NULL.
 * cut: bit 2 into ended[R->t - 1] for the plants of mask (NULL = all); R->t > 0.
 * advantages: the recurrence over the slots [0, R->t), gl = gamma * lam */
void npb_launch_rollout_pre(const npb_rollout_t *R, const void *feat_out, const void *ctl_in, int n_plants, hipStream_t stream);
void npb_launch_rollout_post(const npb_rollout_t *R, const void *feat_out, const double *reward, const uint8_t *done, const int32_t *len,
                             const int32_t *index, int max_steps, int n_plants, hipStream_t stream);
void npb_launch_rollout_cut(const npb_rollout_t *R, const uint8_t *mask, int n_plants, hipStream_t stream);
void npb_launch_rollout_advantages(const npb_rollout_t *R, const npb_rollout_advantages_desc_t *A, double gl, int n_plants, hipStream_t stream);
#ifdef __cplusplus
}
#endif
#endif
