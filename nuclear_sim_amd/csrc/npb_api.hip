/*
 * npb_api.hip -- the C ABI of libnpb.so (include/npb.h): handle, SoA arena, field access, step launch.
 * Host code only; the kernels live in npb_kernels.hip.
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/npb.h"
#include "npb_kernels.h"
#include "npb_noise.h"
#include "npb_minibatch.h"
#include "npb_policy.h"
#include "npb_ppo.h"

/* a side block's rows as recorded with a snapshot or a bank: a packed [rows][pitch] copy beside that arena, or NULL; its allocation */
struct SideCopy { double *rows; size_t pitch, doubles; };

/* npb_sampler_create: what one sampler keeps on the device, one allocation: [side rows][plan: 3 ints per field][plant ids] */
struct Sampler { void *dev; const npb_sample_row_t *side; const int *plan; const int32_t *ids; int n_fields, n_rows, n_watched; };

struct NpbHandle {
  npb_params_t params;
  int n_plants;
  int device;
  size_t pitch;        /* n_plants rounded up to a multiple of the wave size */
  size_t seg;          /* plants per arena segment (npd_arena.h, "segmented arena"), 0 = the arena is one [column][pitch] block */
  int storage;         /* NPB_STORAGE_F64 | NPB_STORAGE_F32: element type of the real-valued columns */
  const npb_launchers_t *K;   /* the launchers of that storage type's build of npb_kernels.hip */
  const npb_attach_launchers_t *A;   /* and of npb_attachments.hip */
  size_t real_bytes;   /* 8 | 4 */
  void *f64;           /* the arena: [NPB_TOTAL_COL64][pitch] 8-byte columns, or [NPB_TOTAL_COL32][pitch] 4-byte ones */
  double *convert;     /* one staging column (pitch doubles) used by get/set_field with host buffers */
  void *maint_side;      /* automatic maintenance: the rule's constants as the device reads them + the screen's cooldown cache (npb_kernels.hip; behind the staging column) */
  std::vector<char> maint_consts_host;
  double *diag; size_t diag_pitch; /* npb_set_diagnostics: the caller's [NPB_DIAG_DIM][diag_pitch] buffer, or NULL */
  /* npb_carry_diagnostics: the carried rows of that buffer (include/npb.h NPB_DIAG_CARRIED) are plant state the handle takes along */
  bool diag_carry;
  int32_t *maint_counts;           /* npb_set_maintenance_count_buffer: the caller's [n_plants] int32 column, or NULL */
  npd_maint_log_t maint_log;       /* npb_set_maintenance_log: the caller's records and cursor, or NULL; no records = no cursor and capacity 0 */
  bool maint_cache_stale;          /* the cooldown cache of the step kernels' maintenance screen must be zeroed before the next step */
  /* npb_set_maintenance_summary: the caller's keys, tables and words, and the fold kernel's ticket word (device, zero between folds; allocated
   * when a summary is first set) */
  bool summary_on; npb_maint_summary_desc_t summary; uint32_t *summary_ticket;
  int last_kernel;                 /* NPB_KERNEL_*: what the last npb_step launched */
  int step_kernel;                 /* 0 = chosen by batch size, 1 = one-wave kernel, 2 = two-wave kernel, 3 = its two-waves-per-SIMD build, 4 = one-wave with streaming stores, 5 = four-wave kernel (npb_set_step_kernel) */
  npb_maint_table_t maint_table;   /* thresholds of the automatic maintenance (include/npb_maint.h) */
  bool maint_table_custom;         /* set through npb_set_maintenance_table: the table is then taken as it is */
  /* npb_set_component_maintenance: automatic maintenance of the steam generators and the condenser in one queue with the pumps' */
  bool cm_on; npb_component_maint_table_t cm_table;
  void *cm_side;       /* [the table as the device reads it][NPB_CMAINT_SIDE_DOUBLES][pitch] doubles (npb_kernels.hip), allocated when first switched on */
  /* the side blocks (g_side below) as npb_snapshot recorded them from this handle and as npb_set_start_bank did from the bank handle, in
   * that handle's pitch */
  struct { SideCopy snap, bank; } side[NPB_SIDE_COUNT];
  void *snap;          /* npb_snapshot: the episode-start arena, the arena's layout, or NULL */
  int32_t *ep_len; double *ep_ret; /* npb_set_autoreset: carried steps / summed reward of each plant's running episode ([pitch] each), or NULL */
  int32_t *ep_index;   /* with them: the number of each plant's running episode ([pitch]), bumped wherever ep_len is zeroed */
  int32_t *ep_out_index;   /* npb_set_episode_index_buffer: the caller's column, or NULL */
  bool autoreset; int max_episode_steps;
  int32_t *ep_out_len; double *ep_out_ret; uint8_t *ep_out_truncated; double *ep_final_obs;   /* npb_set_episode_buffers: the caller's columns, or NULL */
  void *bank; size_t bank_bytes; size_t bank_N; int bank_M;   /* npb_set_start_bank: the bank arena (src's layout), its allocation, its packed pitch (NPB_N of src), its entries */
  int32_t *ep_start;   /* with a bank: carried bank entry of each plant's running episode, -1 = not from the bank ([pitch]), or NULL */
  int32_t *next_slot; int32_t *slot_start; int slot_advance;  /* npb_set_start_slots: the caller's columns (next_slot NULL = no slots) */
  int32_t *ep_out_start;                                       /* npb_set_episode_start_buffer: the caller's column, or NULL */
  void *noise; npb_noise_t noise_g;  /* npb_noise_seed / npb_noise_set_state: the heat-source noise generators (npb_noise.hip), or NULL */
  /* npb_profile_seed: the power profile's generators (a second npb_noise_t), its per-plant columns ([NPB_PROFILE_SIDE][pitch]), its
   * horizon and the rows made of the current profile (all plants advance together), and the block its draws go through */
  void *prof; npb_noise_t prof_g; double *prof_side; int prof_steps, prof_pos; double *prof_z; size_t prof_z_rows;
  /* the seeds npb_noise_seed / npb_profile_seed were last given: each plant's own, which a restart under episode streams uses again */
  std::vector<uint32_t> noise_seeds, prof_seeds;
  /* npb_set_episode_streams: the mode's blocks, per-plant columns and seed tables (one allocation, es_mem), as the kernels read them; the
   * next row of each block a step takes (block = none left); the caller's output columns; whether bank seed tables were given */
  bool es_on; npb_episode_streams_t es; void *es_mem; int es_noise_cur, es_prof_cur; double *es_noise_out, *es_setpoint_out, *es_target_out; bool es_tables;
  /* npb_set_episode_records: the caller's record columns and cursor, and the npb_step calls since they were switched on */
  bool er_on; npb_episode_records_desc_t er; int er_step;
  /* the per-step attachments (attachment_alloc ... state_copy below): each struct is what its kernel reads, and the member named here is
   * the base of its device allocation, NULL = off.
   * npb_set_column_stats: the columns on the device (base cs.cols) and the caller's tables; npb_set_episode_record_stats: the record-side
   * columns that take them */
  npb_column_stats_t cs; bool ers_on; npb_episode_record_stats_desc_t ers;
  npb_record_stats_t *ers_dev;      /* what the records kernel reads of both (device, allocated on first use, uploaded by npb_set_episode_record_stats) */
  /* npb_set_event_windows: the columns, triggers, ring and bookkeeping on the device (base ew.cols, ew_bytes of them), the caller's record
   * columns, and the npb_step calls since they were set */
  npb_event_windows_t ew; size_t ew_bytes; int ew_step;
  /* npb_set_task: the terms, rules, previous samples and bookkeeping on the device (base task.terms) and the caller's outputs;
   * npb_set_episode_record_task: the record-side column that takes the cause word */
  npb_task_t task; bool ert_on; int32_t *ert_cause;
  /* npb_set_features: the columns and the bookkeeping on the device (base feat.cols) and the caller's tensors */
  npb_features_t feat;
  std::vector<npb_feature_col_t> feat_host;      /* the table as npb_set_features uploaded it: the columns' own ref and scale */
  /* npb_set_normalizer: the streams, the running statistics, the return carry and the partials on the device (base norm.streams), the
   * caller's norm_reward, and whether a step folds (npb_normalizer_training) */
  npb_normalizer_t norm; bool norm_training;
  /* npb_set_controls: the axes, the caller's tensors and the handle's bookkeeping and input columns (base ctl.age); ctl_axis[input]: the
   * axis that fills that input column, -1 = none */
  npb_controls_t ctl; int ctl_axis[NPB_CONTROL_INPUT_COUNT];
  /* npb_set_control_orders: the rules, the controls' columns they read, the caller's fired and the handle's since (base ord.since);
   * dropped with the controls */
  npb_control_orders_t ord;
  /* npb_set_rollout: the caller's time-major buffers, the shapes they were bound with, the rows of final_obs every plant has taken (base
   * ro.n_final) and the cursor */
  npb_rollout_t ro;
  /* npb_rollout_moments: the partials' workspace (base mom.ws), grown on demand */
  npb_moments_ws_t mom;
  /* npb_set_policy: the shapes, the parameters on the device as the caller packed them and as the kernel reads them (base pol.theta), the
   * caller's descriptor, and the draw counter t */
  npb_policy_t pol; uint64_t pol_t;
  /* npb_set_policy_core: the GRU cell in front of both nets -- its six gate layers, the caller's hidden, first and final, and the restart
   * words primed and seen on the device (base core.primed; NULL = the policy has no core); dropped with the policy */
  npd_policy_core_t core;
  /* npb_policy_core_segments: the caller's stored segment states [seg_rows][n][H], a row every seg_every slots of the rollout (0 = off);
   * dropped with the policy */
  float *seg_starts; int seg_every, seg_rows;
  /* npb_policy_grad / npb_policy_adam: the gradient, the statistics, the optimiser's m, v and step (base ppo.stats) and the chains'
   * workspace (base ppo.chain_stats), allocated on first use, dropped with the policy */
  npb_ppo_t ppo;
  double *ramp_prev;   /* npb_profile_ramp: the previous setpoint of every plant ([pitch], NaN = none yet), allocated on first use */
  int *plan_dev;       /* npb_gather_fields: {column, sub, kind} per requested field, and the request it was built for */
  std::vector<int> plan_key;
  std::vector<Sampler *> samplers;   /* npb_sampler_create: by id; a destroyed one leaves a NULL entry */
  std::string error;
};

static thread_local std::string g_create_error;

static int fail(NpbHandle *h, int code, const char *what, hipError_t e = hipSuccess) {
  std::string msg = what;
  if (e != hipSuccess) { msg += ": "; msg += hipGetErrorString(e); }
  if (h) h->error = msg; else g_create_error = msg;
  return code;
}
/* every entry point that launches makes the handle's device current for the duration of the call and puts the
 * caller's device back afterwards: a process may hold handles on several GPUs, and a launch on whichever device
 * happened to be current would run against another device's arena.  hipGetDevice is a thread-local read;
 * hipSetDevice is paid only when the caller was elsewhere. */
struct DeviceGuard {
  int prev = -1; bool switched = false; hipError_t err = hipSuccess;
  explicit DeviceGuard(int device) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != device) { err = hipSetDevice(device); switched = err == hipSuccess; }
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
#define NPB_USE_DEVICE(h) DeviceGuard guard__((h)->device); if (guard__.err != hipSuccess) return fail(h, NPB_EHIP, "hipSetDevice", guard__.err)
#define NPB_HIP(h, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return fail(h, NPB_EHIP, #call, e__); } while (0)
static int fail_who(NpbHandle *h, const char *who, const char *what) { return fail(h, NPB_EINVAL, (std::string(who) + what).c_str()); }

/* ---- the lifecycle the per-step attachments share (column statistics, event windows, task, features, controls, rollout, normaliser).  Each keeps its tables
 * and per-plant bookkeeping in one device allocation, whose base is the struct's "is it on" pointer.  npb_set_* = attachment_alloc, fill
 * the struct from the base, attachment_drop the old one, assign; off and npb_destroy = attachment_drop; npb_*_clear = attachment_clear;
 * npb_*_get_state / npb_*_set_state = that attachment's StateParts through state_copy */

/* `bytes` on the device, zeroed, the host table (table_bytes of them, may be 0) uploaded to their start; synchronous, so the host table may
 * go.  Where HIP fails nothing is kept and the failure is reported as `who`'s, about `what`; `nomem`: the code of a refused hipMalloc */
static int attachment_alloc(NpbHandle *h, const char *who, const char *what, const void *table, size_t table_bytes, size_t bytes, char **dev,
                            int nomem = NPB_EHIP) {
  char text[200];
  hipError_t e = hipMalloc((void **)dev, bytes);
  if (e != hipSuccess) {
    snprintf(text, sizeof text, "%s: hipMalloc of %s (%zu bytes) failed", who, what, bytes);
    return fail(h, nomem, text, e);
  }
  e = hipMemset(*dev, 0, bytes);
  if (e == hipSuccess && table_bytes) e = hipMemcpy(*dev, table, table_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) return NPB_OK;
  (void)hipFree(*dev);
  snprintf(text, sizeof text, "%s: setting up %s failed", who, what);
  return fail(h, NPB_EHIP, text, e);
}
/* the attachment off: its allocation freed (hipFree waits for the device: a launch still in flight finishes first), its struct empty */
template <class T> static void attachment_drop(T *attachment, const void *base) {
  if (base) (void)hipFree((void *)base);
  *attachment = T{};
}
static const char *const g_no_event_windows = ": no event windows set (npb_set_event_windows first)";
static const char *const g_no_column_stats = ": no column statistics set (npb_set_column_stats first)";
static const char *const g_no_task = ": no task set (npb_set_task first)";
static const char *const g_no_features = ": no features set (npb_set_features first)";
static const char *const g_no_controls = ": no controls set (npb_set_controls first)";
static const char *const g_no_rollout = ": no rollout set (npb_set_rollout first)";
static const char *const g_no_normalizer = ": no normaliser set (npb_set_normalizer first)";
/* npb_set_features / npb_set_controls while a rollout is set, set and NULL alike: its pre kernel copies their tensors, in the shapes it was bound with */
/* the policy's training buffers go with the policy */
static void ppo_drop(NpbHandle *h) {
  if (h->ppo.chain_stats) (void)hipFree(h->ppo.chain_stats);
  if (h->ppo.hseq) (void)hipFree(h->ppo.hseq);
  attachment_drop(&h->ppo, h->ppo.stats);
}
static const char *const g_no_policy = ": no policy set (npb_set_policy first)";
/* npb_set_features / npb_set_controls / npb_set_rollout while a policy is set, set and NULL alike: it reads and writes their tensors */
static const char *const g_policy_holds = ": a policy is set (npb_set_policy) and reads or writes this attachment's tensors every step; npb_set_policy(h, NULL) first";
static const char *const g_rollout_holds = ": a rollout is set (npb_set_rollout) and records this tensor every step; npb_set_rollout(h, NULL) first";
/* the body of an npb_*_clear: refused with `off` unless the attachment is on, then its launch on the handle's device */
template <class Launch> static int attachment_clear(NpbHandle *h, const char *who, const void *on, const char *off, Launch launch) {
  if (!on) return fail_who(h, who, off);
  NPB_USE_DEVICE(h);
  launch();
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
/* an attachment's checkpointed state: whether it is on (else refused with `off`), and its parts on the device in the order its get_state /
 * set_state take them, stated once for both directions; a part that may be absent is one the caller may pass NULL for (`null_note` says
 * which) */
struct StatePart { void *dev; size_t bytes; bool may_be_absent; };
struct StateParts { const void *on; const char *off, *null_note; int count; StatePart part[7]; };
static int state_copy(NpbHandle *h, const char *who, StateParts (*parts_of)(const NpbHandle *), std::initializer_list<const void *> host,
                      bool to_device, void *stream) {
  if (!h) return NPB_EINVAL;
  const StateParts S = parts_of(h);
  if (!S.on) return fail_who(h, who, S.off);
  for (int k = 0; k < S.count; k++)
    if (!host.begin()[k] && !S.part[k].may_be_absent)
      return fail_who(h, who, (std::string(to_device ? ": NULL input" : ": NULL output") + S.null_note).c_str());
  NPB_USE_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  for (int k = 0; k < S.count; k++) {
    const StatePart &P = S.part[k];
    void *mine = (void *)host.begin()[k];
    if (!P.bytes) continue;
    NPB_HIP(h, to_device ? hipMemcpyAsync(P.dev, mine, P.bytes, hipMemcpyHostToDevice, st) : hipMemcpyAsync(mine, P.dev, P.bytes, hipMemcpyDeviceToHost, st));
  }
  NPB_HIP(h, hipStreamSynchronize(st));      /* the host arrays may go */
  return NPB_OK;
}

/* where the members of the schema live in the arena (include/npb_fields.h: carried fp64 members one per column,
 * then the narrow members -- outputs as float, int32 -- two per 8-byte column or one per 4-byte column) */
struct SectionInfo { int f64_base, nf64, nout, i32_base, ni32, count, col64_base, ncol64, col32_base, ncol32; };
static const SectionInfo g_sections[] = {
#define NPB__INFO(member, T, stype, count) \
  {NPB_##T##_F64_BASE, NPB_##T##_NF64, NPB_##T##_NOUT, NPB_##T##_I32_BASE, NPB_##T##_NI32, (count), \
   NPB_##T##_COL64_BASE, NPB_##T##_NCOL64, NPB_##T##_COL32_BASE, NPB_##T##_NCOL32},
  NPB_SECTIONS(NPB__INFO)
#undef NPB__INFO
};
/* kind: NPB_KIND_F64 / NPB_KIND_I32 and the global slot -> arena column, narrow position, access kind of the field kernels */
static bool locate(int storage, int kind, int slot, int *col, int *sub, int *akind) {
  const int npc = storage == NPB_STORAGE_F32 ? 1 : 2;
  for (const SectionInfo &s : g_sections) {
    const int base = kind == NPB_KIND_F64 ? s.f64_base : s.i32_base, per = kind == NPB_KIND_F64 ? s.nf64 : s.ni32;
    if (per == 0 || slot < base || slot >= base + per * s.count) continue;
    const int inst = (slot - base) / per, k = (slot - base) % per, ncarry = s.nf64 - s.nout;
    const int col0 = (storage == NPB_STORAGE_F32 ? s.col32_base + inst * s.ncol32 : s.col64_base + inst * s.ncol64);
    if (kind == NPB_KIND_F64 && k < ncarry) { *col = col0 + k; *sub = 0; *akind = 0; return true; }
    const int j = kind == NPB_KIND_F64 ? k - ncarry : s.nout + k;
    *col = col0 + ncarry + j / npc; *sub = j % npc; *akind = kind == NPB_KIND_F64 ? 1 : 2;
    return true;
  }
  return false;
}
static size_t arena_columns(int storage) { return storage == NPB_STORAGE_F32 ? (size_t)NPB_TOTAL_COL32 : (size_t)NPB_TOTAL_COL64; }
/* plants the arena has room for: whole segments when it is segmented */
static size_t arena_plants(const NpbHandle *h) { return h->seg ? (h->pitch + h->seg - 1) / h->seg * h->seg : h->pitch; }
/* what the launchers take as the column pitch: the pitch with the segment size in the upper half (npb_kernels.hip, NPD_SEGMENT) */
#define NPB_N(h) ((size_t)(h)->pitch | ((size_t)(h)->seg << 32))
/* where a restore copies from: the start bank with its slots (bank), or else the snapshot, which has no slot or start columns */
static npb_source_t source_of(const NpbHandle *h, bool bank) {
  npb_source_t S = {};
  if (!bank) { S.arena = h->snap; S.N = NPB_N(h); return S; }
  S.arena = h->bank; S.N = h->bank_N; S.M = h->bank_M;
  S.next_slot = h->next_slot; S.episode_start = h->slot_start; S.advance = h->slot_advance; S.start = h->ep_start; S.out_start = h->ep_out_start;
  return S;
}
static double *cm_state(const NpbHandle *h) { return (double *)((char *)h->cm_side + npb_launch_cmaint_state_offset()); }

/* ---- side blocks: per-plant fp64 rows that belong to a plant's state and live beside the arena (npb_kernels.h).  Every episode path takes
 * them along through this one table: npb_snapshot and npb_set_start_bank record them, npb_restore, npb_restore_bank and the autoreset of
 * npb_step put them back.  A further block is an entry here and its copy loop in npd_restore_lanes (npb_kernels.hip). */
struct SideBlock {
  int rows;                                           /* per plant */
  bool (*on)(const NpbHandle *h);
  hipError_t (*pack)(const NpbHandle *h, double *packed, hipStream_t stream);   /* h's live rows into a packed [rows][h->pitch] copy */
  npb_side_restore_t (*live)(const NpbHandle *h);     /* where a restore puts them: the live rows and their pitch */
  const char *no_snapshot, *no_bank;                  /* the block is on and the snapshot / the bank was recorded without it */
  const char *bank_lacks;                             /* npb_set_start_bank: this handle has it and the bank handle has not */
  const char *snapshot_nomem, *bank_nomem;            /* hipMalloc of the copy failed */
};
static const SideBlock g_side[NPB_SIDE_COUNT] = {
  /* NPB_SIDE_CMAINT: the generators' and the condenser's stamps and open orders belong to the episode start as the mpump section does */
  { NPB_CMAINT_SIDE_DOUBLES,
    [](const NpbHandle *h) { return h->cm_on; },
    [](const NpbHandle *h, double *packed, hipStream_t stream) {
      return hipMemcpyAsync(packed, cm_state(h), (size_t)NPB_CMAINT_SIDE_DOUBLES * h->pitch * sizeof(double), hipMemcpyDeviceToDevice, stream); },
    [](const NpbHandle *h) { return npb_side_restore_t{cm_state(h), nullptr, h->pitch, 0}; },
    "the component maintenance is on (npb_set_component_maintenance) and the snapshot was taken without it: npb_snapshot again",
    "the component maintenance is on (npb_set_component_maintenance) and the start bank was set without it: npb_set_start_bank again, from a handle that has it",
    "npb_set_start_bank: this handle has the component maintenance on (npb_set_component_maintenance) and the bank handle has not",
    "npb_snapshot: hipMalloc of the component maintenance's snapshot failed",
    "npb_set_start_bank: hipMalloc of the bank's component maintenance state failed" },
  /* NPB_SIDE_DIAG: the carried rows of the caller's diagnostics buffer (accumulators, latches, ejector values), packed in table order */
  { NPB_DIAG_NUM_CARRIED,
    [](const NpbHandle *h) { return h->diag_carry; },
    [](const NpbHandle *h, double *packed, hipStream_t stream) {
      npb_launch_diag_carried_pack(h->diag, h->diag_pitch, packed, h->pitch, h->pitch, stream);
      return hipGetLastError(); },
    [](const NpbHandle *h) { return npb_side_restore_t{h->diag, nullptr, h->diag_pitch, 0}; },
    "the diagnostics rows are carried (npb_carry_diagnostics) and the snapshot was taken without them: npb_snapshot again",
    "the diagnostics rows are carried (npb_carry_diagnostics) and the start bank was set without them: npb_set_start_bank again, from a handle that carries them",
    "npb_set_start_bank: this handle carries the diagnostics rows (npb_carry_diagnostics) and the bank handle does not",
    "npb_snapshot: hipMalloc of the carried diagnostics rows' snapshot failed",
    "npb_set_start_bank: hipMalloc of the bank's carried diagnostics rows failed" },
};
static void side_free(SideCopy *c) {
  if (c->rows) (void)hipFree(c->rows);
  *c = SideCopy{};
}
/* npb_snapshot (src = h, bank false) / npb_set_start_bank: block b of src into h's snapshot or bank copy, in src's pitch.  A source that
 * has the block off leaves no copy: an older one does not belong to this snapshot or bank */
static int side_record(NpbHandle *h, int b, bool bank, const NpbHandle *src, hipStream_t stream) {
  const SideBlock &B = g_side[b];
  SideCopy *c = bank ? &h->side[b].bank : &h->side[b].snap;
  if (!B.on(src)) {
    if (c->rows) { NPB_HIP(h, hipStreamSynchronize(stream)); side_free(c); }
    return NPB_OK;
  }
  const size_t doubles = (size_t)B.rows * src->pitch;
  if (doubles > c->doubles) {
    side_free(c);
    hipError_t e = hipMalloc((void **)&c->rows, doubles * sizeof(double));
    if (e != hipSuccess) { c->rows = nullptr; return fail(h, NPB_EHIP, bank ? B.bank_nomem : B.snapshot_nomem, e); }
    c->doubles = doubles;
  }
  NPB_HIP(h, B.pack(src, c->rows, stream));
  c->pitch = src->pitch;
  return NPB_OK;
}
/* what a restore from the snapshot or the bank takes along beside the arena.  Returns the first block, in table order or with the last
 * block first, that is on while the source was recorded without it (side_refusal has the message), or -1 */
static int side_restores_of(const NpbHandle *h, bool bank, bool last_first, npb_side_restores_t *out) {
  *out = npb_side_restores_t{};
  for (int i = 0; i < NPB_SIDE_COUNT; i++) {
    const int b = last_first ? NPB_SIDE_COUNT - 1 - i : i;
    if (!g_side[b].on(h)) continue;
    const SideCopy &c = bank ? h->side[b].bank : h->side[b].snap;
    if (!c.rows) return b;
    out->block[b] = g_side[b].live(h);
    out->block[b].src = c.rows; out->block[b].src_pitch = c.pitch;
  }
  return -1;
}
static const char *side_refusal(int b, bool bank) { return bank ? g_side[b].no_bank : g_side[b].no_snapshot; }
/* npb_reset / npb_reset_reference (counters) and npb_restore: the episode counters (with counters) and the carried start entries of the
 * plants of mask (NULL = every lane of the pitch) to 0 and -1 */
static void clear_episodes(NpbHandle *h, const uint8_t *mask, bool counters, hipStream_t stream) {
  int32_t *len = counters ? h->ep_len : nullptr;
  if (len || h->ep_start) npb_launch_episode_clear(mask, len, counters ? h->ep_ret : nullptr, h->ep_index, h->ep_start, h->n_plants, h->pitch, stream);
}
/* npb_reset, npb_reset_reference, npb_restore, npb_restore_bank: a recurrent policy's hidden state restarts with the plants of mask -- they
 * are unprimed, and the policy's next launch reads +0.0 for them (npb_policy_core.hip) */
static void core_restart(NpbHandle *h, const uint8_t *mask, hipStream_t stream) {
  if (h->core.primed) npb_launch_unprime(h->core.primed, mask, h->n_plants, stream);
}
static npb_episode_counters_t counters_of(const NpbHandle *h) { return npb_episode_counters_t{h->ep_len, h->ep_ret, h->ep_index, h->ep_out_index}; }
/* episode streams: the plants whose episode index the call before has bumped begin their streams anew, behind that call's kernels.
 * from_bank: the restart took bank entries, which the carried start column names */
static void restart_streams(NpbHandle *h, bool from_bank, hipStream_t stream, const npb_episode_streams_take_t *take = nullptr) {
  if (h->es_on) npb_launch_episode_streams_restart(&h->es, h->es_noise_cur, h->es_prof_cur, from_bank ? h->ep_start : nullptr, 0, take, stream);
}
static const char *const g_es_owns = ": episode streams are on (npb_set_episode_streams) and the handle owns the streams' consumption; switch the mode off first";
static const struct { int row; double fresh; } g_diag_carried[] = {
#define NPB__X(row, fresh) {row, fresh},
  NPB_DIAG_CARRIED(NPB__X)
#undef NPB__X
};
static_assert(sizeof(g_diag_carried) / sizeof(g_diag_carried[0]) == NPB_DIAG_NUM_CARRIED, "carried diagnostics rows");
/* what NuclearPlantSimulator.reset() leaves in the carried rows, in table order (tools/make_diag_reset_golden.py read them off the live
 * reference: tests/golden/diag_carry/reference_reset.json); NaN = the row is kept */
static npb_diag_carried_values_t diag_reference_reset_values();

/* Where an arena lands in physical memory changes the step kernel's time when the bytes a step touches are about the
 * size of the 256 MB Infinity Cache (65 536 fp64 plants: 276 MB): handles created one after another in one process run
 * at 0.097 ms or at 0.110 ms per step, reproducibly per handle for its whole life, and nothing cheaper than the step
 * kernel itself predicts which (tools/launch_series.py).  So in that zone npb_create allocates up to
 * four candidate arenas, times a dozen launches of the step kernel on each (construction state, no inputs, no
 * outputs), keeps the fastest and frees the rest; the kept arena is initialised again by the caller below.  About 15 ms,
 * once per handle.  NPB_PLACEMENT_PROBE=0 turns it off. */
static void probe_placement(NpbHandle *h, size_t step_columns) {
  const char *env = getenv("NPB_PLACEMENT_PROBE");
  if (env && atoi(env) == 0) return;
  const double touched_mb = (double)step_columns * h->real_bytes * h->pitch / 1.0e6;
  if (touched_mb < 200.0 || touched_mb > 340.0 || h->params.mode == NPB_MODE_PRIMARY) return;
  const size_t bytes = arena_columns(h->storage) * arena_plants(h) * h->real_bytes;
  const int max_candidates = 4, launches = 12;
  void *cand[max_candidates] = {h->f64, nullptr, nullptr, nullptr};
  float ms[max_candidates] = {0, 0, 0, 0};
  hipEvent_t a, b;
  if (hipEventCreate(&a) != hipSuccess) return;
  if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return; }
  /* the clocks first: after an idle period the step kernel needs ~170 launches to reach its steady time (bench.py,
   * "preconditioning"), and the first candidate would otherwise be timed on the ramp -- a 5-7 % bias against it, half of
   * the effect being selected on.  Untimed launches on candidate 0 until ~20 ms have passed. */
  const auto step = [h](void *arena) {      /* no inputs, no outputs, no diagnostics, no maintenance */
    (void)h->K->step(&h->params, h->n_plants, NPB_N(h), arena, nullptr, nullptr, nullptr, nullptr, nullptr,
                     nullptr, nullptr, nullptr, nullptr, nullptr, h->step_kernel, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
  };
  h->K->init(&h->params, h->n_plants, NPB_N(h), cand[0], nullptr, nullptr);
  for (int k = 0; k < 200; k++) step(cand[0]);
  if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); (void)hipEventDestroy(a); (void)hipEventDestroy(b); return; }
  int n = 0;
  for (; n < max_candidates; n++) {
    if (n > 0 && hipMalloc(&cand[n], bytes) != hipSuccess) { cand[n] = nullptr; (void)hipGetLastError(); break; }
    h->K->init(&h->params, h->n_plants, NPB_N(h), cand[n], nullptr, nullptr);
    float best = 1e30f;
    for (int k = 0; k < launches; k++) {
      (void)hipEventRecord(a, nullptr);
      step(cand[n]);
      (void)hipEventRecord(b, nullptr);
      if (hipEventSynchronize(b) != hipSuccess) { best = 1e30f; break; }
      float t = 0;
      if (hipEventElapsedTime(&t, a, b) != hipSuccess) { best = 1e30f; break; }
      if (k >= 4 && t < best) best = t;     /* the first launches warm the caches */
    }
    ms[n] = best;
  }
  /* nothing of a candidate may still be in flight when it is freed (an event wait that failed above leaves that unknown) */
  (void)hipDeviceSynchronize();
  int keep = 0;
  for (int i = 1; i < n; i++) if (ms[i] < ms[keep]) keep = i;
  for (int i = 0; i < n; i++) if (i != keep && cand[i]) (void)hipFree(cand[i]);
  h->f64 = cand[keep];
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
}

/* ---- a per-plant column: THE host-side definition for the column statistics, the event windows and the task (and whoever reads a column
 * next): one view of the descriptor's three spellings, one refusal, one translation into what npd_column_read reads (npb_kernels.hip) */
struct column_view { int kind, slot; const npb_sample_source_t *source; };      /* the arena member (kind, slot), or source != NULL: the caller's side source */
static column_view column_of(int kind, int slot) { return column_view{kind, slot, nullptr}; }
static column_view column_of(const npb_sample_source_t &S) { return column_view{0, 0, &S}; }
/* the {from_source, kind, slot, source} head that npb_event_trigger_t and npb_task_column_t share */
template <class Head> static column_view column_of(const Head &C) { return C.from_source ? column_of(C.source) : column_of(C.kind, C.slot); }
/* column c of a descriptor that lists kinds[] / slots[] and then sources[] (npb_column_stats_desc_t, npb_event_windows_desc_t) */
template <class Desc> static column_view column_of(const Desc *D, int c) {
  return c < D->n_fields ? column_of(D->kinds[c], D->slots[c]) : column_of(D->sources[c - D->n_fields]);
}
/* the five refusals under an entry point's own prefix: static strings, since the *_check functions hand them out without a handle */
enum { COLUMN_BAD_FIELD, COLUMN_NULL_BASE, COLUMN_BAD_TYPE, COLUMN_ROWS, COLUMN_STRIDE, COLUMN_REFUSALS_COUNT };
#define COLUMN_REFUSALS(who) { who ": bad field kind or slot", who ": a side source has a NULL base", who ": a side source has an unknown element type", \
                               who ": a side source must have rows == 1 (one value per plant)", who ": a side source needs a plant stride >= 0" }
static const char *const g_cs_column[COLUMN_REFUSALS_COUNT] = COLUMN_REFUSALS("npb_set_column_stats");
static const char *const g_ew_column[COLUMN_REFUSALS_COUNT] = COLUMN_REFUSALS("npb_set_event_windows");
static const char *const g_task_column[COLUMN_REFUSALS_COUNT] = COLUMN_REFUSALS("npb_set_task");
static const char *const g_feat_column[COLUMN_REFUSALS_COUNT] = COLUMN_REFUSALS("npb_set_features");
/* why a column is refused (who: the caller's table above), or NULL; integer (may be NULL): whether its values are integers, which bit masks need */
static const char *column_refusal(const char *const *who, column_view C, bool *integer) {
  bool is_integer;
  if (C.source) {
    const npb_sample_source_t &S = *C.source;
    if (!S.base) return who[COLUMN_NULL_BASE];
    if (S.type < NPB_SAMPLE_F64 || S.type > NPB_SAMPLE_U8) return who[COLUMN_BAD_TYPE];
    if (S.rows != 1) return who[COLUMN_ROWS];
    if (S.plant_stride < 0) return who[COLUMN_STRIDE];
    is_integer = S.type == NPB_SAMPLE_I32 || S.type == NPB_SAMPLE_U8;
  } else {
    int col, sub, access;
    if ((C.kind != NPB_KIND_F64 && C.kind != NPB_KIND_I32) || !locate(NPB_STORAGE_F64, C.kind, C.slot, &col, &sub, &access)) return who[COLUMN_BAD_FIELD];
    is_integer = C.kind == NPB_KIND_I32;
  }
  if (integer) *integer = is_integer;
  return nullptr;
}
/* the column as the kernels read it, under the handle's storage type (direction / limit stay the caller's); false: no such member */
static bool column_build(const NpbHandle *h, column_view C, npb_colstat_col_t *O) {
  if (C.source) { O->row = C.source->base; O->plant_stride = C.source->plant_stride; O->kind = 3 + C.source->type; return true; }
  return locate(h->storage, C.kind, C.slot, &O->col, &O->sub, &O->kind);
}
/* the eight statistics tables of npb_column_stats_desc_t and npb_episode_record_stats_desc_t: doubles 8-byte, int32 4-byte aligned */
template <class Tables> static bool stat_tables_misaligned(const Tables *D) {
  return ((uintptr_t)D->min & 7u) || ((uintptr_t)D->max & 7u) || ((uintptr_t)D->sum & 7u) || ((uintptr_t)D->sumsq & 7u) || ((uintptr_t)D->last & 7u) ||
         ((uintptr_t)D->first_beyond & 7u) || ((uintptr_t)D->n_beyond & 3u) || ((uintptr_t)D->n_samples & 3u);
}

extern "C" {

int npb_version(void) { return NPB_VERSION; }
int npb_num_f64(void) { return NPB_TOTAL_F64; }
int npb_num_i32(void) { return NPB_TOTAL_I32; }
int npb_obs_dim(void) { return NPB_OBS_DIM; }
int npb_info_dim(void) { return NPB_INFO_DIM; }
int npb_info_nrho(void) { return NPB_INFO_NRHO; }
int npb_diag_dim(void) { return NPB_DIAG_DIM; }
int npb_diag_num_carried(void) { return NPB_DIAG_NUM_CARRIED; }
int npb_diag_carried_row(int k) { return k >= 0 && k < NPB_DIAG_NUM_CARRIED ? g_diag_carried[k].row : -1; }
double npb_diag_carried_fresh(int k) { return k >= 0 && k < NPB_DIAG_NUM_CARRIED ? g_diag_carried[k].fresh : __builtin_nan(""); }
static const char *const g_maint_params[] = {
#define NPB__X(id, name) name,
  NPB_MAINT_PARAMS(NPB__X)
#undef NPB__X
};
static const struct { const char *name; int handler; } g_maint_actions[] = {
#define NPB__X(id, name, handler) {name, handler},
  NPB_MAINT_ACTIONS(NPB__X)
#undef NPB__X
};
int npb_maint_num_params(void) { return NPB_MAINT_NPARAM; }
int npb_maint_num_actions(void) { return NPB_MAINT_NACT; }
const char *npb_maint_param_name(int k) { return k >= 0 && k < NPB_MAINT_NPARAM ? g_maint_params[k] : nullptr; }
const char *npb_maint_action_name(int a) { return a >= 0 && a < NPB_MAINT_NACT ? g_maint_actions[a].name : nullptr; }
int npb_maint_action_has_handler(int a) { return a >= 0 && a < NPB_MAINT_NACT ? g_maint_actions[a].handler : 0; }
static_assert(sizeof(g_maint_params) / sizeof(g_maint_params[0]) == NPB_MAINT_NPARAM, "parameter catalog");
static_assert(sizeof(g_maint_actions) / sizeof(g_maint_actions[0]) == NPB_MAINT_NACT, "action catalog");
static const struct { const char *name; int kind; } g_component_actions[] = {
#define NPB__X(kind, id, name) {name, NPB_COMPONENT_##kind},
  NPB_COMPONENT_ACTIONS(NPB__X)
#undef NPB__X
};
static const char *const g_component_kinds[] = {"steam_generator", "steam_generator_system", "condenser", "ejector"};
static_assert(sizeof(g_component_actions) / sizeof(g_component_actions[0]) == NPB_COMPONENT_NACT, "component catalog");
static_assert(sizeof(g_component_kinds) / sizeof(g_component_kinds[0]) == NPB_COMPONENT_NKIND, "component kinds");
int npb_component_num_actions(void) { return NPB_COMPONENT_NACT; }
const char *npb_component_action_name(int a) { return a >= 0 && a < NPB_COMPONENT_NACT ? g_component_actions[a].name : nullptr; }
int npb_component_action_kind(int a) { return a >= 0 && a < NPB_COMPONENT_NACT ? g_component_actions[a].kind : -1; }
const char *npb_component_kind_name(int kind) { return kind >= 0 && kind < NPB_COMPONENT_NKIND ? g_component_kinds[kind] : nullptr; }
static const struct { const char *name; int kind; } g_turbine_actions[] = {
#define NPB__X(kind, id, name) {name, NPB_TURBINE_##kind},
  NPB_TURBINE_ACTIONS(NPB__X)
#undef NPB__X
};
static const char *const g_turbine_kinds[] = {"turbine", "bearing", "lubrication", "stage"};
static_assert(sizeof(g_turbine_actions) / sizeof(g_turbine_actions[0]) == NPB_TURBINE_NACT, "turbine catalog");
static_assert(sizeof(g_turbine_kinds) / sizeof(g_turbine_kinds[0]) == NPB_TURBINE_NKIND, "turbine kinds");
int npb_turbine_num_actions(void) { return NPB_TURBINE_NACT; }
const char *npb_turbine_action_name(int a) { return a >= 0 && a < NPB_TURBINE_NACT ? g_turbine_actions[a].name : nullptr; }
int npb_turbine_action_kind(int a) { return a >= 0 && a < NPB_TURBINE_NACT ? g_turbine_actions[a].kind : -1; }
const char *npb_turbine_kind_name(int kind) { return kind >= 0 && kind < NPB_TURBINE_NKIND ? g_turbine_kinds[kind] : nullptr; }
size_t npb_state_bytes(void) { return (size_t)NPB_TOTAL_COL64 * 8; }
/* carried fp64 members are read and written, int32 members too, output members are only written (as float);
 * the maint.* section belongs to the maintenance kernel */
static size_t step_bytes(size_t real_bytes, bool kinetics = true) {
  size_t carried = 0, outputs = 0, ints = 0;
  for (const SectionInfo &s : g_sections) {
    if (s.f64_base == NPB_MAINT_F64_BASE || s.f64_base == NPB_MPUMP_F64_BASE) continue;
    carried += (size_t)(s.nf64 - s.nout) * s.count; outputs += (size_t)s.nout * s.count; ints += (size_t)s.ni32 * s.count;
  }
  if (!kinetics) carried -= NPB_PRIM_NKIN; /* ConstantHeatSource: the point-kinetics columns are not touched */
  return 2 * carried * real_bytes + 2 * ints * 4 + outputs * 4 + (4 + 4 * 8) + (NPB_OBS_DIM * 8 + 8 + 1 + 4 + NPB_INFO_DIM * 8);
}
size_t npb_step_bytes_per_plant(void) { return step_bytes(8); }
size_t npb_handle_step_bytes_per_plant(const NpbHandle *h) {
  return step_bytes(h && h->storage == NPB_STORAGE_F32 ? 4 : 8, !h || h->params.heat_source == NPB_HEAT_REACTOR);
}
void npb_default_params(npb_params_t *p) { npb_params_default(p); }

const char *npb_last_error(const NpbHandle *h) { return h ? h->error.c_str() : g_create_error.c_str(); }
int npb_num_plants(const NpbHandle *h) { return h ? h->n_plants : 0; }

int npb_create(const npb_params_t *params, int n_plants, int device, NpbHandle **out) {
  return npb_create_storage(params, n_plants, device, NPB_STORAGE_F64, out);
}

int npb_storage(const NpbHandle *h) { return h ? h->storage : -1; }

int npb_create_storage(const npb_params_t *params, int n_plants, int device, int storage, NpbHandle **out) {
  if (!out || n_plants <= 0) return fail(nullptr, NPB_EINVAL, "npb_create: bad arguments");
  *out = nullptr;
  if (storage != NPB_STORAGE_F64 && storage != NPB_STORAGE_F32) return fail(nullptr, NPB_EINVAL, "npb_create: storage must be NPB_STORAGE_F64 or NPB_STORAGE_F32");
  const size_t real_bytes = storage == NPB_STORAGE_F32 ? sizeof(float) : sizeof(double);
  /* the step kernel addresses a column as (one 64-bit base) + (32-bit byte offset), nuclear_sim_amd/csrc/npd_stage.h;
   * the maintenance sections behind its columns are addressed with 64-bit arithmetic by their own kernel */
  const size_t step_columns = storage == NPB_STORAGE_F32 ? (size_t)NPB_MPUMP_COL32_BASE : (size_t)NPB_MPUMP_COL64_BASE;
  if ((((size_t)n_plants + 63) / 64 * 64) * step_columns * real_bytes >= ((size_t)1 << 32))
    return fail(nullptr, NPB_EINVAL, "npb_create: more than 4 GiB of real-valued state per handle (about one million fp64 plants); use several handles");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) return fail(nullptr, NPB_EHIP, "npb_create: no HIP device", e);
  if (device < 0 || device >= ndev) return fail(nullptr, NPB_EINVAL, "npb_create: device index out of range");
  int caller_device = -1;
  (void)hipGetDevice(&caller_device);
  NPB_HIP(nullptr, hipSetDevice(device));
  NpbHandle *h = new NpbHandle();
  if (params) h->params = *params; else npb_params_default(&h->params);
  npb_maint_table_default(&h->maint_table);
  h->maint_table_custom = false;
  { const char *e = getenv("NPB_STEP_KERNEL"); h->step_kernel = e ? atoi(e) : 0; if (h->step_kernel < 0 || h->step_kernel > 5) h->step_kernel = 0; }
  h->n_plants = n_plants; h->device = device;
  h->pitch = ((size_t)n_plants + 63) / 64 * 64;
  h->storage = storage; h->real_bytes = real_bytes;
  h->K = storage == NPB_STORAGE_F32 ? &npb32_launch_table : &npb_launch_table;
  h->A = storage == NPB_STORAGE_F32 ? &npb32_launch_attach_table : &npb_launch_attach_table;
  h->f64 = nullptr; h->convert = nullptr; h->plan_dev = nullptr;
  /* batches past the two-wave kernel's range keep their arena in segments of 16 384 plants (npd_arena.h, "segmented arena") */
  {   /* NPB_ARENA_SEGMENT=0 turns it off, =<plants> (a multiple of 64) forces that segment size at any batch size: A/B aids */
    const char *e2 = getenv("NPB_ARENA_SEGMENT");
    h->seg = h->pitch > 45056 ? 16384 : 0;     /* from NPB_SEGMENTED_FROM of npb_kernels.hip on: the four-wave kernel's second range and everything above it */
    if (e2) { const long v = atol(e2); h->seg = (v > 0 && v % 64 == 0 && (size_t)v < h->pitch) ? (size_t)v : 0; }
  }
  e = hipMalloc(&h->f64, arena_columns(storage) * arena_plants(h) * real_bytes);
  if (e == hipSuccess) probe_placement(h, step_columns);
  if (e == hipSuccess) e = hipMalloc((void **)&h->convert, h->pitch * sizeof(double) + npb_launch_maint_side_bytes(h->pitch));
  if (e != hipSuccess) {
    if (h->f64) (void)hipFree(h->f64);
    delete h;
    if (caller_device >= 0) (void)hipSetDevice(caller_device);
    return fail(nullptr, NPB_ENOMEM, "npb_create: hipMalloc of the state arena failed", e);
  }
  h->maint_side = (void *)(h->convert + h->pitch);
  h->maint_cache_stale = true;
  h->K->init(&h->params, n_plants, NPB_N(h), h->f64, nullptr, nullptr);
  e = hipDeviceSynchronize();
  if (caller_device >= 0 && caller_device != device) (void)hipSetDevice(caller_device); /* the caller's current device is left as it was */
  if (e != hipSuccess) {
    (void)hipSetDevice(device);
    (void)hipFree(h->f64); if (h->convert) (void)hipFree(h->convert);
    if (caller_device >= 0) (void)hipSetDevice(caller_device);
    delete h; return fail(nullptr, NPB_EHIP, "npb_create: init kernel failed", e);
  }
  *out = h;
  return NPB_OK;
}

int npb_destroy(NpbHandle *h) {
  if (!h) return NPB_OK;
  DeviceGuard guard__(h->device);
  (void)hipFree(h->f64);
  if (h->convert) (void)hipFree(h->convert);
  if (h->plan_dev) (void)hipFree(h->plan_dev);
  if (h->snap) (void)hipFree(h->snap);
  if (h->cm_side) (void)hipFree(h->cm_side);
  if (h->summary_ticket) (void)hipFree(h->summary_ticket);
  for (auto &sd : h->side) { side_free(&sd.snap); side_free(&sd.bank); }
  if (h->ep_len) (void)hipFree(h->ep_len);
  if (h->bank) (void)hipFree(h->bank);
  if (h->ep_start) (void)hipFree(h->ep_start);
  if (h->noise) (void)hipFree(h->noise);
  if (h->prof) (void)hipFree(h->prof);
  if (h->prof_side) (void)hipFree(h->prof_side);
  if (h->prof_z) (void)hipFree(h->prof_z);
  if (h->ramp_prev) (void)hipFree(h->ramp_prev);
  if (h->es_mem) (void)hipFree(h->es_mem);
  if (h->ers_dev) (void)hipFree(h->ers_dev);
  attachment_drop(&h->cs, h->cs.cols); attachment_drop(&h->ew, h->ew.cols); attachment_drop(&h->task, h->task.terms);
  attachment_drop(&h->feat, h->feat.cols); attachment_drop(&h->ord, h->ord.since); attachment_drop(&h->ctl, h->ctl.age); attachment_drop(&h->ro, h->ro.n_final);
  attachment_drop(&h->mom, h->mom.ws); attachment_drop(&h->norm, h->norm.streams);
  ppo_drop(h);
  attachment_drop(&h->core, h->core.primed);
  attachment_drop(&h->pol, h->pol.theta);
  for (Sampler *sm : h->samplers) if (sm) { (void)hipFree(sm->dev); delete sm; }
  delete h;
  return NPB_OK;
}

int npb_set_params(NpbHandle *h, const npb_params_t *params) {
  if (!h || !params) return NPB_EINVAL;
  h->params = *params;
  h->maint_cache_stale = true;
  return NPB_OK;
}

int npb_set_step_kernel(NpbHandle *h, int variant) {
  if (!h || variant < 0 || variant > 5) return NPB_EINVAL;
  h->step_kernel = variant;
  return NPB_OK;
}

int npb_debug_last_step_kernel(const NpbHandle *h) { return h ? h->last_kernel : NPB_KERNEL_NONE; }
const char *npb_step_kernel_name(int id) {
  static const char *const names[NPB_KERNEL_COUNT_] = {"", "npb_step_kernel", "npb_step2_wide_kernel", "npb_step2_kernel", "npb_step_nt_kernel",
                                                       "npb_step_diag_kernel", "npb_step_primary_kernel", "npb_step_maint_kernel", "npb_step2_wide_maint_kernel",
                                                       "npb_step2_maint_kernel", "npb_step_nt_maint_kernel", "npb_step4_kernel", "npb_step4_maint_kernel"};
  return id >= 0 && id < NPB_KERNEL_COUNT_ ? names[id] : nullptr;
}

int npb_set_diagnostics(NpbHandle *h, double *buf, size_t pitch) {
  if (!h) return NPB_EINVAL;
  if (buf && h->params.mode != NPB_MODE_FULL) return fail(h, NPB_EINVAL, "npb_set_diagnostics: full mode only");
  if (buf && pitch < h->pitch) return fail(h, NPB_EINVAL, "npb_set_diagnostics: pitch must be at least n_plants rounded up to 64");
  if (buf && h->autoreset)      /* the buffer carries plant state outside the arena, which a restore from the snapshot would not put back */
    return fail(h, NPB_EINVAL, "npb_set_diagnostics: autoreset is on (npb_set_autoreset); the diagnostics buffer carries plant state the snapshot does not hold");
  if (h->diag_carry) {      /* the buffer is the live copy of plant state the handle takes along */
    if (!buf && h->autoreset)
      return fail(h, NPB_EINVAL, "npb_set_diagnostics: autoreset is on (npb_set_autoreset) and restores the carried diagnostics rows (npb_carry_diagnostics) "
                                 "into this buffer: switch the autoreset off first");
    if (buf && (buf != h->diag || pitch != h->diag_pitch))
      return fail(h, NPB_EINVAL, "npb_set_diagnostics: the diagnostics rows are carried (npb_carry_diagnostics) in the buffer set before; "
                                 "npb_carry_diagnostics(h, 0) first, then move them with npb_get / npb_set_diagnostics_state");
    if (!buf) h->diag_carry = false;
  }
  h->diag = buf; h->diag_pitch = buf ? pitch : 0;
  return NPB_OK;
}

int npb_carry_diagnostics(NpbHandle *h, int on) {
  if (!h) return NPB_EINVAL;
  if (!on) {
    if (h->diag_carry && h->autoreset)
      return fail(h, NPB_EINVAL, "npb_carry_diagnostics: autoreset is on (npb_set_autoreset) with diagnostics, which it restores only while their rows "
                                 "are carried: switch the autoreset off first");
    h->diag_carry = false;
    return NPB_OK;
  }
  if (!h->diag)
    return fail(h, NPB_EINVAL, "npb_carry_diagnostics: no diagnostics buffer (npb_set_diagnostics first; full mode only): its carried rows are what is carried");
  h->diag_carry = true;
  return NPB_OK;
}
int npb_get_diagnostics_state(NpbHandle *h, double *buf, void *stream) {
  if (!h || !buf) return NPB_EINVAL;
  if (!h->diag_carry) return fail(h, NPB_EINVAL, "npb_get_diagnostics_state: the diagnostics rows are not carried (npb_carry_diagnostics first)");
  NPB_USE_DEVICE(h);
  for (int k = 0; k < NPB_DIAG_NUM_CARRIED; k++)
    NPB_HIP(h, hipMemcpyAsync(buf + (size_t)k * h->n_plants, h->diag + (size_t)g_diag_carried[k].row * h->diag_pitch, (size_t)h->n_plants * sizeof(double),
                              hipMemcpyDefault, (hipStream_t)stream));
  NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream));
  return NPB_OK;
}
int npb_set_diagnostics_state(NpbHandle *h, const double *buf, void *stream) {
  if (!h || !buf) return NPB_EINVAL;
  if (!h->diag_carry) return fail(h, NPB_EINVAL, "npb_set_diagnostics_state: the diagnostics rows are not carried (npb_carry_diagnostics first)");
  NPB_USE_DEVICE(h);
  for (int k = 0; k < NPB_DIAG_NUM_CARRIED; k++)
    NPB_HIP(h, hipMemcpyAsync(h->diag + (size_t)g_diag_carried[k].row * h->diag_pitch, buf + (size_t)k * h->n_plants, (size_t)h->n_plants * sizeof(double),
                              hipMemcpyDefault, (hipStream_t)stream));
  NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream));
  return NPB_OK;
}

int npb_set_maintenance_table(NpbHandle *h, const npb_maint_table_t *table) {
  if (!h || !table) return NPB_EINVAL;
  for (int k = 0; k < NPB_MAINT_NPARAM; k++) {
    if (table->rank[k] < 0) continue;
    if (table->action[k] < 0 || table->action[k] >= NPB_MAINT_NACT || table->comparison[k] < 0 || table->comparison[k] > NPB_CMP_NOT_EQUALS ||
        table->priority[k] < NPB_PRIO_LOW || table->priority[k] > NPB_PRIO_EMERGENCY || table->bearing[k] < 0 || table->bearing[k] > NPB_BEARING_THRUST)
      return fail(h, NPB_EINVAL, "npb_set_maintenance_table: action / comparison / priority / bearing code out of range");
  }
  h->maint_table = *table;
  h->maint_table_custom = true;
  h->maint_cache_stale = true;
  return NPB_OK;
}
int npb_set_maintenance_count_buffer(NpbHandle *h, int32_t *counts) {
  if (!h) return NPB_EINVAL;
  h->maint_counts = counts;
  h->maint_cache_stale = true;     /* filled whole before the next step */
  return NPB_OK;
}
/* the episode records read or clear the handle's summary tables: the summary then stays as it is */
static bool er_uses_summary(const NpbHandle *h) { return h->er_on && (h->er.first_created || h->er.clear_summary); }
int npb_set_maintenance_log(NpbHandle *h, void *records, int capacity, uint32_t *cursor) {
  if (!h) return NPB_EINVAL;
  if (capacity < 0) return fail(h, NPB_EINVAL, "npb_set_maintenance_log: capacity must be >= 0");
  if (records && !cursor) return fail(h, NPB_EINVAL, "npb_set_maintenance_log: records without a cursor");
  if (!records && capacity > 0) return fail(h, NPB_EINVAL, "npb_set_maintenance_log: a capacity without records");
  if (((uintptr_t)records & 7u) || ((uintptr_t)cursor & 3u)) return fail(h, NPB_EINVAL, "npb_set_maintenance_log: records must be 8-byte and the cursor 4-byte aligned");
  if (!records && er_uses_summary(h))
    return fail(h, NPB_EINVAL, "npb_set_maintenance_log: episode records that copy or clear the work-order summary are on (npb_set_episode_records), and without a log there is no summary; switch the records off first");
  if (h->summary_on && records && h->summary.consume && capacity < h->n_plants)      /* the summary's own condition on the log it consumes */
    return fail(h, NPB_EINVAL, npb_maint_summary_check(&h->summary, capacity, h->n_plants));
  h->maint_log = npd_maint_log_t{(npb_maint_event_t *)records, records ? cursor : nullptr, records ? capacity : 0};
  h->maint_cache_stale = true;     /* the log's descriptor travels with the rule's constants: uploaded before the next step */
  if (!records) h->summary_on = false;      /* no log, nothing to fold */
  return NPB_OK;
}
size_t npb_maint_event_bytes(void) { return sizeof(npb_maint_event_t); }

/* the per-plant work-order summary (include/npb.h npb_set_maintenance_summary, npd_maint_summary.h) */
const char *npb_maint_summary_check(const npb_maint_summary_desc_t *D, int log_capacity, int n_plants) {
  if (!D) return "npb_set_maintenance_summary: no descriptor";
  if (log_capacity < 0) return "npb_set_maintenance_summary: no maintenance log set (npb_set_maintenance_log first): the summary is folded from its records";
  if (D->n_keys < 1 || D->n_keys > NPB_MAINT_SUMMARY_MAX_KEYS) return "npb_set_maintenance_summary: n_keys must be 1..16 (NPB_MAINT_SUMMARY_MAX_KEYS)";
  for (int j = 0; j < D->n_keys; j++) {
    const npb_maint_summary_key_t &K = D->keys[j];
    if (K.catalog < 0 || K.catalog >= NPB_MAINT_NCATALOG) return "npb_set_maintenance_summary: a key's catalog is none of NPB_MAINT_CATALOG_*";
    /* actions of the catalog (the component catalog with the one automatic action behind it) and the units of the action's kind, or of
     * the catalog's widest kind for "any action" */
    const int nact = K.catalog == NPB_MAINT_CATALOG_FEEDWATER ? NPB_MAINT_NACT : K.catalog == NPB_MAINT_CATALOG_COMPONENT ? NPB_COMPONENT_NACT + 1 : NPB_TURBINE_NACT;
    if (K.action < -1 || K.action >= nact) return "npb_set_maintenance_summary: a key's action is outside its catalog (-1 = any)";
    int units;
    if (K.catalog == NPB_MAINT_CATALOG_FEEDWATER) units = NPB_NUM_PUMPS;
    else if (K.catalog == NPB_MAINT_CATALOG_COMPONENT)
      units = K.action < 0 ? NPB_COMPONENT_UNITS(NPB_COMPONENT_SG) : K.action == NPB_CA_AUTO_CONDENSER_TUBE_PLUGGING ? 1 : NPB_COMPONENT_UNITS(g_component_actions[K.action].kind);
    else units = K.action < 0 ? NPB_TURBINE_UNITS(NPB_TURBINE_STAGE) : NPB_TURBINE_UNITS(g_turbine_actions[K.action].kind);
    if (K.unit < -1 || K.unit >= units) return "npb_set_maintenance_summary: a key's unit is outside its catalog (-1 = any)";
    if (!(K.kinds & NPB_MAINT_CATALOG_KINDS(K.catalog))) return "npb_set_maintenance_summary: a key's kinds are empty: no NPB_MAINT_EVENT_* kind of its catalog";
  }
  if (!D->first_created || !D->first_completed || !D->n_created || !D->n_completed || !D->folded || !D->dropped)
    return "npb_set_maintenance_summary: the four tables and the folded / dropped words must not be NULL";
  if (((uintptr_t)D->first_created & 7u) || ((uintptr_t)D->first_completed & 7u) || ((uintptr_t)D->n_created & 3u) || ((uintptr_t)D->n_completed & 3u) ||
      ((uintptr_t)D->folded & 3u) || ((uintptr_t)D->dropped & 3u))
    return "npb_set_maintenance_summary: the time tables must be 8-byte, the count tables and the words 4-byte aligned";
  if (D->consume && log_capacity < n_plants)
    return "npb_set_maintenance_summary: consume mode needs a log capacity of at least n_plants records, or it loses events as a matter of course";
  return nullptr;
}
int npb_set_maintenance_summary(NpbHandle *h, const npb_maint_summary_desc_t *desc) {
  if (!h) return NPB_EINVAL;
  if (er_uses_summary(h))
    return fail(h, NPB_EINVAL, "npb_set_maintenance_summary: episode records that copy or clear the work-order summary are on (npb_set_episode_records) and hold its tables and key count; switch the records off first");
  if (!desc) { h->summary_on = false; return NPB_OK; }
  if (const char *why = npb_maint_summary_check(desc, h->maint_log.cursor ? h->maint_log.capacity : -1, h->n_plants)) return fail(h, NPB_EINVAL, why);
  if (!h->summary_ticket) {
    NPB_USE_DEVICE(h);
    hipError_t e = hipMalloc((void **)&h->summary_ticket, 256);
    if (e != hipSuccess) { h->summary_ticket = nullptr; return fail(h, NPB_EHIP, "npb_set_maintenance_summary: hipMalloc of the ticket word failed", e); }
    NPB_HIP(h, hipMemset(h->summary_ticket, 0, 256));
  }
  h->summary = *desc;
  h->summary_on = true;
  return NPB_OK;
}
/* behind every kernel that can append records, on its stream */
static void summary_fold(NpbHandle *h, hipStream_t stream) {
  if (h->summary_on) npb_launch_maint_summary_fold(&h->summary, h->maint_log, h->summary_ticket, h->n_plants, stream);
}
int npb_maint_summary_fold(NpbHandle *h, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->summary_on) return fail(h, NPB_EINVAL, "npb_maint_summary_fold: no summary set (npb_set_maintenance_summary first)");
  NPB_USE_DEVICE(h);
  summary_fold(h, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
int npb_maint_summary_clear(NpbHandle *h, const uint8_t *mask, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->summary_on) return fail(h, NPB_EINVAL, "npb_maint_summary_clear: no summary set (npb_set_maintenance_summary first)");
  NPB_USE_DEVICE(h);
  npb_launch_maint_summary_clear(&h->summary, mask, h->n_plants, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}

int npb_perform_maintenance(NpbHandle *h, const int32_t *action, const int32_t *pump, const int32_t *bearing, const double *target_level,
                            uint8_t *success, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!action || !pump) return fail(h, NPB_EINVAL, "npb_perform_maintenance: the action and pump columns must not be NULL");
  NPB_USE_DEVICE(h);
  /* maint_cache_stale is left alone.  The cooldown cache of the step kernels' threshold screen holds, per (plant, pump), which table rows
   * are inside their cooldown and until when: a function of the mpump.last_violation_time stamps, the table and the clock
   * (npd_maint_cache_entry), none of which a handler writes -- it changes members of the pump section only, and those the screen reads
   * fresh from the pump phase's registers at every step (npd_maint_pump_hit).  Nor does the caller's count column move: an operator
   * action is not counted in maintenance_actions_performed.  The log's descriptor travels as a kernel argument, so the call does not
   * depend on the rule's constants having been uploaded (they are only with params.maint_enabled). */
  h->K->operator_maint(h->n_plants, NPB_N(h), h->f64, action, pump, bearing, target_level, success, h->maint_log, (hipStream_t)stream);
  summary_fold(h, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}

int npb_perform_component_maintenance(NpbHandle *h, const int32_t *action, const int32_t *unit, const int32_t *option, const double *amount,
                                      uint8_t *success, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!action) return fail(h, NPB_EINVAL, "npb_perform_component_maintenance: the action column must not be NULL");
  NPB_USE_DEVICE(h);
  /* the components a mode steps are the ones it can service: the reference without its secondary side has no object to call
   * (sim.secondary_physics is None), and primary + steam generators steps no condenser.  maint_cache_stale is left alone, as in
   * npb_perform_maintenance: no handler here writes a pump, a stamp or the table. */
  const unsigned kinds = h->params.mode == NPB_MODE_FULL ? 0xfu
                       : h->params.mode == NPB_MODE_PRIMARY_SG ? (1u << NPB_COMPONENT_SG) | (1u << NPB_COMPONENT_SGSYS) : 0u;
  h->K->operator_component_maint(h->n_plants, NPB_N(h), h->f64, action, unit, option, amount, success, kinds, h->maint_log,
                                 (hipStream_t)stream);
  summary_fold(h, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}

int npb_perform_turbine_maintenance(NpbHandle *h, const int32_t *action, const int32_t *unit, uint8_t *success, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!action) return fail(h, NPB_EINVAL, "npb_perform_turbine_maintenance: the action column must not be NULL");
  NPB_USE_DEVICE(h);
  /* only the full plant steps the turbine: without its secondary side the reference has no object to call, and primary + steam generators
   * carries no turbine.  maint_cache_stale is left alone, as in npb_perform_maintenance: no handler here writes a pump, a stamp or the table. */
  h->K->operator_turbine_maint(h->n_plants, NPB_N(h), h->f64, action, unit, success, h->params.mode == NPB_MODE_FULL, h->maint_log,
                               (hipStream_t)stream);
  summary_fold(h, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
void npb_default_maintenance_table(npb_maint_table_t *table) { if (table) npb_maint_table_default(table); }

void npb_default_component_maintenance_table(npb_component_maint_table_t *table) { if (table) npb_component_maint_table_default(table); }
static const char *const g_cmaint_params[] = {
#define NPB__X(kind, id, name) name,
  NPB_CMAINT_PARAMS(NPB__X)
#undef NPB__X
};
static const int g_cmaint_param_kinds[] = {
#define NPB__X(kind, id, name) NPB_COMPONENT_##kind,
  NPB_CMAINT_PARAMS(NPB__X)
#undef NPB__X
};
static_assert(sizeof(g_cmaint_params) / sizeof(g_cmaint_params[0]) == NPB_CMAINT_NPARAM, "component parameter catalog");
int npb_component_maint_num_params(void) { return NPB_CMAINT_NPARAM; }
const char *npb_component_maint_param_name(int k) { return k >= 0 && k < NPB_CMAINT_NPARAM ? g_cmaint_params[k] : nullptr; }
int npb_component_maint_param_kind(int k) { return k >= 0 && k < NPB_CMAINT_NPARAM ? g_cmaint_param_kinds[k] : -1; }

int npb_set_component_maintenance(NpbHandle *h, const npb_component_maint_table_t *table) {
  if (!h) return NPB_EINVAL;
  /* either way the rule changes hands between the step kernels and npb_maint_all_kernel, which keeps no cooldown cache: the pump
   * stamps it has moved are unknown to the step kernels' screen */
  h->maint_cache_stale = true;
  if (!table) { h->cm_on = false; return NPB_OK; }
  if (h->params.mode != NPB_MODE_FULL) return fail(h, NPB_EINVAL, "npb_set_component_maintenance: full mode only (the other modes step no condenser)");
  for (int q = 0; q < NPB_CMAINT_NPARAM; q++) {
    if (table->rank[q] < 0) continue;
    if (table->comparison[q] < 0 || table->comparison[q] > NPB_CMP_NOT_EQUALS || table->priority[q] < NPB_PRIO_LOW || table->priority[q] > NPB_PRIO_EMERGENCY)
      return fail(h, NPB_EINVAL, "npb_set_component_maintenance: comparison / priority code out of range");
    if (table->action[q] == NPB_CA_AUTO_CONDENSER_TUBE_PLUGGING && g_cmaint_param_kinds[q] == NPB_COMPONENT_COND) continue;
    if (table->action[q] < 0 || table->action[q] >= NPB_COMPONENT_NACT || g_component_actions[table->action[q]].kind != g_cmaint_param_kinds[q])
      return fail(h, NPB_EINVAL, "npb_set_component_maintenance: a row's action is not an entry of the COMPONENT catalog (include/npb_maint.h) of the row's component kind");
  }
  NPB_USE_DEVICE(h);
  const bool fresh = !h->cm_side;
  if (fresh) {
    hipError_t e = hipMalloc(&h->cm_side, npb_launch_cmaint_side_bytes(h->pitch));
    if (e != hipSuccess) { h->cm_side = nullptr; return fail(h, NPB_EHIP, "npb_set_component_maintenance: hipMalloc of the side state failed", e); }
  }
  h->cm_table = *table;
  /* the call has no stream: whatever the handle's earlier steps have in flight, on any stream, reads the old table first */
  NPB_HIP(h, hipDeviceSynchronize());
  NPB_HIP(h, hipMemcpy(h->cm_side, &h->cm_table, sizeof(h->cm_table), hipMemcpyHostToDevice));      /* (npd_cmaint_consts_t is the table) */
  if (fresh) {      /* no stamp, no order; switched off and on again the side state is kept, as the mpump section is */
    npb_launch_cmaint_init(h->cm_side, h->pitch, nullptr, h->n_plants, nullptr);
    NPB_HIP(h, hipGetLastError());
    NPB_HIP(h, hipDeviceSynchronize());
  }
  h->cm_on = true;
  return NPB_OK;
}
size_t npb_component_maintenance_state_bytes(const NpbHandle *h) { return h ? (size_t)NPB_CMAINT_SIDE_DOUBLES * (size_t)h->n_plants * sizeof(double) : 0; }
int npb_get_component_maintenance_state(NpbHandle *h, double *buf, void *stream) {
  if (!h || !buf) return NPB_EINVAL;
  if (!h->cm_side) return fail(h, NPB_EINVAL, "npb_get_component_maintenance_state: no side state (npb_set_component_maintenance first)");
  NPB_USE_DEVICE(h);
  NPB_HIP(h, hipMemcpy2DAsync(buf, (size_t)h->n_plants * sizeof(double), cm_state(h), h->pitch * sizeof(double), (size_t)h->n_plants * sizeof(double),
                              NPB_CMAINT_SIDE_DOUBLES, hipMemcpyDefault, (hipStream_t)stream));
  NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream));
  return NPB_OK;
}
int npb_set_component_maintenance_state(NpbHandle *h, const double *buf, void *stream) {
  if (!h || !buf) return NPB_EINVAL;
  if (!h->cm_side) return fail(h, NPB_EINVAL, "npb_set_component_maintenance_state: no side state (npb_set_component_maintenance first)");
  NPB_USE_DEVICE(h);
  NPB_HIP(h, hipMemcpy2DAsync(cm_state(h), h->pitch * sizeof(double), buf, (size_t)h->n_plants * sizeof(double), (size_t)h->n_plants * sizeof(double),
                              NPB_CMAINT_SIDE_DOUBLES, hipMemcpyDefault, (hipStream_t)stream));
  NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream));
  return NPB_OK;
}

int npb_reset(NpbHandle *h, const uint8_t *mask, void *stream) {
  if (!h) return NPB_EINVAL;
  NPB_USE_DEVICE(h);
  h->maint_cache_stale = true;
  h->K->init(&h->params, h->n_plants, NPB_N(h), h->f64, mask, (hipStream_t)stream);
  if (h->cm_on) npb_launch_cmaint_init(h->cm_side, h->pitch, mask, h->n_plants, (hipStream_t)stream);      /* beside the mpump section the init kernel has just written */
  if (h->diag_carry) {      /* the carried diagnostics rows of a freshly constructed plant */
    npb_diag_carried_values_t fresh;
    for (int k = 0; k < NPB_DIAG_NUM_CARRIED; k++) fresh.v[k] = g_diag_carried[k].fresh;
    npb_launch_diag_carried_put(h->diag, h->diag_pitch, mask, h->n_plants, h->pitch, fresh, (hipStream_t)stream);
  }
  clear_episodes(h, mask, true, (hipStream_t)stream);
  restart_streams(h, false, (hipStream_t)stream);
  core_restart(h, mask, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}

int npb_reset_reference(NpbHandle *h, const uint8_t *mask, int start_at_steady_state, void *stream) {
  if (!h) return NPB_EINVAL;
  NPB_USE_DEVICE(h);
  h->maint_cache_stale = true;
  h->K->reset(&h->params, h->n_plants, NPB_N(h), h->f64, mask, start_at_steady_state != 0, (hipStream_t)stream);
  if (h->diag_carry) npb_launch_diag_carried_put(h->diag, h->diag_pitch, mask, h->n_plants, h->pitch, diag_reference_reset_values(), (hipStream_t)stream);
  clear_episodes(h, mask, true, (hipStream_t)stream);
  restart_streams(h, false, (hipStream_t)stream);
  core_restart(h, mask, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}

/* one member of every plant <-> a contiguous buffer: a small gather / scatter kernel (members share columns and
 * outputs are stored as float, so this is never a plain copy); host buffers go through the staging column */
static int field_args(NpbHandle *h, int kind, int slot, int *col, int *sub, int *akind, size_t *bytes) {
  if (kind != NPB_KIND_F64 && kind != NPB_KIND_I32) return fail(h, NPB_EINVAL, "field kind must be NPB_KIND_F64 or NPB_KIND_I32");
  if (!locate(h->storage, kind, slot, col, sub, akind)) return fail(h, NPB_EINVAL, "field slot out of range");
  *bytes = (size_t)h->n_plants * (kind == NPB_KIND_F64 ? sizeof(double) : sizeof(int32_t));
  return NPB_OK;
}

int npb_get_field(NpbHandle *h, int kind, int slot, void *buf, int buf_is_device, void *stream) {
  if (!h || !buf) return NPB_EINVAL;
  int col, sub, akind; size_t bytes;
  int rc = field_args(h, kind, slot, &col, &sub, &akind, &bytes);
  if (rc) return rc;
  NPB_USE_DEVICE(h);
  void *dst = buf_is_device ? buf : (void *)h->convert;
  h->K->field_get(h->f64, NPB_N(h), col, sub, akind, dst, h->n_plants, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  if (!buf_is_device) {
    NPB_HIP(h, hipMemcpyAsync(buf, dst, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream));
  }
  return NPB_OK;
}

int npb_set_field(NpbHandle *h, int kind, int slot, const void *buf, int buf_is_device, void *stream) {
  if (!h || !buf) return NPB_EINVAL;
  int col, sub, akind; size_t bytes;
  int rc = field_args(h, kind, slot, &col, &sub, &akind, &bytes);
  if (rc) return rc;
  NPB_USE_DEVICE(h);
  h->maint_cache_stale = true;      /* a stamp, a pump member or the clock may just have been written */
  const void *src = buf;
  if (!buf_is_device) {
    NPB_HIP(h, hipMemcpyAsync(h->convert, buf, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    src = h->convert;
  }
  h->K->field_set(h->f64, NPB_N(h), col, sub, akind, src, h->n_plants, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  if (!buf_is_device) NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream));
  return NPB_OK;
}

int npb_gather_fields(NpbHandle *h, int n_fields, const int *kinds, const int *slots, double *out, void *stream) {
  if (!h || !kinds || !slots || !out || n_fields <= 0 || n_fields > NPB_TOTAL_F64 + NPB_TOTAL_I32) return NPB_EINVAL;
  NPB_USE_DEVICE(h);
  std::vector<int> key(2 * (size_t)n_fields);
  for (int f = 0; f < n_fields; f++) { key[2 * f] = kinds[f]; key[2 * f + 1] = slots[f]; }
  if (key != h->plan_key) { /* a log asks for the same members every time: build and upload the plan once */
    std::vector<int> plan(3 * (size_t)n_fields);
    for (int f = 0; f < n_fields; f++)
      if ((kinds[f] != NPB_KIND_F64 && kinds[f] != NPB_KIND_I32) || !locate(h->storage, kinds[f], slots[f], &plan[3 * f], &plan[3 * f + 1], &plan[3 * f + 2]))
        return fail(h, NPB_EINVAL, "npb_gather_fields: bad field kind or slot");
    if (!h->plan_dev) NPB_HIP(h, hipMalloc((void **)&h->plan_dev, sizeof(int) * 3 * (NPB_TOTAL_F64 + NPB_TOTAL_I32)));
    NPB_HIP(h, hipMemcpyAsync(h->plan_dev, plan.data(), sizeof(int) * plan.size(), hipMemcpyHostToDevice, (hipStream_t)stream));
    NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream));
    h->plan_key = key;
  }
  h->K->gather(h->f64, NPB_N(h), h->plan_dev, n_fields, out, h->n_plants, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}

/* samplers: a watch list of plants, arena members and side buffers in one launch per sample (include/npb.h) */
int npb_sampler_create(NpbHandle *h, const npb_sampler_desc_t *desc, int *sampler) {
  if (!h) return fail(nullptr, NPB_EINVAL, "npb_sampler_create: NULL handle");
  if (!desc || !sampler) return fail(h, NPB_EINVAL, "npb_sampler_create: NULL request or NULL sampler id");
  *sampler = -1;
  char msg[192];
  if (desc->n_watched <= 0 || !desc->plants) return fail(h, NPB_EINVAL, "npb_sampler_create: n_watched must be at least 1, with its plant ids");
  std::vector<bool> seen((size_t)h->n_plants, false);
  for (int j = 0; j < desc->n_watched; j++) {
    const int32_t p = desc->plants[j];
    if (p < 0 || p >= h->n_plants) {
      snprintf(msg, sizeof msg, "npb_sampler_create: plant id %d is outside [0, %d)", (int)p, h->n_plants);
      return fail(h, NPB_EINVAL, msg);
    }
    if (seen[(size_t)p]) {
      snprintf(msg, sizeof msg, "npb_sampler_create: plant id %d is listed twice", (int)p);
      return fail(h, NPB_EINVAL, msg);
    }
    seen[(size_t)p] = true;
  }
  if (desc->n_fields < 0 || desc->n_fields > NPB_TOTAL_F64 + NPB_TOTAL_I32 || (desc->n_fields > 0 && (!desc->kinds || !desc->slots)))
    return fail(h, NPB_EINVAL, "npb_sampler_create: bad number of fields, or fields without kinds / slots");
  std::vector<int> plan(3 * (size_t)desc->n_fields);
  for (int f = 0; f < desc->n_fields; f++)
    if ((desc->kinds[f] != NPB_KIND_F64 && desc->kinds[f] != NPB_KIND_I32) ||
        !locate(h->storage, desc->kinds[f], desc->slots[f], &plan[3 * f], &plan[3 * f + 1], &plan[3 * f + 2])) {
      snprintf(msg, sizeof msg, "npb_sampler_create: bad field kind or slot (field %d: kind %d, slot %d)", f, desc->kinds[f], desc->slots[f]);
      return fail(h, NPB_EINVAL, msg);
    }
  if (desc->n_sources < 0 || (desc->n_sources > 0 && !desc->sources)) return fail(h, NPB_EINVAL, "npb_sampler_create: side sources without their descriptors");
  static const size_t width[] = {sizeof(double), sizeof(float), sizeof(int32_t), sizeof(uint8_t)};     /* NPB_SAMPLE_* */
  std::vector<npb_sample_row_t> side;
  for (int k = 0; k < desc->n_sources; k++) {
    const npb_sample_source_t &S = desc->sources[k];
    if (!S.base) { snprintf(msg, sizeof msg, "npb_sampler_create: side source %d has a NULL base", k); return fail(h, NPB_EINVAL, msg); }
    if (S.type < NPB_SAMPLE_F64 || S.type > NPB_SAMPLE_U8) {
      snprintf(msg, sizeof msg, "npb_sampler_create: side source %d has the unknown element type %d", k, S.type);
      return fail(h, NPB_EINVAL, msg);
    }
    if (S.rows <= 0 || S.row_stride < 0 || S.plant_stride < 0) {
      snprintf(msg, sizeof msg, "npb_sampler_create: side source %d needs rows >= 1 and strides >= 0", k);
      return fail(h, NPB_EINVAL, msg);
    }
    for (int q = 0; q < S.rows; q++)
      side.push_back(npb_sample_row_t{(const char *)S.base + (size_t)q * (size_t)S.row_stride * width[S.type], S.plant_stride, S.type, 0});
  }
  const size_t n_rows = (size_t)desc->n_fields + side.size();
  if (n_rows == 0 || n_rows > 65535) return fail(h, NPB_EINVAL, "npb_sampler_create: a request needs between 1 and 65 535 rows");
  NPB_USE_DEVICE(h);
  /* one allocation, the widest alignment first */
  const size_t side_bytes = side.size() * sizeof(npb_sample_row_t), plan_bytes = plan.size() * sizeof(int), ids_bytes = (size_t)desc->n_watched * sizeof(int32_t);
  std::vector<char> host(side_bytes + plan_bytes + ids_bytes);
  if (side_bytes) memcpy(host.data(), side.data(), side_bytes);
  if (plan_bytes) memcpy(host.data() + side_bytes, plan.data(), plan_bytes);
  memcpy(host.data() + side_bytes + plan_bytes, desc->plants, ids_bytes);
  void *dev = nullptr;
  hipError_t e = hipMalloc(&dev, host.size());
  if (e != hipSuccess) return fail(h, NPB_ENOMEM, "npb_sampler_create: hipMalloc of the sampler's plan failed", e);
  e = hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(dev); return fail(h, NPB_EHIP, "npb_sampler_create: upload of the sampler's plan failed", e); }
  Sampler *sm = new Sampler{dev, (const npb_sample_row_t *)dev, (const int *)((const char *)dev + side_bytes),
                            (const int32_t *)((const char *)dev + side_bytes + plan_bytes), desc->n_fields, (int)n_rows, desc->n_watched};
  size_t id = 0;
  while (id < h->samplers.size() && h->samplers[id]) id++;
  if (id == h->samplers.size()) h->samplers.push_back(sm); else h->samplers[id] = sm;
  *sampler = (int)id;
  return NPB_OK;
}

int npb_sampler_sample(NpbHandle *h, int sampler, double *out, void *stream) {
  if (!h) return fail(nullptr, NPB_EINVAL, "npb_sampler_sample: NULL handle");
  if (sampler < 0 || (size_t)sampler >= h->samplers.size() || !h->samplers[(size_t)sampler])
    return fail(h, NPB_EINVAL, "npb_sampler_sample: unknown or destroyed sampler id");
  if (!out) return fail(h, NPB_EINVAL, "npb_sampler_sample: NULL output buffer");
  NPB_USE_DEVICE(h);
  const Sampler *sm = h->samplers[(size_t)sampler];
  h->A->sample(h->f64, NPB_N(h), sm->plan, sm->n_fields, sm->side, sm->n_rows, sm->ids, sm->n_watched, out, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}

int npb_sampler_destroy(NpbHandle *h, int sampler) {
  if (!h) return fail(nullptr, NPB_EINVAL, "npb_sampler_destroy: NULL handle");
  if (sampler < 0 || (size_t)sampler >= h->samplers.size() || !h->samplers[(size_t)sampler])
    return fail(h, NPB_EINVAL, "npb_sampler_destroy: unknown or destroyed sampler id");
  NPB_USE_DEVICE(h);
  Sampler *sm = h->samplers[(size_t)sampler];
  h->samplers[(size_t)sampler] = nullptr;
  (void)hipFree(sm->dev);      /* (hipFree waits for the device: a sample still in flight finishes first) */
  delete sm;
  return NPB_OK;
}

int npb_state_arena(NpbHandle *h, void **arena, size_t *pitch, int *storage) {
  if (!h) return NPB_EINVAL;
  if (h->seg && arena) {      /* column * pitch + plant is NOT where a plant's element is on this arena: say so instead of handing out a pointer */
    return fail(h, NPB_EINVAL, "npb_state_arena: this handle's arena is segmented (npb_state_arena_segment plants per segment): column * pitch + plant is "
                               "not where a plant's element is; use npb_state_arena_layout, which reports the segment size with the pointer");
  }
  if (arena) { *arena = h->f64; h->maint_cache_stale = true; }      /* the caller may write the arena through this pointer (before the next step) */
  if (pitch) *pitch = h->seg ? h->seg : h->pitch;
  if (storage) *storage = h->storage;
  return NPB_OK;
}

int npb_state_arena_layout(NpbHandle *h, void **arena, size_t *pitch, size_t *segment, int *columns, int *storage) {
  if (!h) return NPB_EINVAL;
  if (arena) { *arena = h->f64; h->maint_cache_stale = true; }      /* a query of the layout alone (arena = NULL) leaves the maintenance cache alone */
  if (pitch) *pitch = h->seg ? h->seg : h->pitch;
  if (segment) *segment = h->seg;
  if (columns) *columns = h->storage == NPB_STORAGE_F32 ? (int)NPB_TOTAL_COL32 : (int)NPB_TOTAL_COL64;
  if (storage) *storage = h->storage;
  return NPB_OK;
}

size_t npb_state_arena_segment(const NpbHandle *h) { return h ? h->seg : 0; }

int npb_locate_field(const NpbHandle *h, int kind, int slot, int *column, int *sub, int *access) {
  if (!h) return NPB_EINVAL;
  int c, s2, a;
  if ((kind != NPB_KIND_F64 && kind != NPB_KIND_I32) || !locate(h->storage, kind, slot, &c, &s2, &a)) return NPB_EINVAL;
  if (column) *column = c;
  if (sub) *sub = s2;
  if (access) *access = a;
  return NPB_OK;
}

/* the step's launch of the policy: every plant's features in, the controls' input, value, logp and the extras slots out, at draw t */
static npd_policy_run_t policy_run(const NpbHandle *h) {
  const npb_policy_desc_t &D = h->pol.D;
  npd_policy_run_t R = {};
  R.x = h->feat.out; R.x_f64 = h->feat.out_f64; R.rows = h->n_plants;
  R.act = (void *)h->ctl.in; R.act_f64 = h->ctl.in_f64;
  R.value = D.value; R.logp = D.logp; R.extras = D.extras_in; R.n_extras = D.n_extras; R.value_slot = D.value_slot; R.logp_slot = D.logp_slot;
  R.seed = D.seed; R.t = h->pol_t; R.first = (uint32_t)D.first_plant; R.deterministic = D.deterministic;
  return R;
}
/* every launch of the handle's policy: the recurrent kernel with a core (`cell`: what of the hidden state it reads and writes), else the MLP's (cell NULL) */
static void policy_launch(const NpbHandle *h, const npd_policy_run_t *R, const npd_policy_core_run_t *cell, void *stream) {
  if (cell) npb_launch_policy_core(&h->pol, &h->core, R, cell, (hipStream_t)stream);
  else npb_launch_policy(&h->pol, R, (hipStream_t)stream);
}
int npb_step(NpbHandle *h, const int32_t *action, const double *magnitude, const double *power_setpoint,
             const double *noise_z, const double *cooling_water_temp, double *obs, double *reward, uint8_t *done,
             uint32_t *trip_flags, double *info, void *stream) {
  if (!h) return NPB_EINVAL;
  if (h->autoreset && !done)      /* the episode kernel reads the step's terminations from the done column */
    return fail(h, NPB_EINVAL, "npb_step: autoreset is on (npb_set_autoreset) and needs the done column: it must not be NULL");
  if (h->er_on && h->er.final_obs && !obs)
    return fail(h, NPB_EINVAL, "npb_step: episode records with final_obs are on (npb_set_episode_records) and copy the terminal row of the obs column: it must not be NULL");
  if (h->params.heat_source == NPB_HEAT_EXTERNAL && !noise_z)      /* a NULL column would read as 0 MW thermal, silently */
    return fail(h, NPB_EINVAL, "npb_step: params.heat_source is NPB_HEAT_EXTERNAL, whose thermal power arrives in the noise_z column (include/npb_params.h): it must not be NULL");
  if (h->ctl.age) {      /* an input an axis fills has one writer */
    const double *const given[NPB_CONTROL_INPUT_COUNT] = {power_setpoint, cooling_water_temp};
    static const char *const name[NPB_CONTROL_INPUT_COUNT] = {"power_setpoint", "cooling_water_temp"};
    for (int i = 0; i < NPB_CONTROL_INPUT_COUNT; i++)
      if (h->ctl_axis[i] >= 0 && given[i]) {
        char what[200];
        snprintf(what, sizeof what, "npb_step: the %s column must be NULL: axis %d of the controls fills it (npb_set_controls)", name[i], h->ctl_axis[i]);
        return fail(h, NPB_EINVAL, what);
      }
  }
  if (h->ro.n_final) {      /* the rollout: a slot to record into, the columns it records, and rows for every truncation the horizon can hold */
    if (h->ro.t >= h->ro.D.horizon)
      return fail(h, NPB_EINVAL, "npb_step: the rollout is full (npb_set_rollout: t == horizon): npb_rollout_begin rewinds it");
    if (!h->task.terms && (!reward || !done))      /* (a task brings its own) */
      return fail(h, NPB_EINVAL, "npb_step: a rollout is set (npb_set_rollout) and records the reward and done columns: they must not be NULL");
    if (h->autoreset && h->max_episode_steps > 0 &&
        h->ro.D.final_rows < (h->ro.D.horizon + h->max_episode_steps - 1) / h->max_episode_steps)
      return fail(h, NPB_EINVAL, "npb_step: the rollout's final_rows is below ceil(horizon / max_episode_steps): a truncated plant would find no row for its terminal stack (npb_set_rollout)");
  }
  if (h->norm.streams && h->norm.reward_on && !h->task.terms && (!reward || !done))      /* (a task brings its own) */
    return fail(h, NPB_EINVAL, "npb_step: a normaliser with the return stream is set (npb_set_normalizer) and reads the reward and done columns: they must not be NULL");
  /* what the autoreset's restores take along beside the arena, from the bank while it has slots, else from the snapshot.  The step
   * reports a source without the diagnostics rows first, then the component maintenance's own needs, then a source without its state */
  const bool from_bank = h->bank && h->next_slot;
  npb_side_restores_t side = {};
  const int refused = h->autoreset ? side_restores_of(h, from_bank, true, &side) : -1;
  if (refused == NPB_SIDE_DIAG) return fail(h, NPB_EINVAL, side_refusal(refused, from_bank));
  if (h->cm_on && (!h->params.maint_enabled || h->params.mode != NPB_MODE_FULL))
    return fail(h, NPB_EINVAL, "npb_step: the component maintenance is on (npb_set_component_maintenance) and needs params.maint_enabled and the full mode");
  if (refused >= 0) return fail(h, NPB_EINVAL, side_refusal(refused, from_bank));
  NPB_USE_DEVICE(h);
  npb_episode_streams_take_t es_take = {};
  if (h->es_on) {      /* episode streams: a column the caller leaves out is the handle's current row of that stream */
    const npb_episode_streams_t &S = h->es;
    const bool take_noise = S.noise.key && !noise_z, take_prof = S.prof.key && !power_setpoint;
    const bool fill_noise = take_noise && h->es_noise_cur >= S.block, fill_prof = take_prof && h->es_prof_cur >= S.block;
    if (fill_noise || fill_prof) {
      npb_launch_episode_streams_fill(&S, fill_noise ? 0 : S.block, fill_prof ? 0 : S.block, (hipStream_t)stream);
      if (fill_noise) h->es_noise_cur = 0;
      if (fill_prof) h->es_prof_cur = 0;
    }
    const double *target = nullptr;
    if (take_noise) noise_z = S.noise_rows + (size_t)h->es_noise_cur++ * h->n_plants;
    if (take_prof) {
      power_setpoint = S.setpoint_rows + (size_t)h->es_prof_cur * h->n_plants;
      target = S.target_rows + (size_t)h->es_prof_cur++ * h->n_plants;
    }
    /* the rows taken go into the caller's columns in the restart kernel's launch behind the step (the mode needs the autoreset) */
    es_take = npb_episode_streams_take_t{noise_z, power_setpoint, target, take_noise ? h->es_noise_out : nullptr, take_prof ? h->es_setpoint_out : nullptr,
                                         take_prof ? h->es_target_out : nullptr};
  }
  if (h->pol.theta) {      /* the policy: the features read, the controls' input, value and log-probability written, in front of the rollout's record of them */
    const npd_policy_run_t run = policy_run(h);
    npd_policy_core_run_t cell = {};
    if (h->core.primed) {      /* with a core: the cell first, its hidden state restarted with the episode; slot 0 of a rollout keeps the state it read */
      cell.h = cell.h_out = h->core.hidden; cell.first_out = h->ro.n_final && h->ro.t == 0 ? h->core.first : nullptr;
      cell.primed = h->core.primed; cell.seen = h->core.seen; cell.index = h->ep_index; cell.remember = 1;
      if (h->seg_every && h->ro.n_final && h->ro.t % h->seg_every == 0 && h->ro.t / h->seg_every < h->seg_rows)      /* a slot that begins a segment keeps it too */
        cell.start_out = h->seg_starts + (size_t)(h->ro.t / h->seg_every) * (size_t)h->n_plants * (size_t)h->core.H;
    }
    policy_launch(h, &run, h->core.primed ? &cell : nullptr, stream);
    if (!h->pol.D.deterministic) h->pol_t++;
  }
  if (h->ro.n_final)      /* the rollout's slot t: what the policy saw and what it wrote, before the controls kernel and the step change either */
    npb_launch_rollout_pre(&h->ro, h->feat.out, h->ctl.age ? h->ctl.in : nullptr, h->n_plants, (hipStream_t)stream);
  if (h->ctl.age) {      /* the caller's policy outputs: the actuators moved, the input columns filled, in front of the step */
    h->A->controls(h->f64, NPB_N(h), &h->ctl, &h->params, h->n_plants, h->ep_index, (hipStream_t)stream);
    if (h->ctl_axis[NPB_CONTROL_INPUT_POWER_SETPOINT] >= 0) power_setpoint = h->ctl.column[NPB_CONTROL_INPUT_POWER_SETPOINT];
    if (h->ctl_axis[NPB_CONTROL_INPUT_COOLING_WATER_TEMP] >= 0) cooling_water_temp = h->ctl.column[NPB_CONTROL_INPUT_COOLING_WATER_TEMP];
    if (h->ord.since) {      /* the order rules on the held values: the firing plants serviced as npb_perform_* services them, their records folded */
      h->A->control_orders(h->f64, NPB_N(h), &h->ord, h->maint_log, h->n_plants, (hipStream_t)stream);
      summary_fold(h, (hipStream_t)stream);
    }
  }
  npb_maint_table_t table;
  const bool maint = h->params.maint_enabled != 0;
  const bool in_step = maint && !h->cm_on;      /* the rule inside the step kernels (pumps only); with the components on it is a launch of its own */
  if (maint) {
    table = h->maint_table;
    if (!h->maint_table_custom) {   /* with the default table the two oil_level params of ABI version 1 still set their row */
      table.threshold[NPB_MP_OIL_LEVEL] = h->params.maint_oil_level_threshold;
      table.cooldown_hours[NPB_MP_OIL_LEVEL] = h->params.maint_oil_level_cooldown_hours;
    }
    if (h->maint_cache_stale) {
      /* parameters, table, state or clock may have changed since the last step: the rule's constants go to the device anew and
       * the screen's cooldown cache is zeroed (= nothing known: every wave is looked at once and its entries rebuilt) */
      h->maint_consts_host.resize(npb_launch_maint_consts_bytes());
      npb_launch_maint_consts(&h->params, &table, h->maint_log, h->maint_consts_host.data());
      NPB_HIP(h, hipMemcpyAsync(h->maint_side, h->maint_consts_host.data(), h->maint_consts_host.size(), hipMemcpyHostToDevice, (hipStream_t)stream));
      NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream));      /* the host copy may change again before an asynchronous copy would read it */
      NPB_HIP(h, hipMemsetAsync((char *)h->maint_side + npb_launch_maint_cache_offset(), 0, npb_launch_maint_side_bytes(h->pitch) - npb_launch_maint_cache_offset(),
                                (hipStream_t)stream));
      if (h->maint_counts) {       /* the caller's event-count column: whole once, then kept by the rule for the plants whose count it moves */
        int col, sub, akind;
        if (locate(h->storage, NPB_KIND_I32, NPB_MAINT_I32_BASE + NPB_I32_SLOT(npb_maint_t, MAINT, maintenance_actions_performed), &col, &sub, &akind))
          h->K->field_get(h->f64, NPB_N(h), col, sub, akind, h->maint_counts, h->n_plants, (hipStream_t)stream);
      }
      h->maint_cache_stale = false;
    }
  }
  h->last_kernel = h->K->step(&h->params, h->n_plants, NPB_N(h), h->f64, action, magnitude, power_setpoint,
                              noise_z, cooling_water_temp, obs, reward, done, trip_flags, info, h->step_kernel, h->diag, h->diag_pitch,
                              in_step ? &table : nullptr, in_step ? h->maint_side : nullptr, in_step ? h->maint_counts : nullptr, (hipStream_t)stream);
  if (h->cm_on)      /* the plain step kernel has run: the whole rule, pumps, generators and condenser in one queue */
    h->K->maint_all(NPB_N(h), h->f64, h->maint_side, h->cm_side, h->maint_counts, h->n_plants, h->diag, h->diag_pitch, (hipStream_t)stream);
  else if (maint && h->params.mode != NPB_MODE_FULL)   /* a full-mode step kernel has run the rule itself, for the waves whose pump phase found something */
    h->K->maint(NPB_N(h), h->f64, h->maint_side, h->maint_counts, h->n_plants, (hipStream_t)stream);
  if (maint) summary_fold(h, (hipStream_t)stream);      /* the rule has appended this step's records: the summary is current when the call returns */
  if (h->task.terms) {      /* the caller's reward and termination rule: everything below that deals with episodes reads the task's columns in place of the step's */
    h->A->task(h->f64, NPB_N(h), &h->task, h->n_plants, h->ep_index, (hipStream_t)stream);
    done = h->task.done; reward = h->task.reward;
  }
  if (h->cs.cols)      /* the end-of-step state of the episode this step belonged to, before any restore */
    h->A->column_stats_fold(h->f64, NPB_N(h), &h->cs, h->n_plants, (hipStream_t)stream);
  if (h->ew.cols)      /* the same sample into every plant's ring, the triggers, the windows that are due -- or cut short by an episode that ends here */
    h->A->event_windows(h->f64, NPB_N(h), &h->ew, h->n_plants, h->ew_step++, h->ep_index, h->autoreset ? h->ep_len : nullptr, done,
                        h->max_episode_steps, (hipStream_t)stream);
  const double *recorded_reward = reward;
  if (h->norm.streams) {      /* the running statistics take this step's samples and rewrite ref and scale in the features' table, in front of pass A */
    if (h->norm_training) {
      h->A->normalizer(h->f64, NPB_N(h), &h->norm, h->n_plants, h->ep_index, reward, (hipStream_t)stream);
      npb_launch_normalizer_finish(&h->norm, (h->n_plants + 255) / 256, (hipStream_t)stream);
    }
    if (h->norm.reward_on) {      /* the reward the learner sees; everything that deals with episodes keeps the raw one */
      npb_launch_normalizer_reward(&h->norm, h->n_plants, h->ep_index, reward, done, !h->norm_training, (hipStream_t)stream);
      recorded_reward = h->norm.norm_reward;
    }
  }
  if (h->feat.cols)      /* pass A: this step's frame into every plant's stack, while everything still describes the episode it belongs to */
    h->A->features(h->f64, NPB_N(h), &h->feat, h->n_plants, 0, h->ep_index, (hipStream_t)stream);
  if (h->ro.n_final) {      /* the rollout's slot t: reward, outcome and the truncated plants' stacks, terminal frame included, while the carried length is the old one */
    npb_launch_rollout_post(&h->ro, h->feat.out, recorded_reward, done, h->autoreset ? h->ep_len : nullptr, h->autoreset ? h->ep_index : nullptr,
                            h->max_episode_steps, h->n_plants, (hipStream_t)stream);
    if (h->core.primed && h->core.final)      /* the truncated plants' hidden state beside their terminal stacks: the h' of this step, in the rows the post kernel handed out */
      npb_launch_policy_core_final(&h->core, h->ro.D.final_row + (size_t)h->ro.t * (size_t)h->n_plants, h->n_plants, (hipStream_t)stream);
    h->ro.t++;
  }
  if (h->er_on && h->autoreset)      /* the episodes that end on this step, recorded while everything still describes them; then their summary rows cleared */
    h->A->episode_records(h->n_plants, NPB_N(h), h->f64, done, reward, obs, trip_flags, counters_of(h), h->ep_start,
                          h->max_episode_steps, h->er_step++, &h->er, er_uses_summary(h) ? &h->summary : nullptr,
                          (h->ers_on || h->ert_on) ? h->ers_dev : nullptr, (hipStream_t)stream);
  if (h->autoreset)   /* same stream, nothing read back, the maintenance cache kept per plant by the kernel itself */
    h->K->episode(h->params.mode, h->n_plants, NPB_N(h), h->f64, source_of(h, from_bank), done, reward, obs, counters_of(h),
                  h->ep_out_len, h->ep_out_ret, h->ep_out_truncated, h->ep_final_obs, h->max_episode_steps,
                  maint ? h->maint_side : nullptr, maint ? h->maint_counts : nullptr, side, (hipStream_t)stream);
  if (h->autoreset) restart_streams(h, from_bank, (hipStream_t)stream, &es_take);      /* the plants the episode kernel has just restarted */
  if (h->feat.cols && h->autoreset)      /* pass B: their stacks into `final`, then the fresh frame of the restored state */
    h->A->features(h->f64, NPB_N(h), &h->feat, h->n_plants, 1, h->ep_index, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, NPB_EHIP, "npb_step: kernel launch failed", e);
  return NPB_OK;
}

int npb_snapshot(NpbHandle *h, void *stream) {
  if (!h) return NPB_EINVAL;
  NPB_USE_DEVICE(h);
  const size_t bytes = arena_columns(h->storage) * arena_plants(h) * h->real_bytes;
  if (!h->snap) {
    hipError_t e = hipMalloc(&h->snap, bytes);
    if (e != hipSuccess) { h->snap = nullptr; return fail(h, NPB_EHIP, "npb_snapshot: hipMalloc of the snapshot arena failed", e); }
  }
  NPB_HIP(h, hipMemcpyAsync(h->snap, h->f64, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  for (int b = 0; b < NPB_SIDE_COUNT; b++)      /* the side blocks belong to the episode start too */
    if (int rc = side_record(h, b, false, h, (hipStream_t)stream)) return rc;
  return NPB_OK;
}

/* npb_restore / npb_restore_bank: the plants of mask from the snapshot or from their bank entries, the side blocks with them */
static int restore_from(NpbHandle *h, bool bank, const uint8_t *mask, hipStream_t stream) {
  npb_side_restores_t side;
  if (const int b = side_restores_of(h, bank, false, &side); b >= 0) return fail(h, NPB_EINVAL, side_refusal(b, bank));
  NPB_USE_DEVICE(h);
  const bool maint = h->params.maint_enabled != 0;
  h->K->restore(h->n_plants, NPB_N(h), h->f64, source_of(h, bank), mask, counters_of(h),
                maint ? h->maint_side : nullptr, maint ? h->maint_counts : nullptr, side, stream);
  if (!bank) clear_episodes(h, mask, false, stream);     /* the restored episodes are not from the bank */
  restart_streams(h, bank, stream);
  core_restart(h, mask, stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}

int npb_restore(NpbHandle *h, const uint8_t *mask, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->snap) return fail(h, NPB_EINVAL, "npb_restore: no snapshot (npb_snapshot) to restore from");
  return restore_from(h, false, mask, (hipStream_t)stream);
}

int npb_set_autoreset(NpbHandle *h, int enabled, int max_episode_steps) {
  if (!h) return NPB_EINVAL;
  if (!enabled) {
    if (h->es_on) return fail(h, NPB_EINVAL, "npb_set_autoreset: episode streams are on (npb_set_episode_streams) and read the restarts off the autoreset's episode index; switch the mode off first");
    if (h->er_on) return fail(h, NPB_EINVAL, "npb_set_autoreset: episode records are on (npb_set_episode_records) and record the episodes the autoreset ends; switch the records off first");
    h->autoreset = false; return NPB_OK;
  }
  if (max_episode_steps < 0) return fail(h, NPB_EINVAL, "npb_set_autoreset: max_episode_steps must be >= 0 (0 = no limit)");
  if (!h->snap && !(h->bank && h->next_slot))
    return fail(h, NPB_EINVAL, "npb_set_autoreset: no snapshot (npb_snapshot), nor a start bank with slots (npb_set_start_bank, npb_set_start_slots), to reset to");
  if (h->diag && !h->diag_carry)
    return fail(h, NPB_EINVAL, "npb_set_autoreset: diagnostics are on (npb_set_diagnostics); their buffer carries plant state the snapshot does not hold");
  /* The source the autoreset will restore from must hold the diagnostics rows: that is refused here, at once and in this function's
   * own two texts.  A source without the component maintenance's state is refused only by the next npb_step (side_restores_of).  Both
   * are as callers know them: not to be evened out */
  if (h->diag_carry) {
    const bool bank = h->bank && h->next_slot;
    if (!(bank ? h->side[NPB_SIDE_DIAG].bank : h->side[NPB_SIDE_DIAG].snap).rows)
      return fail(h, NPB_EINVAL, bank ? "npb_set_autoreset: diagnostics are on and their rows carried (npb_carry_diagnostics), but the start bank was set without "
                                        "them: npb_set_start_bank again, from a handle that carries them"
                                      : "npb_set_autoreset: diagnostics are on and their rows carried (npb_carry_diagnostics), but the snapshot was taken "
                                        "without them: npb_snapshot again");
  }
  NPB_USE_DEVICE(h);
  if (!h->ep_len) {     /* one allocation: [pitch] int32 lengths, then [pitch] double returns, then [pitch] int32 episode indices */
    const size_t len_bytes = (h->pitch * sizeof(int32_t) + 255) / 256 * 256;
    hipError_t e = hipMalloc((void **)&h->ep_len, len_bytes + h->pitch * sizeof(double) + h->pitch * sizeof(int32_t));
    if (e != hipSuccess) { h->ep_len = nullptr; return fail(h, NPB_EHIP, "npb_set_autoreset: hipMalloc of the episode counters failed", e); }
    h->ep_ret = (double *)((char *)h->ep_len + len_bytes);
    h->ep_index = (int32_t *)(h->ep_ret + h->pitch);
  }
  const size_t len_bytes = (size_t)((char *)h->ep_ret - (char *)h->ep_len);
  NPB_HIP(h, hipMemset(h->ep_len, 0, len_bytes + h->pitch * sizeof(double) + h->pitch * sizeof(int32_t)));
  if (h->es_on) NPB_HIP(h, hipMemset(h->es.seen_index, 0, h->pitch * sizeof(int32_t)));      /* zeroing the indices restarts nothing */
  h->autoreset = true;
  h->max_episode_steps = max_episode_steps;
  return NPB_OK;
}

int npb_set_episode_buffers(NpbHandle *h, int32_t *length, double *ret, uint8_t *truncated, double *final_obs) {
  if (!h) return NPB_EINVAL;
  h->ep_out_len = length; h->ep_out_ret = ret; h->ep_out_truncated = truncated; h->ep_final_obs = final_obs;
  return NPB_OK;
}

int npb_set_episode_index_buffer(NpbHandle *h, int32_t *index) {
  if (!h) return NPB_EINVAL;
  h->ep_out_index = index;
  return NPB_OK;
}

int npb_set_start_bank(NpbHandle *h, const NpbHandle *src, void *stream) {
  if (!h) return NPB_EINVAL;
  if (h->es_on && h->es_tables && (!src || src->n_plants != h->es.bank_entries))
    return fail(h, NPB_EINVAL, "npb_set_start_bank: episode streams are on with bank seed tables (npb_set_episode_streams) of the present bank's entry count; "
                               "switch the mode off first, then set it again with tables for the new bank");
  NPB_USE_DEVICE(h);
  if (!src) {
    if (h->autoreset && !h->snap)
      return fail(h, NPB_EINVAL, "npb_set_start_bank: autoreset is on and restores from the bank; without it there is no snapshot (npb_snapshot) to fall back on");
    if (h->bank) (void)hipFree(h->bank);
    if (h->ep_start) (void)hipFree(h->ep_start);
    h->bank = nullptr; h->bank_bytes = 0; h->bank_N = 0; h->bank_M = 0; h->ep_start = nullptr;
    for (auto &sd : h->side) side_free(&sd.bank);
    return NPB_OK;
  }
  for (int b = NPB_SIDE_COUNT - 1; b >= 0; b--)      /* the bank's entries would come without the block's rows; the last block is reported first */
    if (g_side[b].on(h) && !g_side[b].on(src)) return fail(h, NPB_EINVAL, g_side[b].bank_lacks);
  if (src->storage != h->storage)
    return fail(h, NPB_EINVAL, "npb_set_start_bank: the bank handle's storage type differs from this handle's (npb_create_storage)");
  if (src->device != h->device)
    return fail(h, NPB_EINVAL, "npb_set_start_bank: the bank handle lives on another device");
  const size_t bytes = arena_columns(src->storage) * arena_plants(src) * src->real_bytes;
  if (!h->ep_start) {       /* a bank after none: no running episode started from it */
    hipError_t e = hipMalloc((void **)&h->ep_start, h->pitch * sizeof(int32_t));
    if (e != hipSuccess) { h->ep_start = nullptr; return fail(h, NPB_EHIP, "npb_set_start_bank: hipMalloc of the start entries failed", e); }
    NPB_HIP(h, hipMemsetAsync(h->ep_start, 0xff, h->pitch * sizeof(int32_t), (hipStream_t)stream));
  }
  if (bytes > h->bank_bytes) {
    if (h->bank) (void)hipFree(h->bank);
    h->bank = nullptr; h->bank_bytes = 0; h->bank_M = 0;
    hipError_t e = hipMalloc(&h->bank, bytes);
    if (e != hipSuccess) { h->bank = nullptr; return fail(h, NPB_EHIP, "npb_set_start_bank: hipMalloc of the bank arena failed", e); }
    h->bank_bytes = bytes;
  }
  NPB_HIP(h, hipMemcpyAsync(h->bank, src->f64, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  h->bank_N = NPB_N(src); h->bank_M = src->n_plants;
  for (int b = 0; b < NPB_SIDE_COUNT; b++)      /* the bank handle's side blocks beside its arena, in its pitch */
    if (int rc = side_record(h, b, true, src, (hipStream_t)stream)) return rc;
  return NPB_OK;
}

int npb_set_start_slots(NpbHandle *h, int32_t *next_slot, int32_t *episode_start, int advance) {
  if (!h) return NPB_EINVAL;
  if (!next_slot) return fail(h, NPB_EINVAL, "npb_set_start_slots: next_slot must not be NULL");
  if (advance < 0) return fail(h, NPB_EINVAL, "npb_set_start_slots: advance must be >= 0");
  h->next_slot = next_slot; h->slot_start = episode_start; h->slot_advance = advance;
  return NPB_OK;
}

int npb_restore_bank(NpbHandle *h, const uint8_t *mask, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->bank || !h->next_slot) return fail(h, NPB_EINVAL, "npb_restore_bank: no start bank (npb_set_start_bank) with slots (npb_set_start_slots) to restore from");
  return restore_from(h, true, mask, (hipStream_t)stream);
}

int npb_set_episode_start_buffer(NpbHandle *h, int32_t *out_start) {
  if (!h) return NPB_EINVAL;
  h->ep_out_start = out_start;
  return NPB_OK;
}

/* ---- the Mersenne-Twister generators (npb_noise_t: the heat-source noise's and the power profile's), between the device's [624][pitch]
 * key columns and numpy's get_state() layout, [n][624]; `who` = the ABI entry, for the messages */
static int seeds_narrow(NpbHandle *h, const char *who, const int64_t *seeds, uint32_t *s32) {
  for (int p = 0; p < h->n_plants; p++) {
    if (seeds[p] < 0 || seeds[p] > (int64_t)0xffffffffLL) return fail_who(h, who, ": a seed is outside [0, 2^32), which numpy.random.RandomState refuses");
    s32[p] = (uint32_t)seeds[p];
  }
  return NPB_OK;
}
static int mt_state_check(NpbHandle *h, const char *who, const int32_t *pos, const int32_t *has_gauss) {
  for (int p = 0; p < h->n_plants; p++) {
    if (pos[p] < 0 || pos[p] > NPB_MT_N) return fail_who(h, who, ": pos outside [0, 624]");
    if (has_gauss[p] != 0 && has_gauss[p] != 1) return fail_who(h, who, ": has_gauss outside {0, 1}");
  }
  return NPB_OK;
}
/* both wait for the stream: the staging rows and the caller's buffers are in use until the copies are done */
static int mt_state_download(NpbHandle *h, const npb_noise_t &g, uint32_t *key, int32_t *pos, int32_t *has_gauss, double *cached, hipStream_t st) {
  const size_t n = (size_t)h->n_plants;
  std::vector<uint32_t> rows((size_t)NPB_MT_N * n);
  NPB_HIP(h, hipMemcpy2DAsync(rows.data(), n * sizeof(uint32_t), g.key, h->pitch * sizeof(uint32_t), n * sizeof(uint32_t), NPB_MT_N, hipMemcpyDeviceToHost, st));
  NPB_HIP(h, hipMemcpyAsync(pos, g.pos, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  NPB_HIP(h, hipMemcpyAsync(has_gauss, g.has_gauss, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  NPB_HIP(h, hipMemcpyAsync(cached, g.gauss, n * sizeof(double), hipMemcpyDeviceToHost, st));
  NPB_HIP(h, hipStreamSynchronize(st));
  for (size_t i = 0; i < (size_t)NPB_MT_N; i++)
    for (size_t p = 0; p < n; p++) key[p * NPB_MT_N + i] = rows[i * n + p];
  return NPB_OK;
}
static int mt_state_upload(NpbHandle *h, const npb_noise_t &g, const uint32_t *key, const int32_t *pos, const int32_t *has_gauss, const double *cached, hipStream_t st) {
  const size_t n = (size_t)h->n_plants;
  std::vector<uint32_t> rows((size_t)NPB_MT_N * n);
  for (size_t i = 0; i < (size_t)NPB_MT_N; i++)
    for (size_t p = 0; p < n; p++) rows[i * n + p] = key[p * NPB_MT_N + i];
  NPB_HIP(h, hipMemcpy2DAsync(g.key, h->pitch * sizeof(uint32_t), rows.data(), n * sizeof(uint32_t), n * sizeof(uint32_t), NPB_MT_N, hipMemcpyHostToDevice, st));
  NPB_HIP(h, hipMemcpyAsync(g.pos, pos, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  NPB_HIP(h, hipMemcpyAsync(g.has_gauss, has_gauss, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  NPB_HIP(h, hipMemcpyAsync(g.gauss, cached, n * sizeof(double), hipMemcpyHostToDevice, st));
  NPB_HIP(h, hipStreamSynchronize(st));
  return NPB_OK;
}

static int noise_alloc(NpbHandle *h, const char *who) {
  if (h->noise) return NPB_OK;
  hipError_t e = hipMalloc(&h->noise, npb_noise_bytes(h->pitch));
  if (e != hipSuccess) { h->noise = nullptr; return fail(h, NPB_EHIP, (std::string(who) + ": hipMalloc of the noise generators failed").c_str(), e); }
  h->noise_g = npb_noise_layout(h->noise, h->pitch);
  return NPB_OK;
}

int npb_noise_seed(NpbHandle *h, const int64_t *seeds, void *stream) {
  if (!h) return NPB_EINVAL;
  if (h->es_on) return fail_who(h, "npb_noise_seed", g_es_owns);
  NPB_USE_DEVICE(h);
  if (!seeds) {
    if (h->noise) { NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream)); (void)hipFree(h->noise); }
    h->noise = nullptr; h->noise_seeds.clear();
    return NPB_OK;
  }
  const int n = h->n_plants;
  std::vector<uint32_t> s32((size_t)n);
  if (int rc = seeds_narrow(h, "npb_noise_seed", seeds, s32.data())) return rc;
  if (int rc = noise_alloc(h, "npb_noise_seed")) return rc;
  /* the seeds travel in the pos column, which the seed kernel then overwrites */
  NPB_HIP(h, hipMemcpyAsync(h->noise_g.pos, s32.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, (hipStream_t)stream));
  npb_launch_noise_seed(h->noise_g, n, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream));    /* s32 is read until the copy is done */
  h->noise_seeds = std::move(s32);
  return NPB_OK;
}

int npb_noise_fill(NpbHandle *h, int k, double *out, void *stream) {
  if (!h) return NPB_EINVAL;
  if (h->es_on) return fail_who(h, "npb_noise_fill", g_es_owns);
  if (!h->noise) return fail(h, NPB_EINVAL, "npb_noise_fill: no noise generators (npb_noise_seed or npb_noise_set_state first)");
  if (k < 1 || !out) return fail(h, NPB_EINVAL, "npb_noise_fill: k must be >= 1 and out non-NULL");
  NPB_USE_DEVICE(h);
  npb_launch_noise_fill(h->noise_g, h->n_plants, k, out, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, NPB_EHIP, "npb_noise_fill: kernel launch failed", e);
  return NPB_OK;
}

int npb_noise_get_state(NpbHandle *h, uint32_t *key, int32_t *pos, int32_t *has_gauss, double *cached, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->noise) return fail(h, NPB_EINVAL, "npb_noise_get_state: no noise generators (npb_noise_seed or npb_noise_set_state first)");
  if (!key || !pos || !has_gauss || !cached) return fail(h, NPB_EINVAL, "npb_noise_get_state: NULL output");
  NPB_USE_DEVICE(h);
  return mt_state_download(h, h->noise_g, key, pos, has_gauss, cached, (hipStream_t)stream);
}

int npb_noise_set_state(NpbHandle *h, const uint32_t *key, const int32_t *pos, const int32_t *has_gauss, const double *cached, void *stream) {
  if (!h) return NPB_EINVAL;
  if (h->es_on) return fail_who(h, "npb_noise_set_state", g_es_owns);
  if (!key || !pos || !has_gauss || !cached) return fail(h, NPB_EINVAL, "npb_noise_set_state: NULL input");
  if (int rc = mt_state_check(h, "npb_noise_set_state", pos, has_gauss)) return rc;
  NPB_USE_DEVICE(h);
  if (int rc = noise_alloc(h, "npb_noise_set_state")) return rc;
  return mt_state_upload(h, h->noise_g, key, pos, has_gauss, cached, (hipStream_t)stream);
}

/* ---- the data-gen runner's power profile (include/npb.h) */
static void profile_free(NpbHandle *h) {
  if (h->prof) (void)hipFree(h->prof);
  if (h->prof_side) (void)hipFree(h->prof_side);
  if (h->prof_z) (void)hipFree(h->prof_z);
  h->prof = nullptr; h->prof_side = nullptr; h->prof_z = nullptr; h->prof_z_rows = 0; h->prof_steps = 0; h->prof_pos = 0;
  h->prof_seeds.clear();
}

int npb_profile_seed(NpbHandle *h, const int64_t *seeds, int steps, const double *base, int n_base, const double *std, int n_std, void *stream) {
  if (!h) return NPB_EINVAL;
  if (h->es_on) return fail_who(h, "npb_profile_seed", g_es_owns);
  NPB_USE_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  if (!seeds) {
    if (h->prof) NPB_HIP(h, hipStreamSynchronize(st));
    profile_free(h);
    return NPB_OK;
  }
  const int n = h->n_plants;
  if (steps < 1) return fail(h, NPB_EINVAL, "npb_profile_seed: steps must be >= 1");
  if ((base && n_base != 1 && n_base != n) || (std && n_std != 1 && n_std != n))
    return fail(h, NPB_EINVAL, "npb_profile_seed: base and std are each NULL, one value or one value per plant");
  std::vector<uint32_t> s32((size_t)n);
  if (int rc = seeds_narrow(h, "npb_profile_seed", seeds, s32.data())) return rc;
  const size_t pitch = h->pitch;
  if (!h->prof) {
    hipError_t e = hipMalloc(&h->prof, npb_noise_bytes(pitch));
    if (e == hipSuccess) e = hipMalloc((void **)&h->prof_side, (size_t)NPB_PROFILE_SIDE * pitch * sizeof(double));
    if (e != hipSuccess) { profile_free(h); return fail(h, NPB_EHIP, "npb_profile_seed: hipMalloc of the profile generators failed", e); }
    h->prof_g = npb_noise_layout(h->prof, pitch);
  }
  /* the load profile's two columns, the runner's cap on the noise taken here; the carried rows start at 0 (position 0 reads none) */
  std::vector<double> side((size_t)NPB_PROFILE_SIDE * pitch, 0.0);
  for (int p = 0; p < n; p++) {
    const double b = base ? base[n_base == 1 ? 0 : p] : 90.0, sd = std ? std[n_std == 1 ? 0 : p] : 2.0;
    side[(size_t)NPB_PROFILE_BASE * pitch + p] = b;
    side[(size_t)NPB_PROFILE_SCALE * pitch + p] = sd < 0.2 ? sd : 0.2;      /* min(0.2, std), a NaN std -> 0.2 as Python's min has it */
  }
  NPB_HIP(h, hipMemcpyAsync(h->prof_side, side.data(), side.size() * sizeof(double), hipMemcpyHostToDevice, st));
  NPB_HIP(h, hipMemcpyAsync(h->prof_g.pos, s32.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  npb_launch_noise_seed(h->prof_g, n, st);
  NPB_HIP(h, hipGetLastError());
  NPB_HIP(h, hipStreamSynchronize(st));    /* side and s32 are read until the copies are done */
  h->prof_steps = steps; h->prof_pos = 0;
  h->prof_seeds = std::move(s32);
  return NPB_OK;
}

int npb_profile_fill(NpbHandle *h, int k, double *setpoint_out, double *target_out, double *z_out, void *stream) {
  if (!h) return NPB_EINVAL;
  if (h->es_on) return fail_who(h, "npb_profile_fill", g_es_owns);
  if (!h->prof) return fail(h, NPB_EINVAL, "npb_profile_fill: no profile (npb_profile_seed first)");
  if (k < 1 || !setpoint_out) return fail(h, NPB_EINVAL, "npb_profile_fill: k must be >= 1 and setpoint_out non-NULL");
  NPB_USE_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  const int n = h->n_plants, draws = npb_profile_draws(h->prof_steps, h->prof_pos, k);
  if ((size_t)draws > h->prof_z_rows) {      /* the draw block grows to the largest block asked for (at most k + 1 rows) */
    NPB_HIP(h, hipStreamSynchronize(st));
    if (h->prof_z) (void)hipFree(h->prof_z);
    h->prof_z = nullptr; h->prof_z_rows = 0;
    hipError_t e = hipMalloc((void **)&h->prof_z, (size_t)draws * n * sizeof(double));
    if (e != hipSuccess) { h->prof_z = nullptr; return fail(h, NPB_EHIP, "npb_profile_fill: hipMalloc of the draw block failed", e); }
    h->prof_z_rows = (size_t)draws;
  }
  if (draws > 0) npb_launch_noise_fill(h->prof_g, n, draws, h->prof_z, st);
  npb_launch_profile_rows(n, k, h->prof_steps, h->prof_pos, h->prof_side, h->pitch, h->prof_z, setpoint_out, target_out, z_out, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, NPB_EHIP, "npb_profile_fill: kernel launch failed", e);
  h->prof_pos = (int)(((long long)h->prof_pos + k) % h->prof_steps);
  return NPB_OK;
}

int npb_profile_ramp(NpbHandle *h, int k, const double *target_in, double *setpoint_out, void *stream) {
  if (!h) return NPB_EINVAL;
  const bool forget = k == 0 && !target_in && !setpoint_out;
  if (!forget && (k < 1 || !target_in || !setpoint_out)) return fail(h, NPB_EINVAL, "npb_profile_ramp: k must be >= 1 and both blocks non-NULL (or 0, NULL, NULL: forget the carried setpoints)");
  NPB_USE_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  if (!h->ramp_prev || forget) {
    if (!h->ramp_prev) {
      hipError_t e = hipMalloc((void **)&h->ramp_prev, h->pitch * sizeof(double));
      if (e != hipSuccess) { h->ramp_prev = nullptr; return fail(h, NPB_EHIP, "npb_profile_ramp: hipMalloc failed", e); }
    }
    npb_launch_profile_set(h->ramp_prev, h->pitch, __builtin_nan(""), st);
  }
  if (!forget) npb_launch_profile_ramp(h->n_plants, k, target_in, setpoint_out, h->ramp_prev, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, NPB_EHIP, "npb_profile_ramp: kernel launch failed", e);
  return NPB_OK;
}

int npb_profile_get_state(NpbHandle *h, uint32_t *key, int32_t *pos, int32_t *has_gauss, double *cached, double *carried, int32_t *position, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->prof) return fail(h, NPB_EINVAL, "npb_profile_get_state: no profile (npb_profile_seed first)");
  if (!key || !pos || !has_gauss || !cached || !carried || !position) return fail(h, NPB_EINVAL, "npb_profile_get_state: NULL output");
  NPB_USE_DEVICE(h);
  const size_t n = (size_t)h->n_plants, pitch = h->pitch;
  hipStream_t st = (hipStream_t)stream;
  NPB_HIP(h, hipMemcpy2DAsync(carried, n * sizeof(double), h->prof_side + (size_t)NPB_PROFILE_CARRIED * pitch, pitch * sizeof(double), n * sizeof(double),
                              NPB_PROFILE_NUM_CARRIED, hipMemcpyDeviceToHost, st));
  if (int rc = mt_state_download(h, h->prof_g, key, pos, has_gauss, cached, st)) return rc;      /* (waits for the stream) */
  *position = h->es_on ? -1 : h->prof_pos;      /* episode streams: every plant has its own (npb_profile_get_positions) */
  return NPB_OK;
}

int npb_profile_set_state(NpbHandle *h, const uint32_t *key, const int32_t *pos, const int32_t *has_gauss, const double *cached, const double *carried,
                          int32_t position, void *stream) {
  if (!h) return NPB_EINVAL;
  if (h->es_on) return fail_who(h, "npb_profile_set_state", g_es_owns);
  if (!h->prof) return fail(h, NPB_EINVAL, "npb_profile_set_state: no profile (npb_profile_seed first: it sets the horizon and the load profiles)");
  if (!key || !pos || !has_gauss || !cached || !carried) return fail(h, NPB_EINVAL, "npb_profile_set_state: NULL input");
  if (position < 0 || position >= h->prof_steps) return fail(h, NPB_EINVAL, "npb_profile_set_state: position outside [0, steps)");
  if (int rc = mt_state_check(h, "npb_profile_set_state", pos, has_gauss)) return rc;
  NPB_USE_DEVICE(h);
  const size_t n = (size_t)h->n_plants, pitch = h->pitch;
  hipStream_t st = (hipStream_t)stream;
  NPB_HIP(h, hipMemcpy2DAsync(h->prof_side + (size_t)NPB_PROFILE_CARRIED * pitch, pitch * sizeof(double), carried, n * sizeof(double), n * sizeof(double),
                              NPB_PROFILE_NUM_CARRIED, hipMemcpyHostToDevice, st));
  if (int rc = mt_state_upload(h, h->prof_g, key, pos, has_gauss, cached, st)) return rc;      /* (waits for the stream) */
  h->prof_pos = position;
  return NPB_OK;
}

/* ---- episode records (include/npb.h) */
const char *npb_episode_records_check(const npb_episode_records_desc_t *D, int has_autoreset, int summary_keys) {
  if (!D) return nullptr;
  if (!has_autoreset) return "npb_set_episode_records: no autoreset (npb_set_autoreset first): the records are of the episodes it ends";
  if (D->capacity < 1) return "npb_set_episode_records: capacity must be >= 1";
  if (!D->plant || !D->episode || !D->start || !D->length || !D->flags || !D->trip_flags || !D->step || !D->ret || !D->end_time || !D->cursor)
    return "npb_set_episode_records: the columns plant, episode, start, length, flags, trip_flags, step, ret, end_time and the cursor must not be NULL";
  if (((uintptr_t)D->plant & 3u) || ((uintptr_t)D->episode & 3u) || ((uintptr_t)D->start & 3u) || ((uintptr_t)D->length & 3u) || ((uintptr_t)D->flags & 3u) ||
      ((uintptr_t)D->trip_flags & 3u) || ((uintptr_t)D->step & 3u) || ((uintptr_t)D->cursor & 3u) || ((uintptr_t)D->ret & 7u) || ((uintptr_t)D->end_time & 7u) ||
      ((uintptr_t)D->final_obs & 7u) || ((uintptr_t)D->first_created & 7u) || ((uintptr_t)D->first_completed & 7u) || ((uintptr_t)D->n_created & 3u) ||
      ((uintptr_t)D->n_completed & 3u))
    return "npb_set_episode_records: the double columns must be 8-byte, the int32 columns and the cursor 4-byte aligned";
  const int tables = (D->first_created != nullptr) + (D->first_completed != nullptr) + (D->n_created != nullptr) + (D->n_completed != nullptr);
  if (tables != 0 && tables != 4) return "npb_set_episode_records: only part of the four summary tables given (first_created, first_completed, n_created, n_completed): all or none";
  if (tables && summary_keys <= 0) return "npb_set_episode_records: summary columns without a work-order summary set (npb_set_maintenance_summary first)";
  if (D->clear_summary && summary_keys <= 0) return "npb_set_episode_records: clear_summary without a work-order summary set (npb_set_maintenance_summary first)";
  return nullptr;
}
int npb_set_episode_records(NpbHandle *h, const npb_episode_records_desc_t *desc) {
  if (!h) return NPB_EINVAL;
  if (!desc) { h->er_on = false; h->ers_on = false; h->ert_on = false; return NPB_OK; }      /* (the record-side statistics and cause column go with the records) */
  if (const char *why = npb_episode_records_check(desc, h->autoreset ? 1 : 0, h->summary_on ? h->summary.n_keys : 0)) return fail(h, NPB_EINVAL, why);
  /* new record columns, perhaps of another capacity: the record-side statistics columns belonged to the old ones and are dropped with
   * them (npb_set_episode_record_stats again, behind this call, for the new ones) */
  h->er = *desc; h->er_step = 0; h->er_on = true; h->ers_on = false; h->ert_on = false;      /* (the cause column too: npb_set_episode_record_task again) */
  return NPB_OK;
}

/* ---- event windows (include/npb.h, npd_event_windows.h) */
const char *npb_event_windows_check(const npb_event_windows_desc_t *D, int n_plants, int has_autoreset) {
  (void)has_autoreset;
  if (!D) return nullptr;
  if (n_plants < 1) return "npb_set_event_windows: n_plants must be >= 1";
  if (D->n_fields < 0 || D->n_sources < 0 || (int64_t)D->n_fields + D->n_sources < 1 || (int64_t)D->n_fields + D->n_sources > NPB_EVENT_WINDOW_COLS_MAX)
    return "npb_set_event_windows: the column count (n_fields + n_sources) must be 1 .. NPB_EVENT_WINDOW_COLS_MAX (16)";
  if (D->n_triggers < 1 || D->n_triggers > NPB_EVENT_WINDOW_TRIGGERS_MAX || !D->triggers)
    return "npb_set_event_windows: the trigger count must be 1 .. NPB_EVENT_WINDOW_TRIGGERS_MAX (8), with their descriptors";
  if (D->pre < 0 || D->post < 0 || (int64_t)D->pre + 1 + D->post > NPB_EVENT_WINDOW_ROWS_MAX)
    return "npb_set_event_windows: the window shape needs pre >= 0, post >= 0 and pre + 1 + post <= NPB_EVENT_WINDOW_ROWS_MAX (1024)";
  if (D->capacity < 1) return "npb_set_event_windows: capacity must be >= 1";
  if ((D->n_fields > 0 && (!D->kinds || !D->slots)) || (D->n_sources > 0 && !D->sources))
    return "npb_set_event_windows: fields without kinds / slots, or side sources without their descriptors";
  for (int c = 0; c < D->n_fields + D->n_sources; c++)
    if (const char *why = column_refusal(g_ew_column, column_of(D, c), nullptr)) return why;
  for (int t = 0; t < D->n_triggers; t++) {
    const npb_event_trigger_t &T = D->triggers[t];
    bool integer = false;
    if (const char *why = column_refusal(g_ew_column, column_of(T), &integer)) return why;
    if (T.mode == NPB_TRIGGER_MODE_BITS_RISE) {
      if (!integer) return "npb_set_event_windows: NPB_TRIGGER_BITS_RISE on a real-valued column (it needs an int32 member, or an I32 or U8 source)";
      if (T.mask == 0u) return "npb_set_event_windows: NPB_TRIGGER_BITS_RISE with mask 0";
    } else if (T.mode == NPB_TRIGGER_MODE_BEYOND) {
      if (T.direction != 1 && T.direction != -1) return "npb_set_event_windows: NPB_TRIGGER_BEYOND with a direction outside {-1, +1}";
      if (T.limit != T.limit) return "npb_set_event_windows: NPB_TRIGGER_BEYOND with a NaN limit";
    } else if (T.mode != NPB_TRIGGER_MODE_INCREASE) {
      return "npb_set_event_windows: an unknown trigger mode";
    }
  }
  const void *words[] = {D->plant, D->episode, D->trigger, D->step, D->n_pre, D->n_post, D->flags, D->retriggers, D->fired, D->cursor};
  for (const void *w : words) {
    if (!w) return "npb_set_event_windows: a NULL record column or cursor";
    if ((uintptr_t)w & 3u) return "npb_set_event_windows: a misaligned record column: the double columns must be 8-byte, the others and the cursor 4-byte aligned";
  }
  const void *doubles[] = {D->time, D->times, D->values};
  for (const void *w : doubles) {
    if (!w) return "npb_set_event_windows: a NULL record column or cursor";
    if ((uintptr_t)w & 7u) return "npb_set_event_windows: a misaligned record column: the double columns must be 8-byte, the others and the cursor 4-byte aligned";
  }
  return nullptr;
}
/* the allocation: [the columns][the triggers] | ring | prev | a_time | the eight 4-byte words per plant; every part 8-byte aligned */
static size_t ew_table_bytes() {
  return NPB_EVENT_WINDOW_COLS_MAX * sizeof(npb_colstat_col_t) + NPB_EVENT_WINDOW_TRIGGERS_MAX * sizeof(npb_event_trigger_col_t);
}
size_t npb_event_windows_bytes(const npb_event_windows_desc_t *D, int n_plants) {
  if (!D || npb_event_windows_check(D, n_plants, 0)) return 0;
  const size_t n = (size_t)n_plants, H = (size_t)D->pre + 1 + (size_t)D->post, n_cols = (size_t)D->n_fields + (size_t)D->n_sources;
  const size_t words = (8 * n * sizeof(int32_t) + 7) / 8 * 8;
  return ew_table_bytes() + (H * (n_cols + 1) + (size_t)D->n_triggers + 1) * n * sizeof(double) + words;
}
int npb_set_event_windows(NpbHandle *h, const npb_event_windows_desc_t *desc) {
  if (!h) return NPB_EINVAL;
  if (const char *why = npb_event_windows_check(desc, h->n_plants, h->autoreset ? 1 : 0)) return fail(h, NPB_EINVAL, why);
  NPB_USE_DEVICE(h);
  if (!desc) { attachment_drop(&h->ew, h->ew.cols); h->ew_bytes = 0; return NPB_OK; }
  struct { npb_colstat_col_t cols[NPB_EVENT_WINDOW_COLS_MAX]; npb_event_trigger_col_t triggers[NPB_EVENT_WINDOW_TRIGGERS_MAX]; } table = {};
  static_assert(sizeof table == NPB_EVENT_WINDOW_COLS_MAX * sizeof(npb_colstat_col_t) + NPB_EVENT_WINDOW_TRIGGERS_MAX * sizeof(npb_event_trigger_col_t), "packed");
  const int n_cols = desc->n_fields + desc->n_sources;
  for (int c = 0; c < n_cols; c++)
    if (!column_build(h, column_of(desc, c), &table.cols[c])) return fail(h, NPB_EINVAL, g_ew_column[COLUMN_BAD_FIELD]);
  for (int t = 0; t < desc->n_triggers; t++) {
    const npb_event_trigger_t &T = desc->triggers[t];
    npb_event_trigger_col_t &O = table.triggers[t];
    if (!column_build(h, column_of(T), &O.c)) return fail(h, NPB_EINVAL, g_ew_column[COLUMN_BAD_FIELD]);
    O.mode = T.mode; O.mask = T.mask;
    if (T.mode == NPB_TRIGGER_MODE_BEYOND) { O.c.direction = T.direction; O.c.limit = T.limit; }
  }
  const size_t bytes = npb_event_windows_bytes(desc, h->n_plants), n = (size_t)h->n_plants, H = (size_t)desc->pre + 1 + (size_t)desc->post;
  /* the tables up, everything else zero (the indices last seen too: a first sample that finds another index empties an empty ring) */
  char *dev = nullptr;
  if (int rc = attachment_alloc(h, "npb_set_event_windows", "the ring and the bookkeeping", &table, sizeof table, bytes, &dev)) return rc;
  npb_event_windows_t W = {};
  W.cols = (const npb_colstat_col_t *)dev; W.triggers = (const npb_event_trigger_col_t *)(dev + sizeof table.cols);
  W.n_cols = n_cols; W.n_triggers = desc->n_triggers; W.pre = desc->pre; W.post = desc->post;
  W.ring = (double *)(dev + sizeof table);
  W.prev = W.ring + H * (size_t)(n_cols + 1) * n;
  W.a_time = W.prev + (size_t)desc->n_triggers * n;
  int32_t *words = (int32_t *)(W.a_time + n);
  W.valid = words; W.due = words + n; W.seen = words + 2 * n; W.a_step = words + 3 * n; W.a_n_pre = words + 4 * n; W.a_trigger = words + 5 * n;
  W.a_retriggers = words + 6 * n; W.a_fired = (uint32_t *)(words + 7 * n);
  W.D = npb_event_window_records_t{desc->capacity, desc->plant, desc->episode, desc->trigger, desc->step, desc->n_pre, desc->n_post, desc->flags,
                                   desc->retriggers, desc->fired, desc->time, desc->times, desc->values, desc->cursor};
  /* every plant unprimed and idle (idle is not zero: due = -1) before the first step can read it */
  npb_launch_event_windows_clear(&W, nullptr, h->n_plants, nullptr);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) { (void)hipFree(dev); return fail(h, NPB_EHIP, "npb_set_event_windows: setting up the ring and the bookkeeping failed", e); }
  attachment_drop(&h->ew, h->ew.cols);
  h->ew = W; h->ew_bytes = bytes; h->ew_step = 0;
  return NPB_OK;
}
int npb_event_windows_clear(NpbHandle *h, const uint8_t *mask, void *stream) {
  if (!h) return NPB_EINVAL;
  return attachment_clear(h, "npb_event_windows_clear", h->ew.cols, g_no_event_windows,
                          [&] { npb_launch_event_windows_clear(&h->ew, mask, h->n_plants, (hipStream_t)stream); });
}

/* ---- column statistics (include/npb.h, npd_column_stats.h) */
const char *npb_column_stats_check(const npb_column_stats_desc_t *D, int n_plants) {
  if (!D) return nullptr;
  if (n_plants < 1) return "npb_set_column_stats: n_plants must be >= 1";
  if (D->n_fields < 0 || D->n_sources < 0 || (int64_t)D->n_fields + D->n_sources < 1 || (int64_t)D->n_fields + D->n_sources > NPB_COLUMN_STATS_MAX)
    return "npb_set_column_stats: the column count (n_fields + n_sources) must be 1 .. NPB_COLUMN_STATS_MAX (32)";
  if ((D->n_fields > 0 && (!D->kinds || !D->slots)) || (D->n_sources > 0 && !D->sources))
    return "npb_set_column_stats: fields without kinds / slots, or side sources without their descriptors";
  const int n_cols = D->n_fields + D->n_sources;
  for (int c = 0; c < n_cols; c++)
    if (const char *why = column_refusal(g_cs_column, column_of(D, c), nullptr)) return why;
  bool limited = false;
  for (int c = 0; D->direction && c < n_cols; c++) {
    if (D->direction[c] < -1 || D->direction[c] > 1) return "npb_set_column_stats: a direction outside {-1, 0, +1}";
    if (D->direction[c] != 0) {
      if (!D->limit || D->limit[c] != D->limit[c]) return "npb_set_column_stats: a NaN limit (or a direction without the limit array)";
      limited = true;
    }
  }
  if (!D->n_samples) return "npb_set_column_stats: n_samples must not be NULL";
  if (stat_tables_misaligned(D)) return "npb_set_column_stats: a misaligned table: the double tables must be 8-byte, the int32 tables 4-byte aligned";
  if ((D->first_beyond || D->n_beyond) && !limited) return "npb_set_column_stats: limit tables (first_beyond, n_beyond) without a limit on any column";
  return nullptr;
}
int npb_set_column_stats(NpbHandle *h, const npb_column_stats_desc_t *desc) {
  if (!h) return NPB_EINVAL;
  if (h->ers_on)
    return fail(h, NPB_EINVAL, "npb_set_column_stats: episode records that copy or clear the column statistics are on (npb_set_episode_record_stats) and hold its tables and column count; switch them off first");
  if (const char *why = npb_column_stats_check(desc, h->n_plants)) return fail(h, NPB_EINVAL, why);
  NPB_USE_DEVICE(h);
  if (!desc) { attachment_drop(&h->cs, h->cs.cols); return NPB_OK; }
  const int n_cols = desc->n_fields + desc->n_sources;
  npb_colstat_col_t cols[NPB_COLUMN_STATS_MAX] = {};
  for (int c = 0; c < n_cols; c++) {
    npb_colstat_col_t &C = cols[c];
    if (!column_build(h, column_of(desc, c), &C)) return fail(h, NPB_EINVAL, g_cs_column[COLUMN_BAD_FIELD]);
    C.direction = desc->direction ? desc->direction[c] : 0;
    C.limit = C.direction ? desc->limit[c] : 0.0;
  }
  char *dev = nullptr;
  if (int rc = attachment_alloc(h, "npb_set_column_stats", "the column table", cols, sizeof cols, sizeof cols, &dev, NPB_ENOMEM)) return rc;
  attachment_drop(&h->cs, h->cs.cols);
  h->cs = npb_column_stats_t{(const npb_colstat_col_t *)dev, n_cols, desc->min, desc->max, desc->sum, desc->sumsq, desc->last, desc->first_beyond,
                             desc->n_beyond, desc->n_samples};
  return NPB_OK;
}
int npb_column_stats_fold(NpbHandle *h, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->cs.cols) return fail(h, NPB_EINVAL, "npb_column_stats_fold: no column statistics set (npb_set_column_stats first)");
  NPB_USE_DEVICE(h);
  h->A->column_stats_fold(h->f64, NPB_N(h), &h->cs, h->n_plants, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
int npb_column_stats_clear(NpbHandle *h, const uint8_t *mask, void *stream) {
  if (!h) return NPB_EINVAL;
  return attachment_clear(h, "npb_column_stats_clear", h->cs.cols, g_no_column_stats,
                          [&] { npb_launch_column_stats_clear(&h->cs, mask, h->n_plants, (hipStream_t)stream); });
}
/* what the records kernel reads beside its own descriptor -- the column statistics with their record-side columns, the task's cause column
 * with its own -- into the handle's device copy (allocated on first use); synchronous: a records kernel in flight has finished */
static int upload_record_side(NpbHandle *h, const char *who, const npb_episode_record_stats_desc_t *rs, int32_t *cause) {
  if (!h->ers_dev) {
    hipError_t e = hipMalloc((void **)&h->ers_dev, sizeof(npb_record_stats_t));
    if (e != hipSuccess) { h->ers_dev = nullptr; return fail(h, NPB_ENOMEM, (std::string(who) + ": hipMalloc of the device copy failed").c_str(), e); }
  }
  npb_record_stats_t host = {};
  if (rs) { host.st = h->cs; host.rs = *rs; }
  if (cause) { host.task_cause = h->task.cause; host.cause = cause; }
  NPB_HIP(h, hipMemcpy(h->ers_dev, &host, sizeof host, hipMemcpyHostToDevice));
  return NPB_OK;
}
int npb_set_episode_record_stats(NpbHandle *h, const npb_episode_record_stats_desc_t *D) {
  if (!h) return NPB_EINVAL;
  if (!D) {
    if (h->ers_on && h->ert_on) {      /* the cause column stays: the device copy without the statistics */
      NPB_USE_DEVICE(h);
      if (int rc = upload_record_side(h, "npb_set_episode_record_stats", nullptr, h->ert_cause)) return rc;
    }
    h->ers_on = false;
    return NPB_OK;
  }
  if (!h->er_on) return fail(h, NPB_EINVAL, "npb_set_episode_record_stats: no episode records (npb_set_episode_records first)");
  if (!h->cs.cols) return fail(h, NPB_EINVAL, "npb_set_episode_record_stats: no column statistics set (npb_set_column_stats first)");
  if (stat_tables_misaligned(D)) return fail(h, NPB_EINVAL, "npb_set_episode_record_stats: the double columns must be 8-byte, the int32 columns 4-byte aligned");
  if ((D->min && !h->cs.min) || (D->max && !h->cs.max) || (D->sum && !h->cs.sum) || (D->sumsq && !h->cs.sumsq) || (D->last && !h->cs.last) ||
      (D->first_beyond && !h->cs.first_beyond) || (D->n_beyond && !h->cs.n_beyond))
    return fail(h, NPB_EINVAL, "npb_set_episode_record_stats: a record-side column for a statistic the handle does not keep (its table in npb_set_column_stats is NULL)");
  NPB_USE_DEVICE(h);
  if (int rc = upload_record_side(h, "npb_set_episode_record_stats", D, h->ert_on ? h->ert_cause : nullptr)) return rc;
  h->ers = *D; h->ers_on = true;
  return NPB_OK;
}

/* ---- tasks (include/npb.h, npd_task.h) */
const char *npb_task_check(const npb_task_desc_t *D, int n_plants) {
  if (!D) return nullptr;
  if (n_plants < 1) return "npb_set_task: n_plants must be >= 1";
  if (D->n_terms < 0 || D->n_terms > NPB_TASK_TERMS_MAX || (D->n_terms > 0 && !D->terms))
    return "npb_set_task: the term count must be 0 .. NPB_TASK_TERMS_MAX (16), with their descriptors";
  if (D->n_rules < 0 || D->n_rules > NPB_TASK_RULES_MAX || (D->n_rules > 0 && !D->rules))
    return "npb_set_task: the rule count must be 0 .. NPB_TASK_RULES_MAX (8), with their descriptors";
  if (D->n_terms + D->n_rules == 0) return "npb_set_task: a task with neither reward terms nor termination rules";
  if (D->bias != D->bias) return "npb_set_task: a NaN bias";
  for (int t = 0; t < D->n_terms; t++) {
    const npb_task_term_t &T = D->terms[t];
    bool integer = false;
    if (const char *why = column_refusal(g_task_column, column_of(T.column), &integer)) return why;
    if (T.kind < NPB_TASK_VALUE || T.kind > NPB_TASK_DELTA) return "npb_set_task: an unknown term kind";
    if (T.weight != T.weight) return "npb_set_task: a NaN weight";
    if (T.kind == NPB_TASK_ABS_ERR || T.kind == NPB_TASK_SQ_ERR) {
      if (T.ref_from_column) { if (const char *why = column_refusal(g_task_column, column_of(T.ref_column), nullptr)) return why; }
      else if (T.ref != T.ref) return "npb_set_task: a NaN ref";
    } else if (T.kind == NPB_TASK_BEYOND || T.kind == NPB_TASK_EXCESS) {
      if (T.direction != 1 && T.direction != -1) return "npb_set_task: a BEYOND or EXCESS term with a direction outside {-1, +1}";
      if (T.limit != T.limit) return "npb_set_task: a NaN limit";
    } else if (T.kind == NPB_TASK_BITS) {
      if (!integer) return "npb_set_task: NPB_TASK_BITS on a real-valued column (it needs an int32 member, or an I32 or U8 source)";
      if (T.mask == 0u) return "npb_set_task: NPB_TASK_BITS with mask 0";
    }
  }
  for (int r = 0; r < D->n_rules; r++) {
    const npb_task_rule_t &R = D->rules[r];
    bool integer = false;
    if (const char *why = column_refusal(g_task_column, column_of(R.column), &integer)) return why;
    if (R.terminal_reward != R.terminal_reward) return "npb_set_task: a NaN terminal reward";
    if (R.mode == NPB_TASK_RULE_MODE_BITS_ANY) {
      if (!integer) return "npb_set_task: NPB_TASK_RULE_BITS_ANY on a real-valued column (it needs an int32 member, or an I32 or U8 source)";
      if (R.mask == 0u) return "npb_set_task: NPB_TASK_RULE_BITS_ANY with mask 0";
    } else if (R.mode == NPB_TASK_RULE_MODE_BEYOND) {
      if (R.direction != 1 && R.direction != -1) return "npb_set_task: NPB_TASK_RULE_BEYOND with a direction outside {-1, +1}";
      if (R.limit != R.limit) return "npb_set_task: a NaN limit";
    } else if (R.mode != NPB_TASK_RULE_MODE_NONFINITE) {
      return "npb_set_task: an unknown rule mode";
    }
  }
  if (!D->reward || !D->done) return "npb_set_task: a NULL output: the reward and done columns are mandatory";
  if (((uintptr_t)D->reward & 7u) || ((uintptr_t)D->terms_out & 7u) || ((uintptr_t)D->cause & 3u))
    return "npb_set_task: a misaligned output: the double columns must be 8-byte, the cause column 4-byte aligned";
  return nullptr;
}
int npb_set_task(NpbHandle *h, const npb_task_desc_t *desc) {
  if (!h) return NPB_EINVAL;
  if (h->ert_on)
    return fail(h, NPB_EINVAL, "npb_set_task: episode records that copy the task's cause word are on (npb_set_episode_record_task) and hold its cause column; drop that first");
  if (h->task.terms && h->norm.streams && h->norm.reward_on)
    return fail(h, NPB_EINVAL, "npb_set_task: a normaliser is set (npb_set_normalizer) whose return stream reads the task's reward; npb_set_normalizer(h, NULL) first");
  if (const char *why = npb_task_check(desc, h->n_plants)) return fail(h, NPB_EINVAL, why);
  NPB_USE_DEVICE(h);
  if (!desc) { attachment_drop(&h->task, h->task.terms); return NPB_OK; }
  /* the allocation: [the terms][the rules] | prev [n_delta][n] | primed [n] | seen [n]; every part 8-byte aligned */
  struct { npb_task_term_col_t terms[NPB_TASK_TERMS_MAX]; npb_task_rule_col_t rules[NPB_TASK_RULES_MAX]; } table = {};
  static_assert(sizeof table == NPB_TASK_TERMS_MAX * sizeof(npb_task_term_col_t) + NPB_TASK_RULES_MAX * sizeof(npb_task_rule_col_t) && sizeof table % 8 == 0, "packed");
  int n_delta = 0;
  for (int t = 0; t < desc->n_terms; t++) {
    const npb_task_term_t &T = desc->terms[t];
    npb_task_term_col_t &O = table.terms[t];
    if (!column_build(h, column_of(T.column), &O.c)) return fail(h, NPB_EINVAL, g_task_column[COLUMN_BAD_FIELD]);
    O.w = T.weight; O.kind = T.kind; O.prev_row = -1;
    if (T.kind == NPB_TASK_ABS_ERR || T.kind == NPB_TASK_SQ_ERR) {
      if (T.ref_from_column) { O.ref_col = 1; if (!column_build(h, column_of(T.ref_column), &O.r)) return fail(h, NPB_EINVAL, g_task_column[COLUMN_BAD_FIELD]); }
      else O.ref = T.ref;
    } else if (T.kind == NPB_TASK_BEYOND || T.kind == NPB_TASK_EXCESS) { O.c.direction = T.direction; O.c.limit = T.limit; }
    else if (T.kind == NPB_TASK_BITS) O.mask = T.mask;
    else if (T.kind == NPB_TASK_DELTA) O.prev_row = n_delta++;
  }
  for (int r = 0; r < desc->n_rules; r++) {
    const npb_task_rule_t &R = desc->rules[r];
    npb_task_rule_col_t &O = table.rules[r];
    if (!column_build(h, column_of(R.column), &O.c)) return fail(h, NPB_EINVAL, g_task_column[COLUMN_BAD_FIELD]);
    O.terminal = R.terminal_reward; O.mode = R.mode; O.mask = R.mask;
    if (R.mode == NPB_TASK_RULE_MODE_BEYOND) { O.c.direction = R.direction; O.c.limit = R.limit; }
  }
  const size_t n = (size_t)h->n_plants, words = (2 * n * sizeof(int32_t) + 7) / 8 * 8;
  const size_t bytes = sizeof table + (size_t)n_delta * n * sizeof(double) + words;
  /* the tables up, everything else zero: every plant unprimed (the indices last seen too: a first sample that finds another index
   * unprimes an unprimed plant) */
  char *dev = nullptr;
  if (int rc = attachment_alloc(h, "npb_set_task", "the tables and the previous samples", &table, sizeof table, bytes, &dev)) return rc;
  npb_task_t T = {};
  T.terms = (const npb_task_term_col_t *)dev; T.rules = (const npb_task_rule_col_t *)(dev + sizeof table.terms);
  T.n_terms = desc->n_terms; T.n_rules = desc->n_rules; T.n_delta = n_delta; T.bias = desc->bias;
  T.reward = desc->reward; T.done = desc->done; T.cause = desc->cause; T.terms_out = desc->terms_out;
  T.prev = (double *)(dev + sizeof table);
  T.primed = (int32_t *)(T.prev + (size_t)n_delta * n); T.seen = T.primed + n;
  attachment_drop(&h->task, h->task.terms);
  h->task = T;
  return NPB_OK;
}
int npb_task_clear(NpbHandle *h, const uint8_t *mask, void *stream) {
  if (!h) return NPB_EINVAL;
  return attachment_clear(h, "npb_task_clear", h->task.terms, g_no_task, [&] { npb_launch_unprime(h->task.primed, mask, h->n_plants, (hipStream_t)stream); });
}
/* prev, primed, seen; without DELTA terms there is no prev */
static StateParts task_state_parts(const NpbHandle *h) {
  const size_t n = (size_t)h->n_plants;
  return {h->task.terms, g_no_task, " (prev may be NULL only for a task without DELTA terms)", 3,
          {{h->task.prev, (size_t)h->task.n_delta * n * sizeof(double), h->task.n_delta == 0}, {h->task.primed, n * sizeof(int32_t), false},
           {h->task.seen, n * sizeof(int32_t), false}}};
}
int npb_task_get_state(NpbHandle *h, double *prev, int32_t *primed, int32_t *seen, void *stream) {
  return state_copy(h, "npb_task_get_state", task_state_parts, {prev, primed, seen}, false, stream);
}
int npb_task_set_state(NpbHandle *h, const double *prev, const int32_t *primed, const int32_t *seen, void *stream) {
  return state_copy(h, "npb_task_set_state", task_state_parts, {prev, primed, seen}, true, stream);
}
int npb_set_episode_record_task(NpbHandle *h, int32_t *cause) {
  if (!h) return NPB_EINVAL;
  if (!cause) {
    if (h->ert_on && h->ers_on) {      /* the statistics stay: the device copy without the cause column */
      NPB_USE_DEVICE(h);
      if (int rc = upload_record_side(h, "npb_set_episode_record_task", &h->ers, nullptr)) return rc;
    }
    h->ert_on = false; h->ert_cause = nullptr;
    return NPB_OK;
  }
  if (!h->er_on) return fail(h, NPB_EINVAL, "npb_set_episode_record_task: no episode records (npb_set_episode_records first)");
  if (!h->task.terms) return fail(h, NPB_EINVAL, "npb_set_episode_record_task: no task set (npb_set_task first)");
  if (!h->task.cause) return fail(h, NPB_EINVAL, "npb_set_episode_record_task: the task keeps no cause column (its cause output in npb_set_task is NULL)");
  if ((uintptr_t)cause & 3u) return fail(h, NPB_EINVAL, "npb_set_episode_record_task: the cause column must be 4-byte aligned");
  NPB_USE_DEVICE(h);
  if (int rc = upload_record_side(h, "npb_set_episode_record_task", h->ers_on ? &h->ers : nullptr, cause)) return rc;
  h->ert_on = true; h->ert_cause = cause;
  return NPB_OK;
}

/* ---- features (include/npb.h, npd_features.h) */
const char *npb_features_check(const npb_features_desc_t *D, int n_plants) {
  if (!D) return nullptr;
  if (n_plants < 1) return "npb_set_features: n_plants must be >= 1";
  if (D->n_columns < 1 || D->n_columns > NPB_FEATURES_COLS_MAX || !D->columns)
    return "npb_set_features: the column count must be 1 .. NPB_FEATURES_COLS_MAX (64), with their descriptors";
  if (D->stack < 1 || D->stack > NPB_FEATURES_STACK_MAX) return "npb_set_features: the stack depth must be 1 .. NPB_FEATURES_STACK_MAX (16)";
  if (D->stack * D->n_columns > NPB_FEATURES_CELLS_MAX) return "npb_set_features: stack * columns must be <= NPB_FEATURES_CELLS_MAX (256)";
  for (int c = 0; c < D->n_columns; c++) {
    const npb_feature_column_t &F = D->columns[c];
    bool integer = false;
    if (const char *why = column_refusal(g_feat_column, column_of(F.column), &integer)) return why;
    if (F.kind == NPB_FEATURE_KIND_AFFINE) {
      if (F.scale != F.scale) return "npb_set_features: a NaN scale";
      if (F.ref != F.ref) return "npb_set_features: a NaN ref";
      if (F.ref_from_column) { if (const char *why = column_refusal(g_feat_column, column_of(F.ref_column), nullptr)) return why; }
    } else if (F.kind == NPB_FEATURE_KIND_BITS) {
      if (!integer) return "npb_set_features: NPB_FEATURE_BITS on a real-valued column (it needs an int32 member, or an I32 or U8 source)";
      if (F.mask == 0u) return "npb_set_features: NPB_FEATURE_BITS with mask 0";
    } else {
      return "npb_set_features: an unknown feature kind";
    }
    if (F.lo != F.lo || F.hi != F.hi) return "npb_set_features: a NaN clip limit (lo, hi)";
    if (F.lo > F.hi) return "npb_set_features: a clip with lo > hi";
    if (F.fresh != F.fresh) return "npb_set_features: a NaN fresh value";
  }
  if (D->out_type != NPB_FEATURES_F32 && D->out_type != NPB_FEATURES_F64) return "npb_set_features: an unknown out type";
  if (!D->out) return "npb_set_features: a NULL out tensor";
  const uintptr_t low = D->out_type == NPB_FEATURES_F64 ? 7u : 3u;
  if (((uintptr_t)D->out & low) || ((uintptr_t)D->final & low))
    return "npb_set_features: a misaligned tensor: out and final must be 4-byte aligned for float, 8-byte for double";
  return nullptr;
}
int npb_set_features(NpbHandle *h, const npb_features_desc_t *desc) {
  if (!h) return NPB_EINVAL;
  if (h->pol.theta) return fail_who(h, "npb_set_features", g_policy_holds);
  if (h->ro.n_final) return fail_who(h, "npb_set_features", g_rollout_holds);
  if (h->norm.streams && h->norm.n_cols)
    return fail(h, NPB_EINVAL, "npb_set_features: a normaliser with columns is set (npb_set_normalizer) and rewrites this table every step; npb_set_normalizer(h, NULL) first");
  if (const char *why = npb_features_check(desc, h->n_plants)) return fail(h, NPB_EINVAL, why);
  NPB_USE_DEVICE(h);
  if (!desc) { attachment_drop(&h->feat, h->feat.cols); h->feat_host.clear(); return NPB_OK; }
  /* the allocation: [the columns] | primed [n] | seen [n] */
  std::vector<npb_feature_col_t> table(NPB_FEATURES_COLS_MAX);
  for (int c = 0; c < desc->n_columns; c++) {
    const npb_feature_column_t &F = desc->columns[c];
    npb_feature_col_t &O = table[c];
    O = npb_feature_col_t{};
    if (!column_build(h, column_of(F.column), &O.c)) return fail(h, NPB_EINVAL, g_feat_column[COLUMN_BAD_FIELD]);
    O.kind = F.kind; O.mask = F.mask; O.scale = F.scale; O.ref = F.ref; O.lo = F.lo; O.hi = F.hi; O.nan_to = F.nan_to; O.fresh = F.fresh;
    if (F.nan_to != F.nan_to) { const uint64_t quiet = 0x7ff8000000000000ull; memcpy(&O.nan_to, &quiet, sizeof quiet); }      /* the NaN that stays: sign clear, no payload */
    O.live = (!F.column.from_source || F.fresh_live) ? 1 : 0;
    if (F.kind == NPB_FEATURE_KIND_AFFINE && F.ref_from_column) {
      O.ref_col = 1;
      if (!column_build(h, column_of(F.ref_column), &O.r)) return fail(h, NPB_EINVAL, g_feat_column[COLUMN_BAD_FIELD]);
      if (!F.ref_column.from_source || F.ref_fresh_live) O.live |= 2;
    }
  }
  const size_t n = (size_t)h->n_plants, table_bytes = table.size() * sizeof(npb_feature_col_t), bytes = table_bytes + 2 * n * sizeof(int32_t);
  static_assert(sizeof(npb_feature_col_t) % 8 == 0, "packed");
  /* the columns up, everything else zero: every plant unprimed */
  char *dev = nullptr;
  if (int rc = attachment_alloc(h, "npb_set_features", "the columns and the bookkeeping", table.data(), table_bytes, bytes, &dev)) return rc;
  npb_features_t F = {};
  F.cols = (const npb_feature_col_t *)dev; F.n_cols = desc->n_columns; F.stack = desc->stack; F.out_f64 = desc->out_type == NPB_FEATURES_F64;
  F.out = desc->out; F.final = desc->final;
  F.primed = (int32_t *)(dev + table_bytes); F.seen = F.primed + n;
  attachment_drop(&h->feat, h->feat.cols);
  h->feat = F;
  h->feat_host = table;
  return NPB_OK;
}
int npb_features_prime(NpbHandle *h, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->feat.cols) return fail(h, NPB_EINVAL, "npb_features_prime: no features set (npb_set_features first)");
  NPB_USE_DEVICE(h);
  h->A->features(h->f64, NPB_N(h), &h->feat, h->n_plants, 2, h->ep_index, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
int npb_features_clear(NpbHandle *h, const uint8_t *mask, void *stream) {
  if (!h) return NPB_EINVAL;
  return attachment_clear(h, "npb_features_clear", h->feat.cols, g_no_features,
                          [&] { npb_launch_unprime(h->feat.primed, mask, h->n_plants, (hipStream_t)stream); });
}
/* primed, seen (the stack is the caller's tensor) */
static StateParts features_state_parts(const NpbHandle *h) {
  const size_t words = (size_t)h->n_plants * sizeof(int32_t);
  return {h->feat.cols, g_no_features, "", 2, {{h->feat.primed, words, false}, {h->feat.seen, words, false}}};
}
int npb_features_get_state(NpbHandle *h, int32_t *primed, int32_t *seen, void *stream) {
  return state_copy(h, "npb_features_get_state", features_state_parts, {primed, seen}, false, stream);
}
int npb_features_set_state(NpbHandle *h, const int32_t *primed, const int32_t *seen, void *stream) {
  return state_copy(h, "npb_features_set_state", features_state_parts, {primed, seen}, true, stream);
}

/* ---- controls (include/npb.h, npd_controls.h) */
static bool is_finite(double x) { return x - x == 0.0; }
const char *npb_controls_check(const npb_controls_desc_t *D, int n_plants, int heat_source) {
  if (!D) return nullptr;
  if (n_plants < 1) return "npb_set_controls: n_plants must be >= 1";
  if (D->n_axes < 1 || D->n_axes > NPB_CONTROLS_AXES_MAX || !D->axes)
    return "npb_set_controls: the axis count must be 1 .. NPB_CONTROLS_AXES_MAX (8), with their descriptors";
  if (D->interval < 1 || D->interval > NPB_CONTROLS_INTERVAL_MAX) return "npb_set_controls: the interval must be 1 .. NPB_CONTROLS_INTERVAL_MAX (64)";
  bool actuator[NPB_ACTUATOR_COUNT] = {}, input[NPB_CONTROL_INPUT_COUNT] = {};
  for (int a = 0; a < D->n_axes; a++) {
    const npb_control_axis_t &X = D->axes[a];
    if (X.kind == NPB_CONTROL_KIND_RATE || X.kind == NPB_CONTROL_KIND_TARGET) {
      if (X.target < 0 || X.target >= NPB_ACTUATOR_COUNT) return "npb_set_controls: an unknown actuator";
      if (actuator[X.target]) return "npb_set_controls: two axes on one actuator";
      actuator[X.target] = true;
    } else if (X.kind == NPB_CONTROL_KIND_COLUMN) {
      if (X.target < 0 || X.target >= NPB_CONTROL_INPUT_COUNT) return "npb_set_controls: an unknown input";
      if (input[X.target]) return "npb_set_controls: two axes on one input";
      input[X.target] = true;
    } else if (X.kind != NPB_CONTROL_KIND_VALUE) {
      return "npb_set_controls: an unknown control kind";
    }
    if (!is_finite(X.scale) || !is_finite(X.offset) || !is_finite(X.nan_to) || !is_finite(X.deadband) || !is_finite(X.max_magnitude))
      return "npb_set_controls: a NaN or infinite scale, offset, nan_to, deadband or max_magnitude";
    if (X.deadband < 0.0) return "npb_set_controls: a negative deadband";
    if (X.max_magnitude < 0.0) return "npb_set_controls: a negative max_magnitude";
    if (X.lo != X.lo || X.hi != X.hi) return "npb_set_controls: a NaN clip limit (lo, hi)";
    if (X.lo > X.hi) return "npb_set_controls: a clip with lo > hi";
  }
  if (D->in_type != NPB_CONTROLS_F32 && D->in_type != NPB_CONTROLS_F64) return "npb_set_controls: an unknown input type";
  if (!D->in) return "npb_set_controls: a NULL in tensor";
  if ((uintptr_t)D->in & (D->in_type == NPB_CONTROLS_F64 ? 7u : 3u))
    return "npb_set_controls: a misaligned in tensor: 4-byte aligned for float, 8-byte for double";
  if (!D->held || !D->prev) return "npb_set_controls: NULL held or prev";
  if (((uintptr_t)D->held | (uintptr_t)D->prev) & 7u) return "npb_set_controls: misaligned held or prev: 8-byte aligned";
  if (input[NPB_CONTROL_INPUT_POWER_SETPOINT] && heat_source == NPB_HEAT_EXTERNAL)
    return "npb_set_controls: a POWER_SETPOINT axis under NPB_HEAT_EXTERNAL, where the power_setpoint column carries the plugin's power";
  return nullptr;
}
int npb_set_controls(NpbHandle *h, const npb_controls_desc_t *desc) {
  if (!h) return NPB_EINVAL;
  if (h->pol.theta) return fail_who(h, "npb_set_controls", g_policy_holds);
  if (h->ro.n_final) return fail_who(h, "npb_set_controls", g_rollout_holds);
  if (const char *why = npb_controls_check(desc, h->n_plants, h->params.heat_source)) return fail(h, NPB_EINVAL, why);
  NPB_USE_DEVICE(h);
  if (!desc) { attachment_drop(&h->ord, h->ord.since); attachment_drop(&h->ctl, h->ctl.age); return NPB_OK; }
  npb_controls_t C = {};
  int axis_of[NPB_CONTROL_INPUT_COUNT] = {-1, -1};
  for (int a = 0; a < desc->n_axes; a++) {
    C.axes[a] = desc->axes[a];
    if (desc->axes[a].kind == NPB_CONTROL_KIND_COLUMN) axis_of[desc->axes[a].target] = a;
  }
  if (axis_of[NPB_CONTROL_INPUT_POWER_SETPOINT] >= 0 && h->es_on && h->es.prof.key)
    return fail(h, NPB_EINVAL, "npb_set_controls: a POWER_SETPOINT axis while episode streams drive the profile (npb_set_episode_streams)");
  /* the allocation: age [n] | primed [n] | seen [n] (padded to 8 bytes) | the two input columns [n] each; no table, all zero: every
   * plant unprimed */
  const size_t n = (size_t)h->n_plants, words = (3 * n + 1) & ~(size_t)1, bytes = words * sizeof(int32_t) + NPB_CONTROL_INPUT_COUNT * n * sizeof(double);
  char *dev = nullptr;
  if (int rc = attachment_alloc(h, "npb_set_controls", "the bookkeeping and the input columns", nullptr, 0, bytes, &dev)) return rc;
  C.n_axes = desc->n_axes; C.interval = desc->interval; C.in_f64 = desc->in_type == NPB_CONTROLS_F64;
  C.in = desc->in; C.held = desc->held; C.prev = desc->prev;
  C.age = (int32_t *)dev; C.primed = C.age + n; C.seen = C.primed + n;
  for (int i = 0; i < NPB_CONTROL_INPUT_COUNT; i++) C.column[i] = (double *)(dev + words * sizeof(int32_t)) + (size_t)i * n;
  attachment_drop(&h->ord, h->ord.since);      /* the rules read the old axes' columns */
  attachment_drop(&h->ctl, h->ctl.age);
  h->ctl = C;
  for (int i = 0; i < NPB_CONTROL_INPUT_COUNT; i++) h->ctl_axis[i] = axis_of[i];
  return NPB_OK;
}
int npb_controls_clear(NpbHandle *h, const uint8_t *mask, void *stream) {
  if (!h) return NPB_EINVAL;
  return attachment_clear(h, "npb_controls_clear", h->ctl.age, g_no_controls,
                          [&] { npb_launch_unprime(h->ctl.primed, mask, h->n_plants, (hipStream_t)stream); });
}
/* held, prev (the caller's tensors, which the decode carries from step to step), age, primed, seen */
static StateParts controls_state_parts(const NpbHandle *h) {
  const size_t n = (size_t)h->n_plants, values = (size_t)h->ctl.n_axes * n * sizeof(double), words = n * sizeof(int32_t);
  return {h->ctl.age, g_no_controls, "", 5,
          {{h->ctl.held, values, false}, {h->ctl.prev, values, false}, {h->ctl.age, words, false}, {h->ctl.primed, words, false}, {h->ctl.seen, words, false}}};
}
int npb_controls_get_state(NpbHandle *h, double *held, double *prev, int32_t *age, int32_t *primed, int32_t *seen, void *stream) {
  return state_copy(h, "npb_controls_get_state", controls_state_parts, {held, prev, age, primed, seen}, false, stream);
}
int npb_controls_set_state(NpbHandle *h, const double *held, const double *prev, const int32_t *age, const int32_t *primed, const int32_t *seen,
                           void *stream) {
  return state_copy(h, "npb_controls_set_state", controls_state_parts, {held, prev, age, primed, seen}, true, stream);
}

/* ---- order rules on the controls' axes (include/npb.h, npd_control_orders.h) */
const char *npb_control_orders_check(const npb_control_orders_desc_t *D, const npb_controls_desc_t *C, int n_plants, int mode) {
  if (!D) return nullptr;
  if (n_plants < 1) return "npb_set_control_orders: n_plants must be >= 1";
  if (!C || C->n_axes < 1 || C->n_axes > NPB_CONTROLS_AXES_MAX || !C->axes) return "npb_set_control_orders: no controls set (npb_set_controls first)";
  if (D->n_orders < 1 || D->n_orders > NPB_CONTROL_ORDERS_MAX || !D->orders)
    return "npb_set_control_orders: the rule count must be 1 .. NPB_CONTROL_ORDERS_MAX (8), with their descriptors";
  for (int r = 0; r < D->n_orders; r++) {
    const npb_control_order_t &R = D->orders[r];
    if (R.axis < 0 || R.axis >= C->n_axes) return "npb_set_control_orders: a rule on an axis the controls do not have";
    if (C->axes[R.axis].kind != NPB_CONTROL_KIND_VALUE) return "npb_set_control_orders: a rule on an axis that is not NPB_CONTROL_VALUE";
    if (R.family == NPB_ORDER_PUMP) {
      if (R.action < 0 || R.action >= NPB_MAINT_NACT) return "npb_set_control_orders: a pump action outside the catalog (NPB_MA_*)";
      if (!g_maint_actions[R.action].handler) return "npb_set_control_orders: a pump action without a handler";
      if (R.unit < 0 || R.unit >= NPB_NUM_PUMPS) return "npb_set_control_orders: a feedwater pump that does not exist (0 .. 3)";
      if (R.action == NPB_MA_BEARING_REPLACEMENT && (R.option < NPB_BEARING_ALL || R.option > NPB_BEARING_THRUST))
        return "npb_set_control_orders: a bearing outside NPB_BEARING_ALL .. NPB_BEARING_THRUST";
    } else if (R.family == NPB_ORDER_COMPONENT) {
      if (R.action < 0 || R.action >= NPB_COMPONENT_NACT) return "npb_set_control_orders: a component action outside the catalog (NPB_CA_*)";
      const int kind = g_component_actions[R.action].kind;
      const bool ignored = kind == NPB_COMPONENT_SGSYS || kind == NPB_COMPONENT_COND;
      if (!ignored && (R.unit < 0 || R.unit >= NPB_COMPONENT_UNITS(kind))) return "npb_set_control_orders: a generator or ejector that does not exist";
      const bool sg_side = kind == NPB_COMPONENT_SG || kind == NPB_COMPONENT_SGSYS;
      if (!(mode == NPB_MODE_FULL || (mode == NPB_MODE_PRIMARY_SG && sg_side))) return "npb_set_control_orders: a component the mode does not step";
    } else if (R.family == NPB_ORDER_TURBINE) {
      if (R.action < 0 || R.action >= NPB_TURBINE_NACT) return "npb_set_control_orders: a turbine action outside the catalog (NPB_TA_*)";
      const int kind = g_turbine_actions[R.action].kind;
      const bool ignored = kind == NPB_TURBINE_SYSTEM || kind == NPB_TURBINE_LUBE;
      if (!ignored && (R.unit < 0 || R.unit >= NPB_TURBINE_UNITS(kind))) return "npb_set_control_orders: a turbine bearing or stage that does not exist";
      if (R.action == NPB_TA_BEARING_THRUST_BEARING_ADJUSTMENT && R.unit != NPB_TURBINE_THRUST_BEARING)
        return "npb_set_control_orders: a thrust adjustment on a journal bearing";
      if (mode != NPB_MODE_FULL) return "npb_set_control_orders: a turbine rule in a mode that steps no turbine";
    } else {
      return "npb_set_control_orders: an unknown family (NPB_ORDER_PUMP, _COMPONENT, _TURBINE)";
    }
    if (!is_finite(R.threshold) || !is_finite(R.amount)) return "npb_set_control_orders: a NaN or infinite threshold or amount";
    if (R.min_interval < 1) return "npb_set_control_orders: min_interval must be >= 1";
  }
  if (!D->fired) return "npb_set_control_orders: a NULL fired";
  if ((uintptr_t)D->fired & 7u) return "npb_set_control_orders: a misaligned fired: 8-byte aligned";
  return nullptr;
}
static const char *const g_no_control_orders = ": no order rules set (npb_set_control_orders first)";
int npb_set_control_orders(NpbHandle *h, const npb_control_orders_desc_t *desc) {
  if (!h) return NPB_EINVAL;
  if (h->pol.theta) return fail_who(h, "npb_set_control_orders", g_policy_holds);
  NPB_USE_DEVICE(h);
  if (!desc) { attachment_drop(&h->ord, h->ord.since); return NPB_OK; }
  if (!h->ctl.age) return fail_who(h, "npb_set_control_orders", g_no_controls);
  npb_controls_desc_t C = {};
  C.n_axes = h->ctl.n_axes; C.axes = h->ctl.axes;
  if (const char *why = npb_control_orders_check(desc, &C, h->n_plants, h->params.mode)) return fail(h, NPB_EINVAL, why);
  npb_control_orders_t O = {};
  for (int r = 0; r < desc->n_orders; r++) {
    npb_control_order_t R = desc->orders[r];      /* what the family's call ignores is 0 here, as its kernel makes it before it logs */
    if (R.family == NPB_ORDER_PUMP) { if (R.action != NPB_MA_BEARING_REPLACEMENT) R.option = 0; }
    else if (R.family == NPB_ORDER_COMPONENT) {
      const int kind = g_component_actions[R.action].kind;
      if (kind == NPB_COMPONENT_SGSYS || kind == NPB_COMPONENT_COND) R.unit = 0;
    } else {
      const int kind = g_turbine_actions[R.action].kind;
      if (kind == NPB_TURBINE_SYSTEM || kind == NPB_TURBINE_LUBE) R.unit = 0;
      R.option = 0;
    }
    O.rule[r] = R;
  }
  /* the allocation: since [n_orders][n], every cell NEVER */
  const size_t cells = (size_t)desc->n_orders * (size_t)h->n_plants;
  std::vector<int32_t> never(cells, NPB_CONTROL_ORDER_NEVER);
  char *dev = nullptr;
  if (int rc = attachment_alloc(h, "npb_set_control_orders", "the rules' since words", never.data(), cells * sizeof(int32_t), cells * sizeof(int32_t), &dev)) return rc;
  O.n_orders = desc->n_orders; O.interval = h->ctl.interval; O.held = h->ctl.held; O.age = h->ctl.age;
  O.fired = desc->fired; O.since = (int32_t *)dev;
  attachment_drop(&h->ord, h->ord.since);
  h->ord = O;
  return NPB_OK;
}
static StateParts control_orders_state_parts(const NpbHandle *h) {
  return {h->ord.since, g_no_control_orders, "", 1, {{h->ord.since, (size_t)h->ord.n_orders * (size_t)h->n_plants * sizeof(int32_t), false}}};
}
int npb_control_orders_get_state(NpbHandle *h, int32_t *since, void *stream) {
  return state_copy(h, "npb_control_orders_get_state", control_orders_state_parts, {since}, false, stream);
}
int npb_control_orders_set_state(NpbHandle *h, const int32_t *since, void *stream) {
  return state_copy(h, "npb_control_orders_set_state", control_orders_state_parts, {since}, true, stream);
}

/* ---- the rollout (include/npb.h, npd_rollout.h) */
const char *npb_rollout_check(const npb_rollout_desc_t *D, int n_plants, int features_cells, int n_axes) {
  if (!D) return nullptr;
  if (n_plants < 1) return "npb_set_rollout: n_plants must be >= 1";
  if (features_cells < 1) return "npb_set_rollout: the features' stack must have cells (K * C >= 1): a rollout needs features";
  if (D->horizon < 1 || D->horizon > NPB_ROLLOUT_HORIZON_MAX) return "npb_set_rollout: the horizon must be 1 .. NPB_ROLLOUT_HORIZON_MAX (4096)";
  if (D->n_extras < 0 || D->n_extras > NPB_ROLLOUT_EXTRAS_MAX) return "npb_set_rollout: the extras count must be 0 .. NPB_ROLLOUT_EXTRAS_MAX (8)";
  if (n_axes < 0) return "npb_set_rollout: a negative axis count";
  if (D->act && n_axes == 0) return "npb_set_rollout: an act buffer without axes (no controls are set)";
  if (!D->act && n_axes > 0) return "npb_set_rollout: controls are set and the act buffer is NULL";
  if (D->final_rows < 0) return "npb_set_rollout: final_rows must be >= 0";
  if ((int64_t)n_plants * D->final_rows > INT32_MAX) return "npb_set_rollout: n_plants * final_rows is beyond what final_row (int32) holds";
  if (D->final_rows > 0 && !D->final_obs) return "npb_set_rollout: final_rows > 0 and final_obs is NULL";
  if (!D->obs || !D->reward || !D->ended || !D->episode || !D->final_row) return "npb_set_rollout: NULL obs, reward, ended, episode or final_row";
  if (D->n_extras > 0 && (!D->extras_in || !D->extra)) return "npb_set_rollout: extras without their input (extras_in) or their buffer (extra)";
  if (((uintptr_t)D->obs | (uintptr_t)D->act | (uintptr_t)D->extras_in | (uintptr_t)D->extra | (uintptr_t)D->final_obs) & 15u)
    return "npb_set_rollout: misaligned obs, act, extras_in, extra or final_obs: 16-byte aligned";
  if ((uintptr_t)D->reward & 7u) return "npb_set_rollout: a misaligned reward buffer: 8-byte aligned";
  if (((uintptr_t)D->episode | (uintptr_t)D->final_row) & 3u) return "npb_set_rollout: misaligned episode or final_row: 4-byte aligned";
  return nullptr;
}
static int rollout_rewind(NpbHandle *h, npb_rollout_t *R, hipStream_t stream) {
  const size_t n = (size_t)h->n_plants;
  NPB_HIP(h, hipMemsetAsync(R->n_final, 0, n * sizeof(int32_t), stream));
  NPB_HIP(h, hipMemsetAsync(R->D.final_row, 0xff, (size_t)R->D.horizon * n * sizeof(int32_t), stream));      /* -1 */
  R->t = 0;
  return NPB_OK;
}
int npb_set_rollout(NpbHandle *h, const npb_rollout_desc_t *desc) {
  if (!h) return NPB_EINVAL;
  if (h->pol.theta) return fail_who(h, "npb_set_rollout", g_policy_holds);
  if (desc && !h->feat.cols) return fail(h, NPB_EINVAL, "npb_set_rollout: no features set (npb_set_features first): the rollout records their tensor");
  const int cells = h->feat.n_cols * h->feat.stack, n_axes = h->ctl.age ? h->ctl.n_axes : 0;
  if (const char *why = npb_rollout_check(desc, h->n_plants, cells, n_axes)) return fail(h, NPB_EINVAL, why);
  NPB_USE_DEVICE(h);
  if (!desc) { attachment_drop(&h->ro, h->ro.n_final); return NPB_OK; }
  char *dev = nullptr;
  if (int rc = attachment_alloc(h, "npb_set_rollout", "the final-row counters", nullptr, 0, (size_t)h->n_plants * sizeof(int32_t), &dev)) return rc;
  npb_rollout_t R = {};
  R.n_final = (int32_t *)dev; R.D = *desc; R.cells = cells; R.n_axes = n_axes;
  R.obs_bytes = h->feat.out_f64 ? 8 : 4; R.act_bytes = h->ctl.in_f64 ? 8 : 4;
  if (!R.D.final_obs) R.D.final_rows = 0;
  if (int rc = rollout_rewind(h, &R, nullptr)) { (void)hipFree(dev); return rc; }
  NPB_HIP(h, hipStreamSynchronize(nullptr));
  attachment_drop(&h->ro, h->ro.n_final);
  h->ro = R;
  return NPB_OK;
}
int npb_rollout_steps(const NpbHandle *h) { return h && h->ro.n_final ? h->ro.t : -1; }
int npb_rollout_begin(NpbHandle *h, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->ro.n_final) return fail_who(h, "npb_rollout_begin", g_no_rollout);
  NPB_USE_DEVICE(h);
  return rollout_rewind(h, &h->ro, (hipStream_t)stream);
}
int npb_rollout_cut(NpbHandle *h, const uint8_t *mask, void *stream) {
  if (!h) return NPB_EINVAL;
  if (h->ro.n_final && h->ro.t == 0) return NPB_OK;      /* nothing recorded yet: nothing in front of slot 0 */
  return attachment_clear(h, "npb_rollout_cut", h->ro.n_final, g_no_rollout,
                          [&] { npb_launch_rollout_cut(&h->ro, mask, h->n_plants, (hipStream_t)stream); });
}
int npb_rollout_advantages(NpbHandle *h, const npb_rollout_advantages_desc_t *A, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->ro.n_final) return fail_who(h, "npb_rollout_advantages", g_no_rollout);
  if (!A) return fail(h, NPB_EINVAL, "npb_rollout_advantages: a NULL descriptor");
  if (h->ro.t == 0) return fail(h, NPB_EINVAL, "npb_rollout_advantages: nothing recorded yet (t == 0)");
  if (!(A->gamma >= 0.0 && A->gamma <= 1.0) || !(A->lam >= 0.0 && A->lam <= 1.0))
    return fail(h, NPB_EINVAL, "npb_rollout_advantages: gamma and lam must lie in [0, 1] (a NaN does not)");
  if (!A->adv && !A->ret) return fail(h, NPB_EINVAL, "npb_rollout_advantages: adv and ret are both NULL");
  if (A->out_type != NPB_ROLLOUT_F32 && A->out_type != NPB_ROLLOUT_F64) return fail(h, NPB_EINVAL, "npb_rollout_advantages: an unknown out type");
  if (h->ro.D.final_rows > 0 && !A->final_value)
    return fail(h, NPB_EINVAL, "npb_rollout_advantages: the rollout keeps terminal stacks (final_rows > 0) and final_value, the caller's value of them, is NULL");
  NPB_USE_DEVICE(h);
  npb_launch_rollout_advantages(&h->ro, A, A->gamma * A->lam, h->n_plants, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}

/* ---- the policy (include/npb.h, npb_policy.hip) */
const char *npb_policy_check(const npb_policy_desc_t *D, int n_plants, int features_cells, int n_axes) {
  if (!D) return nullptr;
  if (n_plants < 1) return "npb_set_policy: n_plants must be >= 1";
  if (features_cells < 1 || features_cells > NPB_FEATURES_CELLS_MAX) return "npb_set_policy: the features' stack must have 1 .. NPB_FEATURES_CELLS_MAX (256) cells: a policy needs features";
  if (n_axes < 1 || n_axes > NPB_CONTROLS_AXES_MAX) return "npb_set_policy: the axis count must be 1 .. NPB_CONTROLS_AXES_MAX (8): a policy needs controls";
  if (D->actor_layers < 1 || D->actor_layers > NPB_POLICY_HIDDEN_MAX || D->critic_layers < 1 || D->critic_layers > NPB_POLICY_HIDDEN_MAX)
    return "npb_set_policy: the actor and the critic have 1 .. NPB_POLICY_HIDDEN_MAX (3) hidden layers each";
  for (int l = 0; l < D->actor_layers; l++)
    if (D->actor_width[l] < 1 || D->actor_width[l] > NPB_POLICY_WIDTH_MAX) return "npb_set_policy: a hidden layer of the actor must be 1 .. NPB_POLICY_WIDTH_MAX (128) wide";
  for (int l = 0; l < D->critic_layers; l++)
    if (D->critic_width[l] < 1 || D->critic_width[l] > NPB_POLICY_WIDTH_MAX) return "npb_set_policy: a hidden layer of the critic must be 1 .. NPB_POLICY_WIDTH_MAX (128) wide";
  if (D->activation != NPB_POLICY_RELU && D->activation != NPB_POLICY_TANH) return "npb_set_policy: an unknown activation";
  if (D->first_plant < 0 || D->first_plant + (int64_t)n_plants > ((int64_t)1 << 32)) return "npb_set_policy: first_plant must be >= 0 and first_plant + n_plants <= 2^32, what the counter's first word holds";
  if (!D->value || !D->logp) return "npb_set_policy: NULL value or logp";
  if (((uintptr_t)D->value | (uintptr_t)D->logp) & 3u) return "npb_set_policy: misaligned value or logp: 4-byte aligned";
  if (!D->extras_in) {
    if (D->value_slot >= 0 || D->logp_slot >= 0) return "npb_set_policy: a value or logp slot without extras_in";
  } else {
    if (D->n_extras < 1 || D->n_extras > NPB_ROLLOUT_EXTRAS_MAX) return "npb_set_policy: extras_in with an extras count outside 1 .. NPB_ROLLOUT_EXTRAS_MAX (8)";
    if (D->value_slot < -1 || D->value_slot >= D->n_extras || D->logp_slot < -1 || D->logp_slot >= D->n_extras)
      return "npb_set_policy: a value or logp slot outside -1 .. E - 1";
    if (D->value_slot >= 0 && D->value_slot == D->logp_slot) return "npb_set_policy: value and logp in the same slot";
    if ((uintptr_t)D->extras_in & 3u) return "npb_set_policy: a misaligned extras_in: 4-byte aligned";
  }
  return nullptr;
}
int64_t npb_policy_count(const npb_policy_desc_t *D, int features_cells, int n_axes) {
  if (!D || npb_policy_check(D, 1, features_cells, n_axes)) return 0;
  npb_policy_t P = {};
  npb_policy_layout(D, features_cells, n_axes, &P);
  return (int64_t)P.theta_count;
}
static void policy_drop(NpbHandle *h) {
  ppo_drop(h);
  attachment_drop(&h->core, h->core.primed);
  attachment_drop(&h->pol, h->pol.theta);
  h->pol_t = 0;
  h->seg_starts = nullptr; h->seg_every = h->seg_rows = 0;
}
static int set_policy(NpbHandle *h, const npb_policy_desc_t *desc, const npb_policy_core_t *core);
int npb_set_policy(NpbHandle *h, const npb_policy_desc_t *desc) { return set_policy(h, desc, nullptr); }
int npb_set_policy_core(NpbHandle *h, const npb_policy_desc_t *desc, const npb_policy_core_t *core) { return set_policy(h, desc, desc ? core : nullptr); }
const char *npb_policy_core_check(const npb_policy_core_t *C, int n_plants, int features_cells) {
  if (!C) return nullptr;
  if (n_plants < 1) return "npb_set_policy_core: n_plants must be >= 1";
  if (features_cells < 1 || features_cells > NPB_FEATURES_CELLS_MAX) return "npb_set_policy_core: the features' stack must have 1 .. NPB_FEATURES_CELLS_MAX (256) cells";
  if (C->width < 1 || C->width > NPB_POLICY_WIDTH_MAX) return "npb_set_policy_core: the core must be 1 .. NPB_POLICY_WIDTH_MAX (128) wide";
  if (C->gates != NPB_POLICY_GATES_SOFT && C->gates != NPB_POLICY_GATES_HARD) return "npb_set_policy_core: unknown gates";
  if (!C->hidden) return "npb_set_policy_core: NULL hidden";
  if (C->final_rows < 0) return "npb_set_policy_core: final_rows must be >= 0";
  if ((C->final_rows > 0) != (C->final != nullptr)) return "npb_set_policy_core: final goes with final_rows > 0, and NULL with 0";
  if ((int64_t)n_plants * C->final_rows > INT32_MAX) return "npb_set_policy_core: n_plants * final_rows is beyond what the rollout's final_row (int32) holds";
  if (((uintptr_t)C->hidden | (uintptr_t)C->first | (uintptr_t)C->final) & 3u) return "npb_set_policy_core: misaligned hidden, first or final: 4-byte aligned";
  return nullptr;
}
int64_t npb_policy_core_count(const npb_policy_desc_t *D, const npb_policy_core_t *C, int features_cells, int n_axes) {
  if (!C) return npb_policy_count(D, features_cells, n_axes);
  if (!D || npb_policy_check(D, 1, features_cells, n_axes) || C->width < 1 || C->width > NPB_POLICY_WIDTH_MAX) return 0;
  npd_policy_core_t G = {};
  npb_policy_core_layout(C->width, C->gates, features_cells, &G);
  npb_policy_t P = {};
  npb_policy_layout_at(D, features_cells, C->width, n_axes, G.theta_count, G.padded_count, &P);
  return (int64_t)P.theta_count;
}
static int set_policy(NpbHandle *h, const npb_policy_desc_t *desc, const npb_policy_core_t *core) {
  if (!h) return NPB_EINVAL;
  if (desc && !h->feat.cols) return fail(h, NPB_EINVAL, "npb_set_policy: no features set (npb_set_features first): the policy reads their tensor");
  if (desc && !h->ctl.age) return fail(h, NPB_EINVAL, "npb_set_policy: no controls set (npb_set_controls first): the policy writes their input");
  if (const char *why = npb_policy_check(desc, h->n_plants, h->feat.n_cols * h->feat.stack, h->ctl.n_axes)) return fail(h, NPB_EINVAL, why);
  if (desc && desc->extras_in && (!h->ro.n_final || desc->extras_in != h->ro.D.extras_in || desc->n_extras != h->ro.D.n_extras))
    return fail(h, NPB_EINVAL, "npb_set_policy: extras_in and its count must be the set rollout's (npb_set_rollout first)");
  if (const char *why = npb_policy_core_check(core, h->n_plants, h->feat.n_cols * h->feat.stack)) return fail(h, NPB_EINVAL, why);
  if (core && core->final && (!h->ro.n_final || core->final_rows != h->ro.D.final_rows))
    return fail(h, NPB_EINVAL, "npb_set_policy_core: final and final_rows go with the set rollout's final_obs and final_rows (npb_set_rollout first)");
  NPB_USE_DEVICE(h);
  if (!desc) { policy_drop(h); return NPB_OK; }
  npb_policy_t P = {};
  npd_policy_core_t G = {};
  if (core) {
    npb_policy_core_layout(core->width, core->gates, h->feat.n_cols * h->feat.stack, &G);
    G.hidden = core->hidden; G.first = core->first; G.final = core->final; G.final_rows = core->final_rows;
  }
  npb_policy_layout_at(desc, h->feat.n_cols * h->feat.stack, core ? core->width : h->feat.n_cols * h->feat.stack, h->ctl.n_axes, G.theta_count, G.padded_count, &P);
  /* the allocation: theta [theta_count, padded to 4 floats] | the kernel's copy of the weights [padded_count]; all zero */
  const size_t theta_floats = ((size_t)P.theta_count + 3) & ~(size_t)3, bytes = (theta_floats + P.padded_count) * sizeof(float);
  char *dev = nullptr;
  if (int rc = attachment_alloc(h, "npb_set_policy", "the parameters", nullptr, 0, bytes, &dev)) return rc;
  P.theta = (float *)dev; P.padded = P.theta + theta_floats;
  if (core) {      /* the restart words: primed [n] | seen [n], all zero: every plant unprimed */
    char *words = nullptr;
    if (int rc = attachment_alloc(h, "npb_set_policy_core", "the restart words", nullptr, 0, 2 * (size_t)h->n_plants * sizeof(int32_t), &words)) { (void)hipFree(dev); return rc; }
    G.primed = (int32_t *)words; G.seen = G.primed + h->n_plants;
  }
  policy_drop(h);
  h->pol = P; h->core = G;
  return NPB_OK;
}
int npb_policy_load(NpbHandle *h, const float *theta, int theta_is_device, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->pol.theta) return fail_who(h, "npb_policy_load", g_no_policy);
  if (!theta) return fail(h, NPB_EINVAL, "npb_policy_load: NULL theta");
  NPB_USE_DEVICE(h);
  NPB_HIP(h, hipMemcpyAsync(h->pol.theta, theta, (size_t)h->pol.theta_count * sizeof(float), theta_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                            (hipStream_t)stream));
  if (!theta_is_device) NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream));      /* the host array may go */
  npb_launch_policy_repack(&h->pol, h->core.primed ? &h->core : nullptr, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
/* what npb_policy_values and npb_policy_values_hidden share, their own refusals behind them: rows NULL = the current features (with a core: and the current
 * hidden state, the restart rule applied); the checks of type, count and alignment (`misaligned`: the entry point's words for the last); the critic's launch */
static int policy_values(NpbHandle *h, const char *who, const char *misaligned, const void *rows, int type, int n_rows, const float *hidden_rows, float *out, void *stream) {
  const bool own = !rows;
  if (own) { rows = h->feat.out; type = h->feat.out_f64 ? NPB_FEATURES_F64 : NPB_FEATURES_F32; n_rows = h->n_plants; }
  if (type != NPB_FEATURES_F32 && type != NPB_FEATURES_F64) return fail_who(h, who, ": an unknown type");
  if (n_rows < 1) return fail_who(h, who, ": n_rows must be >= 1");
  if (!out || ((uintptr_t)out & 3u) || ((uintptr_t)hidden_rows & 3u) || ((uintptr_t)rows & (type == NPB_FEATURES_F64 ? 7u : 3u))) return fail_who(h, who, misaligned);
  NPB_USE_DEVICE(h);
  npd_policy_run_t R = {};
  R.x = rows; R.x_f64 = type == NPB_FEATURES_F64; R.rows = n_rows; R.value = out;
  npd_policy_core_run_t cell = {};
  cell.h = own ? h->core.hidden : hidden_rows;
  if (own) { cell.primed = h->core.primed; cell.seen = h->core.seen; cell.index = h->ep_index; }
  policy_launch(h, &R, h->core.primed ? &cell : nullptr, stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
int npb_policy_values(NpbHandle *h, const void *rows, int type, int n_rows, float *out, void *stream) {
  if (!h) return NPB_EINVAL;
  const char *who = "npb_policy_values";
  if (!h->pol.theta) return fail_who(h, who, g_no_policy);
  if (h->core.primed) return fail_who(h, who, ": the policy has a core, and its critic reads a hidden state beside the rows: npb_policy_values_hidden");
  return policy_values(h, who, ": a NULL or misaligned out (4-byte aligned), or rows misaligned for their type", rows, type, n_rows, nullptr, out, stream);
}
static const char *const g_no_core = ": the policy has no core (npb_set_policy_core)";
int npb_policy_values_hidden(NpbHandle *h, const void *rows, int type, int n_rows, const float *hidden_rows, float *out, void *stream) {
  if (!h) return NPB_EINVAL;
  const char *who = "npb_policy_values_hidden";
  if (!h->pol.theta) return fail_who(h, who, g_no_policy);
  if (!h->core.primed) return fail_who(h, who, g_no_core);
  if (!rows && hidden_rows) return fail_who(h, who, ": hidden_rows without rows: the current features go with the handle's own hidden state");
  if (rows && !hidden_rows) return fail_who(h, who, ": rows of the caller's need hidden_rows, the state in front of each");
  return policy_values(h, who, ": a NULL or misaligned out, misaligned hidden_rows (4-byte aligned), or rows misaligned for their type", rows, type, n_rows, hidden_rows,
                       out, stream);
}
/* ---- truncated segments (include/npb.h): the stored start states beside a rollout */
const char *npb_policy_core_segments_check(int every, const float *starts, int rows, int horizon, int core_width) {
  if (every == 0) return nullptr;
  if (core_width < 1) return "npb_policy_core_segments: the policy has no core (npb_set_policy_core first)";
  if (horizon < 1) return "npb_policy_core_segments: no rollout set (npb_set_rollout first): its horizon bounds every and the rows";
  if (every < 0 || every > horizon) return "npb_policy_core_segments: every must be 0 (off) or 1 .. the rollout's horizon";
  if (rows < (horizon + every - 1) / every) return "npb_policy_core_segments: too few rows: starts has ceil(horizon / every) of them";
  if (!starts || ((uintptr_t)starts & 3u)) return "npb_policy_core_segments: a NULL or misaligned starts: 4-byte aligned";
  return nullptr;
}
int npb_policy_core_segments(NpbHandle *h, int every, float *starts, int rows) {
  if (!h) return NPB_EINVAL;
  if (const char *why = npb_policy_core_segments_check(every, starts, rows, h->ro.n_final ? h->ro.D.horizon : 0, h->core.primed ? h->core.H : 0))
    return fail(h, NPB_EINVAL, why);
  h->seg_every = every; h->seg_starts = every ? starts : nullptr; h->seg_rows = every ? rows : 0;
  return NPB_OK;
}

/* hidden (the caller's tensor, which the cell carries from step to step), seen, primed */
static StateParts policy_core_state_parts(const NpbHandle *h) {
  const size_t n = (size_t)h->n_plants, words = n * sizeof(int32_t);
  if (!h->pol.theta) return {nullptr, g_no_policy, "", 0, {}};
  return {h->core.primed, g_no_core, "", 3, {{h->core.hidden, n * (size_t)h->core.H * sizeof(float), false}, {h->core.seen, words, false}, {h->core.primed, words, false}}};
}
int npb_policy_core_get_state(NpbHandle *h, float *hidden, int32_t *seen, int32_t *primed, void *stream) {
  return state_copy(h, "npb_policy_core_get_state", policy_core_state_parts, {hidden, seen, primed}, false, stream);
}
int npb_policy_core_set_state(NpbHandle *h, const float *hidden, const int32_t *seen, const int32_t *primed, void *stream) {
  return state_copy(h, "npb_policy_core_set_state", policy_core_state_parts, {hidden, seen, primed}, true, stream);
}
int npb_policy_noise(NpbHandle *h, uint64_t t, double *z, uint32_t *words, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->pol.theta) return fail_who(h, "npb_policy_noise", g_no_policy);
  if ((!z && !words) || ((uintptr_t)z & 7u) || ((uintptr_t)words & 3u)) return fail(h, NPB_EINVAL, "npb_policy_noise: z and words both NULL, or one of them misaligned");
  NPB_USE_DEVICE(h);
  npb_launch_policy_noise(&h->pol, t, h->n_plants, z, words, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
int npb_policy_get_state(NpbHandle *h, uint64_t *t) {
  if (!h) return NPB_EINVAL;
  if (!h->pol.theta) return fail_who(h, "npb_policy_get_state", g_no_policy);
  if (!t) return fail(h, NPB_EINVAL, "npb_policy_get_state: NULL output");
  *t = h->pol_t;
  return NPB_OK;
}
int npb_policy_set_state(NpbHandle *h, uint64_t t) {
  if (!h) return NPB_EINVAL;
  if (!h->pol.theta) return fail_who(h, "npb_policy_set_state", g_no_policy);
  h->pol_t = t;
  return NPB_OK;
}
int npb_collect(NpbHandle *h, int steps, double *obs, double *reward, uint8_t *done, uint32_t *trip_flags, double *info, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->pol.theta) return fail_who(h, "npb_collect", g_no_policy);
  if (!h->ro.n_final) return fail_who(h, "npb_collect", g_no_rollout);
  if (steps < 1) return fail(h, NPB_EINVAL, "npb_collect: steps must be >= 1");
  if (h->ro.t + steps > h->ro.D.horizon)
    return fail(h, NPB_EINVAL, "npb_collect: the rollout has no room for that many steps (t + steps > horizon): npb_rollout_begin rewinds it");
  if (h->params.heat_source == NPB_HEAT_EXTERNAL)
    return fail(h, NPB_EINVAL, "npb_collect: params.heat_source is NPB_HEAT_EXTERNAL, whose thermal power the caller brings every step: npb_step");
  if (h->params.hs_noise_enabled && !(h->es_on && h->es.noise.key))
    return fail(h, NPB_EINVAL, "npb_collect: the heat-source noise is enabled and its draws come from the caller every step: npb_step, or episode streams (npb_set_episode_streams)");
  if (h->prof && !(h->es_on && h->es.prof.key))
    return fail(h, NPB_EINVAL, "npb_collect: a power profile is seeded (npb_profile_seed) and its rows come from the caller every step: npb_step, or episode streams (npb_set_episode_streams)");
  for (int s = 0; s < steps; s++)
    if (int rc = npb_step(h, nullptr, nullptr, nullptr, nullptr, nullptr, obs, reward, done, trip_flags, info, stream)) return rc;
  return NPB_OK;
}

/* ---- training the policy (include/npb.h, npb_ppo.hip) */
const char *npb_ppo_check(const npb_ppo_desc_t *D, int features_cells, int n_axes) {
  if (!D) return "npb_policy_grad: a NULL descriptor";
  if (features_cells < 1 || features_cells > NPB_FEATURES_CELLS_MAX) return "npb_policy_grad: the features' stack must have 1 .. NPB_FEATURES_CELLS_MAX (256) cells";
  if (n_axes < 1 || n_axes > NPB_CONTROLS_AXES_MAX) return "npb_policy_grad: the axis count must be 1 .. NPB_CONTROLS_AXES_MAX (8)";
  if (!D->obs) return "npb_policy_grad: obs is NULL";
  if (!D->act) return "npb_policy_grad: act is NULL";
  if (!D->logp_old) return "npb_policy_grad: logp_old is NULL";
  if (!D->adv) return "npb_policy_grad: adv is NULL";
  if (!D->ret) return "npb_policy_grad: ret is NULL";
  if (D->obs_type != NPB_FEATURES_F32 && D->obs_type != NPB_FEATURES_F64) return "npb_policy_grad: an unknown obs type";
  if (D->act_type != NPB_CONTROLS_F32 && D->act_type != NPB_CONTROLS_F64) return "npb_policy_grad: an unknown act type";
  if (D->adv_type != NPB_ROLLOUT_F32 && D->adv_type != NPB_ROLLOUT_F64) return "npb_policy_grad: an unknown adv type";
  if (D->count < 1) return "npb_policy_grad: count must be >= 1";
  if (D->rows_per_chain < 32 || D->rows_per_chain % 32) return "npb_policy_grad: rows_per_chain must be a positive multiple of 32";
  if (!(D->clip > 0.0 && D->clip < 1.0)) return "npb_policy_grad: clip must lie inside (0, 1)";
  if (!(D->vf_coef - D->vf_coef == 0.0) || !(D->ent_coef - D->ent_coef == 0.0)) return "npb_policy_grad: vf_coef and ent_coef must be finite";
  if (!(D->max_grad_norm >= 0.0) || !(D->max_grad_norm - D->max_grad_norm == 0.0)) return "npb_policy_grad: max_grad_norm must be finite and >= 0 (0 = off)";
  if (D->max_blocks < 0) return "npb_policy_grad: max_blocks must be >= 0";
  if (((uintptr_t)D->obs & (D->obs_type == NPB_FEATURES_F64 ? 7u : 3u)) || ((uintptr_t)D->act & (D->act_type == NPB_CONTROLS_F64 ? 7u : 3u)) ||
      (((uintptr_t)D->adv | (uintptr_t)D->ret) & (D->adv_type == NPB_ROLLOUT_F64 ? 7u : 3u)) || ((uintptr_t)D->logp_old & 3u))
    return "npb_policy_grad: a misaligned obs, act, logp_old, adv or ret: aligned to their element";
  if ((((uintptr_t)D->logp_new | (uintptr_t)D->value_new) & 3u) || ((uintptr_t)D->ratio & 7u))
    return "npb_policy_grad: a misaligned logp_new, value_new (4-byte aligned) or ratio (8-byte aligned)";
  return nullptr;
}
/* the training buffers on first use, and the chains' workspace grown to `chains` */
static int ppo_room(NpbHandle *h, const char *who, size_t chains) {
  npb_ppo_t &O = h->ppo;
  if (!O.stats) {
    const size_t floats = ((size_t)h->pol.theta_count + 3) & ~(size_t)3, tree = npb_moments_workspace((int64_t)h->pol.std);
    char *dev = nullptr;
    if (int rc = attachment_alloc(h, who, "the gradient and the optimiser's state", nullptr, 0,
                                  (NPB_PPO_STATS + NPB_PPO_STATS_MORE + 1 + tree) * sizeof(double) + 3 * floats * sizeof(float), &dev)) return rc;
    O.stats = (double *)dev; O.more = O.stats + NPB_PPO_STATS; O.gate = (uint32_t *)(O.more + NPB_PPO_STATS_MORE);      /* (two words in one double's room) */
    O.tree = O.more + NPB_PPO_STATS_MORE + 1; O.tree_count = tree;
    O.grad = (float *)(O.tree + tree); O.m = O.grad + floats; O.v = O.m + floats; O.floats = floats; O.step = 0;
  }
  if (chains > O.chains) {      /* (hipFree of the old one waits for a launch that still reads it) */
    char *dev = nullptr;
    if (int rc = attachment_alloc(h, who, "the chains' workspace", nullptr, 0, chains * (NPD_PPO_ROWVALS * sizeof(double) + O.floats * sizeof(float)), &dev)) return rc;
    if (O.chain_stats) (void)hipFree(O.chain_stats);
    O.chain_stats = (double *)dev; O.partials = (float *)(O.chain_stats + chains * NPD_PPO_ROWVALS); O.chains = chains;
  }
  return NPB_OK;
}
const char *npb_ppo_more_check(const npb_ppo_more_t *M, int count) {
  if (!M) return nullptr;
  (void)count;      /* (value_old's length: nothing on the host can see it) */
  if (!(M->clip_vf >= 0.0) || !(M->clip_vf - M->clip_vf == 0.0)) return "npb_policy_grad_more: clip_vf must be finite and >= 0 (0 = off)";
  if (!(M->kl_limit >= 0.0) || !(M->kl_limit - M->kl_limit == 0.0)) return "npb_policy_grad_more: kl_limit must be finite and >= 0 (0 = no gate)";
  if (M->clip_vf > 0.0 && !M->value_old) return "npb_policy_grad_more: clip_vf > 0 and value_old is NULL";
  if ((uintptr_t)M->value_old & 3u) return "npb_policy_grad_more: a misaligned value_old (4-byte aligned)";
  return nullptr;
}
static const char *const g_train_open = ": between npb_policy_train_begin and npb_policy_train_end (npb_policy_train_end first)";
static const char *adam_refusal(double lr, double b1, double b2, double eps) {
  if (!(lr - lr == 0.0) || !(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0) || !(eps >= 0.0) || !(eps - eps == 0.0))
    return ": lr must be finite, b1 and b2 lie in [0, 1), eps be finite and >= 0";
  return nullptr;
}
static const char *const g_core_untrained = ": the policy has a core (npb_set_policy_core), and training through time is not built into the row-wise entry points: rows carry no order; npb_policy_grad_seq, npb_policy_update_seq and npb_policy_shard_sums_seq take whole sequences";
static const char *const g_seq_no_core = ": the policy has no core (npb_set_policy_core): sequences are a recurrent policy's; rows go to npb_policy_grad";
/* THE REQUEST: what a training call was asked to do.  Every entry point that forms a gradient -- npb_policy_grad, _grad_more, _update, _update_more,
 * _shard_sums and their _seq and _segments companions -- is a wrapper that names itself, fills one of these and hands it to ppo_request.
 * kind: what the entry point takes -- rows, whole sequences through the core (S) or segments (S and G).  It is the entry point's, not read off
 * the pointers: a NULL S or G of the caller's is then refused by the kind's own check, in its words and at its place in the order, and never
 * mistaken for another kind.  shard: the sums of one shard into out with the divisor count_total, the handle's gradient left alone (it stands
 * beside out because a shard call's NULL out is a refusal, not a gradient call) */
enum PpoKind { PPO_ROWS, PPO_SEQ, PPO_SEGMENTS };
struct PpoRequest {
  PpoKind kind;
  const npb_ppo_desc_t *D; const npb_ppo_more_t *M; const npb_ppo_seq_t *S; const npb_ppo_segments_t *G;
  bool shard; int64_t count_total; double *out;
};
/* THE ONE ORDER OF REFUSALS of a request ("The training calls: one request path"): no policy; a core under rows, or no core under
 * sequences; the request's exported check (npb_ppo_check, npb_ppo_seq_check or npb_ppo_segments_check); npb_ppo_more_check; then a shard
 * call's own -- a gate, count_total below the minibatch's or beyond 2^53, a NULL or misaligned out.  Then the rooms -- the chains' workspace (a
 * chain is rows_per_chain rows, or plants) and, for sequences without a hidden of the caller's, h' [t][plants][H] -- and the launch.  In
 * front of it an entry point's own refusals: a NULL handle, "the gate is an update's" of a gradient call, and an update's gate rule
 * (ppo_gate).  Behind the check S is not NULL for sequences and segments, and G is not NULL for segments */
static int ppo_request(NpbHandle *h, const char *who, const PpoRequest &Q, void *stream) {
  const npb_ppo_desc_t *D = Q.D;
  const bool rows = Q.kind == PPO_ROWS;
  const npb_ppo_seq_t *S = rows ? nullptr : Q.S;
  const npb_ppo_segments_t *G = Q.kind == PPO_SEGMENTS ? Q.G : nullptr;
  if (!h->pol.theta) return fail_who(h, who, g_no_policy);
  if (rows && h->core.primed) return fail_who(h, who, g_core_untrained);
  if (!rows && !h->core.primed) return fail_who(h, who, g_seq_no_core);
  if (const char *why = rows                   ? npb_ppo_check(D, h->pol.cells, h->pol.n_axes)
                        : Q.kind == PPO_SEQ    ? npb_ppo_seq_check(D, S, h->pol.cells, h->pol.n_axes)
                                               : npb_ppo_segments_check(D, S, G, h->pol.cells, h->pol.n_axes))
    return fail(h, NPB_EINVAL, why);
  if (const char *why = npb_ppo_more_check(Q.M, D->count)) return fail(h, NPB_EINVAL, why);
  if (Q.shard) {
    if (Q.M && Q.M->kl_limit > 0.0) return fail_who(h, who, ": kl_limit > 0: the gate belongs to the combine (npb_policy_apply_shards)");
    if (Q.count_total < (int64_t)D->count)
      return fail_who(h, who, S ? ": count_total < desc->count: it is the cells of the whole update" : ": count_total < desc->count: it is the rows of the whole update");
    if (Q.count_total > ((int64_t)1 << 53)) return fail_who(h, who, ": count_total is beyond 2^53");
    if (!Q.out || ((uintptr_t)Q.out & 7u)) return fail_who(h, who, ": a NULL or misaligned out (8-byte aligned)");
  }
  NPB_USE_DEVICE(h);
  if (int rc = ppo_room(h, who, ((size_t)(S ? S->plants : D->count) + D->rows_per_chain - 1) / D->rows_per_chain)) return rc;
  const size_t floats = S ? (size_t)D->count * (size_t)h->core.H : 0;
  if (S && !S->hidden && floats > h->ppo.hseq_floats) {      /* (hipFree of the old one waits for a launch that still reads it) */
    char *dev = nullptr;
    if (int rc = attachment_alloc(h, who, "the sequences' hidden states", nullptr, 0, floats * sizeof(float), &dev)) return rc;
    if (h->ppo.hseq) (void)hipFree(h->ppo.hseq);
    h->ppo.hseq = (float *)dev; h->ppo.hseq_floats = floats;
  }
  const double n = Q.shard ? (double)Q.count_total : (double)D->count;
  double *out = Q.shard ? Q.out : nullptr;
  if (S) npb_launch_ppo_grad_seq(&h->pol, &h->core, &h->ppo, D, Q.M, S, G, n, out, (hipStream_t)stream);
  else npb_launch_ppo_grad(&h->pol, &h->ppo, D, Q.M, n, out, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
static int ppo_adam(NpbHandle *h, const char *who, double lr, double b1, double b2, double eps, int gated, void *stream) {
  if (!h->pol.theta) return fail_who(h, who, g_no_policy);
  if (const char *why = adam_refusal(lr, b1, b2, eps)) return fail_who(h, who, why);
  if (!h->ppo.stats) return fail_who(h, who, ": no gradient formed yet (npb_policy_grad first)");
  NPB_USE_DEVICE(h);
  h->ppo.step++;
  npb_launch_ppo_adam(&h->pol, &h->ppo, lr, b1, b2, eps, gated, (hipStream_t)stream);
  npb_launch_policy_repack(&h->pol, h->core.primed ? &h->core : nullptr, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
int npb_policy_grad(NpbHandle *h, const npb_ppo_desc_t *D, void *stream) {
  if (!h) return NPB_EINVAL;
  return ppo_request(h, "npb_policy_grad", {PPO_ROWS, D}, stream);
}
int npb_policy_grad_more(NpbHandle *h, const npb_ppo_desc_t *D, const npb_ppo_more_t *M, void *stream) {
  if (!h) return NPB_EINVAL;
  if (M && M->kl_limit > 0.0) return fail(h, NPB_EINVAL, "npb_policy_grad_more: kl_limit > 0: the gate is an update's (npb_policy_update_more)");
  return ppo_request(h, "npb_policy_grad_more", {PPO_ROWS, D, M}, stream);
}
int npb_policy_adam(NpbHandle *h, double lr, double b1, double b2, double eps, void *stream) {
  if (!h) return NPB_EINVAL;
  if (h->ppo.armed) return fail_who(h, "npb_policy_adam", g_train_open);
  return ppo_adam(h, "npb_policy_adam", lr, b1, b2, eps, 0, stream);
}
/* THE GATE RULE of an update (npb_policy_update and its companions, npb_policy_apply_shards), in front of everything else the update refuses:
 * kl_limit > 0 only between npb_policy_train_begin and npb_policy_train_end, kl_limit == 0 never inside, and Adam's arguments refused in front
 * of the gradient (a gated gradient counts itself applied: its Adam step must not be refused behind it) */
static int ppo_gate(NpbHandle *h, const char *who, int gated, double lr, double b1, double b2, double eps) {
  if (gated && !h->ppo.armed) return fail_who(h, who, ": kl_limit > 0 outside npb_policy_train_begin / npb_policy_train_end (npb_policy_train_begin first)");
  if (!gated && h->ppo.armed) return fail_who(h, who, ": kl_limit == 0 between npb_policy_train_begin and npb_policy_train_end: every update of the pair is gated");
  if (h->pol.theta)
    if (const char *why = adam_refusal(lr, b1, b2, eps)) return fail_who(h, who, why);
  return NPB_OK;
}
static int ppo_update(NpbHandle *h, const char *who, const PpoRequest &Q, double lr, double b1, double b2, double eps, void *stream) {
  const int gated = Q.M && Q.M->kl_limit > 0.0;
  if (int rc = ppo_gate(h, who, gated, lr, b1, b2, eps)) return rc;
  if (int rc = ppo_request(h, who, Q, stream)) return rc;
  return ppo_adam(h, who, lr, b1, b2, eps, gated, stream);
}
int npb_policy_update(NpbHandle *h, const npb_ppo_desc_t *D, double lr, double b1, double b2, double eps, void *stream) {
  if (!h) return NPB_EINVAL;
  return ppo_update(h, "npb_policy_update", {PPO_ROWS, D}, lr, b1, b2, eps, stream);
}
int npb_policy_update_more(NpbHandle *h, const npb_ppo_desc_t *D, const npb_ppo_more_t *M, double lr, double b1, double b2, double eps, void *stream) {
  if (!h) return NPB_EINVAL;
  return ppo_update(h, "npb_policy_update_more", {PPO_ROWS, D, M}, lr, b1, b2, eps, stream);
}
int npb_policy_train_begin(NpbHandle *h, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->pol.theta) return fail_who(h, "npb_policy_train_begin", g_no_policy);
  if (h->ppo.armed) return fail_who(h, "npb_policy_train_begin", g_train_open);
  NPB_USE_DEVICE(h);
  if (int rc = ppo_room(h, "npb_policy_train_begin", 0)) return rc;
  NPB_HIP(h, hipMemsetAsync(h->ppo.gate, 0, 2 * sizeof(uint32_t), (hipStream_t)stream));
  h->ppo.armed = 1; h->ppo.step0 = h->ppo.step;
  return NPB_OK;
}
int npb_policy_train_end(NpbHandle *h, uint32_t *applied, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->pol.theta) return fail_who(h, "npb_policy_train_end", g_no_policy);
  if (!h->ppo.armed) return fail_who(h, "npb_policy_train_end", ": no npb_policy_train_begin before it");
  NPB_USE_DEVICE(h);
  h->ppo.armed = 0; h->ppo.step = h->ppo.step0;      /* (whatever HIP says below, nothing stays armed) */
  uint32_t n = 0;
  NPB_HIP(h, hipMemcpyAsync(&n, h->ppo.gate + NPD_PPO_GATE_APPLIED, sizeof n, hipMemcpyDeviceToHost, (hipStream_t)stream));
  NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream));
  h->ppo.step = h->ppo.step0 + n;
  if (applied) *applied = n;
  return NPB_OK;
}
/* ---- one policy across shards: a handle's pinned double sums, and the combine of W of them (include/npb.h, npb_ppo.hip) */
int64_t npb_ppo_shard_count(int64_t theta_count, int n_axes) { return theta_count - 2 * (int64_t)n_axes + NPB_PPO_SHARD_ROWS; }
const char *npb_ppo_shards_check(const npb_ppo_shards_t *S, int64_t count, int n_axes) {
  if (!S) return "npb_policy_apply_shards: a NULL descriptor";
  if (n_axes < 1 || n_axes > NPB_CONTROLS_AXES_MAX) return "npb_policy_apply_shards: the axis count must be 1 .. NPB_CONTROLS_AXES_MAX (8)";
  if (count <= 2 * (int64_t)n_axes) return "npb_policy_apply_shards: theta's count leaves no weights before log_std and std";
  if (!S->sums) return "npb_policy_apply_shards: sums is NULL";
  if ((uintptr_t)S->sums & 7u) return "npb_policy_apply_shards: a misaligned sums (8-byte aligned)";
  if (S->n_shards < 1 || S->n_shards > NPB_PPO_SHARDS_MAX) return "npb_policy_apply_shards: n_shards must be 1 .. NPB_PPO_SHARDS_MAX (64)";
  if (S->count_total < 1 || S->count_total > ((int64_t)1 << 53)) return "npb_policy_apply_shards: count_total must be 1 .. 2^53";
  if (!(S->ent_coef - S->ent_coef == 0.0)) return "npb_policy_apply_shards: ent_coef must be finite";
  if (!(S->max_grad_norm >= 0.0) || !(S->max_grad_norm - S->max_grad_norm == 0.0)) return "npb_policy_apply_shards: max_grad_norm must be finite and >= 0 (0 = off)";
  if (!(S->kl_limit >= 0.0) || !(S->kl_limit - S->kl_limit == 0.0)) return "npb_policy_apply_shards: kl_limit must be finite and >= 0 (0 = no gate)";
  return nullptr;
}
int npb_policy_shard_sums(NpbHandle *h, const npb_ppo_desc_t *D, const npb_ppo_more_t *M, int64_t count_total, double *out, void *stream) {
  if (!h) return NPB_EINVAL;
  return ppo_request(h, "npb_policy_shard_sums", {PPO_ROWS, D, M, nullptr, nullptr, true, count_total, out}, stream);
}
static int ppo_combine(NpbHandle *h, const char *who, const npb_ppo_shards_t *S, void *stream) {
  if (!h->pol.theta) return fail_who(h, who, g_no_policy);
  if (const char *why = npb_ppo_shards_check(S, (int64_t)h->pol.theta_count, h->pol.n_axes)) return fail(h, NPB_EINVAL, why);
  NPB_USE_DEVICE(h);
  if (int rc = ppo_room(h, who, 0)) return rc;
  npb_launch_ppo_combine(&h->pol, &h->ppo, S, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
int npb_policy_combine_shards(NpbHandle *h, const npb_ppo_shards_t *S, void *stream) {
  if (!h) return NPB_EINVAL;
  if (S && S->kl_limit > 0.0) return fail(h, NPB_EINVAL, "npb_policy_combine_shards: kl_limit > 0: the gate is an update's (npb_policy_apply_shards)");
  return ppo_combine(h, "npb_policy_combine_shards", S, stream);
}
int npb_policy_apply_shards(NpbHandle *h, const npb_ppo_shards_t *S, double lr, double b1, double b2, double eps, void *stream) {
  if (!h) return NPB_EINVAL;
  const char *who = "npb_policy_apply_shards";
  const int gated = S && S->kl_limit > 0.0;
  if (int rc = ppo_gate(h, who, gated, lr, b1, b2, eps)) return rc;
  if (int rc = ppo_combine(h, who, S, stream)) return rc;
  return ppo_adam(h, who, lr, b1, b2, eps, gated, stream);
}

/* ---- training through time: whole sequences through the recurrent core (include/npb.h, npb_ppo_seq.hip) */
const char *npb_ppo_seq_check(const npb_ppo_desc_t *D, const npb_ppo_seq_t *S, int features_cells, int n_axes) {
  if (!S) return "npb_policy_grad_seq: a NULL sequence descriptor";
  if (const char *why = npb_ppo_check(D, features_cells, n_axes)) return why;
  if (S->t < 1) return "npb_policy_grad_seq: t must be >= 1";
  if (S->plants < 1) return "npb_policy_grad_seq: plants must be >= 1";
  if ((int64_t)S->t * S->plants != (int64_t)D->count) return "npb_policy_grad_seq: desc->count must be t * plants";
  if (S->n_plants < 1) return "npb_policy_grad_seq: n_plants must be >= 1";
  if ((int64_t)S->t * S->n_plants > INT32_MAX) return "npb_policy_grad_seq: t * n_plants is beyond 2^31 - 1";
  if (!S->episode) return "npb_policy_grad_seq: episode is NULL";
  if (!S->ended) return "npb_policy_grad_seq: ended is NULL";
  if (!S->first) return "npb_policy_grad_seq: first is NULL";
  if (((uintptr_t)S->index | (uintptr_t)S->episode | (uintptr_t)S->first | (uintptr_t)S->hidden) & 3u)
    return "npb_policy_grad_seq: a misaligned index, episode, first or hidden: 4-byte aligned";
  return nullptr;
}
/* the same for truncated segments (include/npb.h): what npb_ppo_seq_check refuses, and the segments' own */
const char *npb_ppo_segments_check(const npb_ppo_desc_t *D, const npb_ppo_seq_t *S, const npb_ppo_segments_t *G, int features_cells, int n_axes) {
  if (const char *why = npb_ppo_seq_check(D, S, features_cells, n_axes)) return why;
  if (!G) return "npb_policy_grad_segments: a NULL segments descriptor";
  if (G->every < 1) return "npb_policy_grad_segments: every must be >= 1";
  if (G->chunks < 1) return "npb_policy_grad_segments: chunks must be >= 1";
  if (S->t != G->every) return "npb_policy_grad_segments: seq->t must be every: a sequence of the minibatch is one segment";
  if ((int64_t)G->chunks * G->every * S->n_plants > INT32_MAX) return "npb_policy_grad_segments: chunks * every * n_plants is beyond 2^31 - 1";
  return nullptr;
}
int npb_policy_grad_seq(NpbHandle *h, const npb_ppo_desc_t *D, const npb_ppo_more_t *M, const npb_ppo_seq_t *S, void *stream) {
  if (!h) return NPB_EINVAL;
  if (M && M->kl_limit > 0.0) return fail(h, NPB_EINVAL, "npb_policy_grad_seq: kl_limit > 0: the gate is an update's (npb_policy_update_seq)");
  return ppo_request(h, "npb_policy_grad_seq", {PPO_SEQ, D, M, S}, stream);
}
int npb_policy_grad_segments(NpbHandle *h, const npb_ppo_desc_t *D, const npb_ppo_more_t *M, const npb_ppo_seq_t *S, const npb_ppo_segments_t *G, void *stream) {
  if (!h) return NPB_EINVAL;
  if (M && M->kl_limit > 0.0) return fail(h, NPB_EINVAL, "npb_policy_grad_segments: kl_limit > 0: the gate is an update's (npb_policy_update_segments)");
  return ppo_request(h, "npb_policy_grad_segments", {PPO_SEGMENTS, D, M, S, G}, stream);
}
int npb_policy_update_seq(NpbHandle *h, const npb_ppo_desc_t *D, const npb_ppo_more_t *M, const npb_ppo_seq_t *S, double lr, double b1, double b2, double eps,
                          void *stream) {
  if (!h) return NPB_EINVAL;
  return ppo_update(h, "npb_policy_update_seq", {PPO_SEQ, D, M, S}, lr, b1, b2, eps, stream);
}
int npb_policy_update_segments(NpbHandle *h, const npb_ppo_desc_t *D, const npb_ppo_more_t *M, const npb_ppo_seq_t *S, const npb_ppo_segments_t *G, double lr,
                               double b1, double b2, double eps, void *stream) {
  if (!h) return NPB_EINVAL;
  return ppo_update(h, "npb_policy_update_segments", {PPO_SEGMENTS, D, M, S, G}, lr, b1, b2, eps, stream);
}
int npb_policy_shard_sums_seq(NpbHandle *h, const npb_ppo_desc_t *D, const npb_ppo_more_t *M, const npb_ppo_seq_t *S, int64_t count_total, double *out,
                              void *stream) {
  if (!h) return NPB_EINVAL;
  return ppo_request(h, "npb_policy_shard_sums_seq", {PPO_SEQ, D, M, S, nullptr, true, count_total, out}, stream);
}
int npb_policy_shard_sums_segments(NpbHandle *h, const npb_ppo_desc_t *D, const npb_ppo_more_t *M, const npb_ppo_seq_t *S, const npb_ppo_segments_t *G,
                                   int64_t count_total, double *out, void *stream) {
  if (!h) return NPB_EINVAL;
  return ppo_request(h, "npb_policy_shard_sums_segments", {PPO_SEGMENTS, D, M, S, G, true, count_total, out}, stream);
}
/* the refresh of the stored states under the current theta (npb_ppo_seq.hip's forward sweep over the rollout's own tensors) */
int npb_policy_segment_starts(NpbHandle *h, int every, void *stream) {
  if (!h) return NPB_EINVAL;
  const char *who = "npb_policy_segment_starts";
  if (!h->pol.theta) return fail_who(h, who, g_no_policy);
  if (!h->core.primed) return fail_who(h, who, g_seq_no_core);
  if (!h->ro.n_final) return fail_who(h, who, g_no_rollout);
  if (!h->seg_every) return fail_who(h, who, ": no stored states set (npb_policy_core_segments first)");
  if (every != h->seg_every) return fail_who(h, who, ": every is not the one the stored states were set with (npb_policy_core_segments)");
  if (!h->core.first) return fail_who(h, who, ": the core has no first: the state in front of slot 0 is where the recurrence starts");
  if (h->ro.t < 1) return fail_who(h, who, ": nothing recorded yet (t == 0)");
  if (h->ro.t % every) return fail_who(h, who, ": the recorded slots are not a multiple of every: ragged last segments are not supported");
  NPB_USE_DEVICE(h);
  if (h->ro.t / every > 1) {
    npb_launch_segment_starts(&h->pol, &h->core, h->ro.D.obs, h->ro.obs_bytes == 8, h->ro.t, h->n_plants, every, h->ro.D.episode, h->ro.D.ended, h->seg_starts,
                              (hipStream_t)stream);
    NPB_HIP(h, hipGetLastError());
  }
  return NPB_OK;
}

/* a copy between device buffers on the stream */
static int ppo_copy_out(NpbHandle *h, const char *who, const void *src, void *dst, size_t bytes, size_t align, bool needs_grad, void *stream) {
  if (!h->pol.theta) return fail_who(h, who, g_no_policy);
  if (!dst || ((uintptr_t)dst & (align - 1))) return fail_who(h, who, ": a NULL or misaligned output");
  if (needs_grad && !h->ppo.stats) return fail_who(h, who, ": no gradient formed yet (npb_policy_grad first)");
  NPB_USE_DEVICE(h);
  NPB_HIP(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return NPB_OK;
}
int npb_policy_get_grad(NpbHandle *h, float *grad, void *stream) {
  if (!h) return NPB_EINVAL;
  return ppo_copy_out(h, "npb_policy_get_grad", h->ppo.grad, grad, (size_t)h->pol.theta_count * sizeof(float), 4, true, stream);
}
int npb_policy_get_stats(NpbHandle *h, double *stats, void *stream) {
  if (!h) return NPB_EINVAL;
  return ppo_copy_out(h, "npb_policy_get_stats", h->ppo.stats, stats, NPB_PPO_STATS * sizeof(double), 8, true, stream);
}
int npb_policy_get_stats_more(NpbHandle *h, double *more, void *stream) {
  if (!h) return NPB_EINVAL;
  return ppo_copy_out(h, "npb_policy_get_stats_more", h->ppo.more, more, NPB_PPO_STATS_MORE * sizeof(double), 8, true, stream);
}
int npb_policy_get_theta(NpbHandle *h, float *theta, void *stream) {
  if (!h) return NPB_EINVAL;
  return ppo_copy_out(h, "npb_policy_get_theta", h->pol.theta, theta, (size_t)h->pol.theta_count * sizeof(float), 4, false, stream);
}
int npb_policy_optimizer_get_state(NpbHandle *h, float *m, float *v, uint64_t *step, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->pol.theta) return fail_who(h, "npb_policy_optimizer_get_state", g_no_policy);
  if (!m || !v || !step) return fail(h, NPB_EINVAL, "npb_policy_optimizer_get_state: NULL output");
  if (h->ppo.armed) return fail_who(h, "npb_policy_optimizer_get_state", g_train_open);
  NPB_USE_DEVICE(h);
  if (int rc = ppo_room(h, "npb_policy_optimizer_get_state", 0)) return rc;
  const size_t bytes = (size_t)h->pol.theta_count * sizeof(float);
  NPB_HIP(h, hipMemcpyAsync(m, h->ppo.m, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  NPB_HIP(h, hipMemcpyAsync(v, h->ppo.v, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream));
  *step = h->ppo.step;
  return NPB_OK;
}
int npb_policy_optimizer_set_state(NpbHandle *h, const float *m, const float *v, uint64_t step, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->pol.theta) return fail_who(h, "npb_policy_optimizer_set_state", g_no_policy);
  if (!m || !v) return fail(h, NPB_EINVAL, "npb_policy_optimizer_set_state: NULL input");
  if (h->ppo.armed) return fail_who(h, "npb_policy_optimizer_set_state", g_train_open);
  NPB_USE_DEVICE(h);
  if (int rc = ppo_room(h, "npb_policy_optimizer_set_state", 0)) return rc;
  const size_t bytes = (size_t)h->pol.theta_count * sizeof(float);
  NPB_HIP(h, hipMemcpyAsync(h->ppo.m, m, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  NPB_HIP(h, hipMemcpyAsync(h->ppo.v, v, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream));      /* the host arrays may go */
  h->ppo.step = step;
  return NPB_OK;
}

/* ---- the normaliser (include/npb.h, npd_normalizer.h, npb_minibatch.hip): running statistics of the features' raw columns and of the
 * discounted return, folded behind every step.  What a column of the features is to it: its kind and whether its ref is a second column --
 * read off the caller's descriptor by the check without a handle, off the handle's host table by npb_set_normalizer */
struct NormFeatures { int n; int kind[NPB_FEATURES_COLS_MAX]; int ref_col[NPB_FEATURES_COLS_MAX]; };
static const char *normalizer_refusal(const npb_normalizer_desc_t *D, int n_plants, const NormFeatures *F) {
  if (!D) return nullptr;
  if (n_plants < 1) return "npb_set_normalizer: n_plants must be >= 1";
  if (D->n_columns < 0 || D->n_columns > NPB_FEATURES_COLS_MAX || (D->n_columns > 0 && !D->columns))
    return "npb_set_normalizer: the column count must be 0 .. NPB_FEATURES_COLS_MAX (64), with their indices";
  if (D->n_columns == 0 && !D->reward) return "npb_set_normalizer: neither columns nor reward: nothing to normalise";
  if (D->n_columns > 0 && !F) return "npb_set_normalizer: columns chosen while no features are set (npb_set_features first)";
  bool taken[NPB_FEATURES_COLS_MAX] = {};
  for (int c = 0; c < D->n_columns; c++) {
    const int j = D->columns[c];
    if (j < 0 || j >= F->n) return "npb_set_normalizer: a column index out of range: it names a column of the features";
    if (taken[j]) return "npb_set_normalizer: a column named twice";
    taken[j] = true;
    if (F->kind[j] != NPB_FEATURE_KIND_AFFINE) return "npb_set_normalizer: a NPB_FEATURE_BITS column cannot be normalised";
    if (F->ref_col[j]) return "npb_set_normalizer: a column whose ref is a second column (a setpoint error) cannot be normalised";
  }
  if (!(D->eps >= 0.0)) return "npb_set_normalizer: eps must be >= 0 (a NaN is not)";
  if (D->reward) {
    if (!(D->gamma >= 0.0 && D->gamma <= 1.0)) return "npb_set_normalizer: gamma must lie in [0, 1] (a NaN does not)";
    if (!(D->clip > 0.0)) return "npb_set_normalizer: clip must be positive (a NaN is not)";
    if (!D->norm_reward) return "npb_set_normalizer: a NULL norm_reward: the return stream writes it";
    if ((uintptr_t)D->norm_reward & 7u) return "npb_set_normalizer: a misaligned norm_reward: 8-byte aligned";
  }
  return nullptr;
}
const char *npb_normalizer_check(const npb_normalizer_desc_t *D, int n_plants, const npb_features_desc_t *features) {
  NormFeatures F = {};
  if (D && n_plants < 1) return normalizer_refusal(D, n_plants, nullptr);
  if (features) {
    if (const char *why = npb_features_check(features, n_plants)) return why;
    F.n = features->n_columns;
    for (int j = 0; j < F.n; j++) { F.kind[j] = features->columns[j].kind; F.ref_col[j] = features->columns[j].ref_from_column != 0; }
  }
  return normalizer_refusal(D, n_plants, features ? &F : nullptr);
}
/* the table back to the columns' own ref and scale */
static int normalizer_restore_table(NpbHandle *h, const char *who) {
  if (!h->feat.cols || h->feat_host.empty()) return NPB_OK;
  hipError_t e = hipMemcpy((void *)h->feat.cols, h->feat_host.data(), h->feat_host.size() * sizeof(npb_feature_col_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(h, NPB_EHIP, (std::string(who) + ": putting the features' own ref and scale back failed").c_str(), e);
  return NPB_OK;
}
int npb_set_normalizer(NpbHandle *h, const npb_normalizer_desc_t *desc) {
  if (!h) return NPB_EINVAL;
  if (h->ro.n_final)
    return fail(h, NPB_EINVAL, "npb_set_normalizer: a rollout is set (npb_set_rollout) and records the reward the normaliser would change; npb_set_rollout(h, NULL) first: set the normaliser, then the rollout");
  NormFeatures F = {};
  if (h->feat.cols) {
    F.n = h->feat.n_cols;
    for (int j = 0; j < F.n; j++) { F.kind[j] = h->feat_host[j].kind; F.ref_col[j] = h->feat_host[j].ref_col; }
  }
  if (const char *why = normalizer_refusal(desc, h->n_plants, h->feat.cols ? &F : nullptr)) return fail(h, NPB_EINVAL, why);
  NPB_USE_DEVICE(h);
  /* the old normaliser's columns get their own ref and scale back (a synchronous copy on the null stream: the caller has let the steps on
   * a non-blocking stream of its own finish, as before every npb_set_*) -- but only once nothing can fail any more: off here, and below
   * behind the new allocation, so that a refused replacement leaves the old normaliser AND its table as they were */
  const bool had_columns = h->norm.streams && h->norm.n_cols;
  if (!desc) {
    if (had_columns) { if (int rc = normalizer_restore_table(h, "npb_set_normalizer")) return rc; }
    attachment_drop(&h->norm, h->norm.streams);
    return NPB_OK;
  }
  /* the allocation: [the streams] | count, mean, M2, scale [S] | the shards' base [3][S] (normalizer_base) | the partials [3 S][every level]
   * | ret [n] | primed, seen, ended [n] */
  const int C = desc->n_columns, S = C + (desc->reward ? 1 : 0);
  std::vector<npb_norm_stream_t> table(NPB_NORM_STREAMS_MAX);
  for (int c = 0; c < C; c++) {
    const npb_feature_col_t &O = h->feat_host[desc->columns[c]];
    table[c] = npb_norm_stream_t{O.c, O.ref, O.scale, desc->columns[c], 0};
  }
  if (desc->reward) table[C] = npb_norm_stream_t{npb_colstat_col_t{}, 0.0, 1.0, -1, 0};
  static_assert(sizeof(npb_norm_stream_t) % 8 == 0, "packed");
  const size_t n = (size_t)h->n_plants, table_bytes = table.size() * sizeof(npb_norm_stream_t), ws = npb_moments_workspace(h->n_plants);
  const size_t doubles = 7 * (size_t)S + 3 * (size_t)S * ws + (desc->reward ? n : 0);
  const size_t bytes = table_bytes + doubles * sizeof(double) + (desc->reward ? 3 * n * sizeof(int32_t) : 0);
  char *dev = nullptr;
  if (int rc = attachment_alloc(h, "npb_set_normalizer", "the streams, the statistics and the partials", table.data(), table_bytes, bytes, &dev)) return rc;
  if (had_columns) { if (int rc = normalizer_restore_table(h, "npb_set_normalizer")) { (void)hipFree(dev); return rc; } }
  npb_normalizer_t Z = {};
  Z.streams = (const npb_norm_stream_t *)dev; Z.n_streams = S; Z.n_cols = C; Z.reward_on = desc->reward != 0;
  Z.eps = desc->eps; Z.gamma = desc->gamma; Z.clip = desc->clip;
  Z.count = (double *)(dev + table_bytes); Z.mean = Z.count + S; Z.M2 = Z.mean + S; Z.scale = Z.M2 + S;
  Z.partial = Z.scale + 4 * (size_t)S; Z.ws_stride = ws;
  if (desc->reward) {
    Z.ret = Z.partial + 3 * (size_t)S * ws;
    Z.primed = (int32_t *)(Z.ret + n); Z.seen = Z.primed + n; Z.ended = Z.seen + n;
    Z.norm_reward = desc->norm_reward;
  }
  Z.feat_cols = (npb_feature_col_t *)h->feat.cols;
  attachment_drop(&h->norm, h->norm.streams);
  h->norm = Z;
  h->norm_training = true;
  npb_launch_normalizer_finish(&h->norm, 0, nullptr);      /* no batch: scale[] takes the streams' own, which the reward kernel reads */
  NPB_HIP(h, hipGetLastError());
  NPB_HIP(h, hipStreamSynchronize(nullptr));
  return NPB_OK;
}
/* what the shards agreed on at the last synchronisation, device [3][S]: count, mean, M2; zeros from npb_set_normalizer on */
static double *normalizer_base(const NpbHandle *h) { return h->norm.scale + h->norm.n_streams; }
int npb_normalizer_training(NpbHandle *h, int on) {
  if (!h) return NPB_EINVAL;
  if (!h->norm.streams) return fail_who(h, "npb_normalizer_training", g_no_normalizer);
  h->norm_training = on != 0;
  return NPB_OK;
}
int npb_normalizer_clear(NpbHandle *h, const uint8_t *mask, void *stream) {
  if (!h) return NPB_EINVAL;
  if (h->norm.streams && !h->norm.reward_on) return NPB_OK;      /* no return stream: no carry to start again */
  return attachment_clear(h, "npb_normalizer_clear", h->norm.streams, g_no_normalizer,
                          [&] { npb_launch_unprime(h->norm.primed, mask, h->n_plants, (hipStream_t)stream); });
}
/* count, mean, M2; with the return stream ret, primed, seen, ended */
static StateParts normalizer_state_parts(const NpbHandle *h) {
  const npb_normalizer_t &Z = h->norm;
  const size_t n = Z.reward_on ? (size_t)h->n_plants : 0, s = (size_t)Z.n_streams * sizeof(double), words = n * sizeof(int32_t);
  const bool none = !Z.reward_on;
  return {Z.streams, g_no_normalizer, " (ret, primed, seen and ended may be NULL only without the return stream)", 7,
          {{Z.count, s, false}, {Z.mean, s, false}, {Z.M2, s, false}, {Z.ret, n * sizeof(double), none}, {Z.primed, words, none},
           {Z.seen, words, none}, {Z.ended, words, none}}};
}
int npb_normalizer_get_state(NpbHandle *h, double *count, double *mean, double *M2, double *ret, int32_t *primed, int32_t *seen, int32_t *ended,
                             void *stream) {
  return state_copy(h, "npb_normalizer_get_state", normalizer_state_parts, {count, mean, M2, ret, primed, seen, ended}, false, stream);
}
int npb_normalizer_set_state(NpbHandle *h, const double *count, const double *mean, const double *M2, const double *ret, const int32_t *primed,
                             const int32_t *seen, const int32_t *ended, void *stream) {
  if (int rc = state_copy(h, "npb_normalizer_set_state", normalizer_state_parts, {count, mean, M2, ret, primed, seen, ended}, true, stream)) return rc;
  NPB_USE_DEVICE(h);
  npb_launch_normalizer_finish(&h->norm, 0, (hipStream_t)stream);      /* the table follows the loaded state */
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
/* ---- one normaliser across shards (include/npb.h, npb_minibatch.hip): a handle's delta since the base, and the combine of W of them */
int npb_normalizer_shard_count(NpbHandle *h) {
  if (!h) return 0;
  if (!h->norm.streams) { (void)fail_who(h, "npb_normalizer_shard_count", g_no_normalizer); return 0; }
  return 3 * h->norm.n_streams;
}
const char *npb_normalizer_shards_check(const double *deltas, int n_shards) {
  if (!deltas) return "npb_normalizer_apply_shards: deltas is NULL";
  if ((uintptr_t)deltas & 7u) return "npb_normalizer_apply_shards: a misaligned deltas (8-byte aligned)";
  if (n_shards < 1 || n_shards > NPB_PPO_SHARDS_MAX) return "npb_normalizer_apply_shards: n_shards must be 1 .. NPB_PPO_SHARDS_MAX (64)";
  return nullptr;
}
int npb_normalizer_shard_delta(NpbHandle *h, double *out, void *stream) {
  if (!h) return NPB_EINVAL;
  const char *who = "npb_normalizer_shard_delta";
  if (!h->norm.streams) return fail_who(h, who, g_no_normalizer);
  if (!out || ((uintptr_t)out & 7u)) return fail_who(h, who, ": a NULL or misaligned out (8-byte aligned)");
  NPB_USE_DEVICE(h);
  npb_launch_normalizer_delta(&h->norm, normalizer_base(h), out, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
int npb_normalizer_apply_shards(NpbHandle *h, const double *deltas, int n_shards, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->norm.streams) return fail_who(h, "npb_normalizer_apply_shards", g_no_normalizer);
  if (const char *why = npb_normalizer_shards_check(deltas, n_shards)) return fail(h, NPB_EINVAL, why);
  NPB_USE_DEVICE(h);
  npb_launch_normalizer_combine(&h->norm, normalizer_base(h), deltas, n_shards, (hipStream_t)stream);
  npb_launch_normalizer_finish(&h->norm, 0, (hipStream_t)stream);      /* no batch: the table follows the state */
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
static int normalizer_base_copy(NpbHandle *h, const char *who, double *host, bool to_device, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->norm.streams) return fail_who(h, who, g_no_normalizer);
  if (!host) return fail_who(h, who, to_device ? ": NULL input" : ": NULL output");
  NPB_USE_DEVICE(h);
  const size_t bytes = 3 * (size_t)h->norm.n_streams * sizeof(double);
  NPB_HIP(h, to_device ? hipMemcpyAsync(normalizer_base(h), host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream)
                       : hipMemcpyAsync(host, normalizer_base(h), bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  NPB_HIP(h, hipStreamSynchronize((hipStream_t)stream));      /* the host array may go */
  return NPB_OK;
}
int npb_normalizer_get_base(NpbHandle *h, double *base, void *stream) { return normalizer_base_copy(h, "npb_normalizer_get_base", base, false, stream); }
int npb_normalizer_set_base(NpbHandle *h, const double *base, void *stream) {
  return normalizer_base_copy(h, "npb_normalizer_set_base", (double *)base, true, stream);
}

/* ---- between the advantages and the optimiser (include/npb.h, npb_minibatch.hip): pinned moments, the permutation, the minibatch */
static const char *moments_check(const npb_moments_desc_t *M) {
  if (!M) return "npb_rollout_moments: a NULL descriptor";
  if (!M->src || !M->out) return "npb_rollout_moments: NULL src or out";
  if (M->type != NPB_ROLLOUT_F32 && M->type != NPB_ROLLOUT_F64) return "npb_rollout_moments: an unknown type";
  if (M->rows < 1 || M->cols < 1) return "npb_rollout_moments: rows and cols must be >= 1";
  if (M->cols > INT32_MAX) return "npb_rollout_moments: cols beyond 2^31 - 1";
  if (M->rows > ((int64_t)1 << 53) / M->cols) return "npb_rollout_moments: rows * cols beyond 2^53, what a double counts exactly";
  if (M->ddof < 0) return "npb_rollout_moments: ddof must be >= 0";
  if (M->rows * M->cols <= (int64_t)M->ddof) return "npb_rollout_moments: rows * cols <= ddof: nothing to divide by";
  if ((uintptr_t)M->src & (M->type == NPB_ROLLOUT_F64 ? 7u : 3u)) return "npb_rollout_moments: src is misaligned for its type";
  if ((uintptr_t)M->out & 7u) return "npb_rollout_moments: a misaligned out: 8-byte aligned";
  return nullptr;
}
/* the partials' workspace holds a tensor of `cols` columns */
static int moments_room(NpbHandle *h, const char *who, int64_t cols) {
  const size_t need = npb_moments_workspace(cols);
  if (need > h->mom.cap) {      /* (hipFree of the old one waits for a launch that still reads it) */
    char *dev = nullptr;
    if (int rc = attachment_alloc(h, who, "the partials' workspace", nullptr, 0, need * sizeof(double), &dev)) return rc;
    attachment_drop(&h->mom, h->mom.ws);
    h->mom.ws = (double *)dev; h->mom.cap = need;
  }
  return NPB_OK;
}
int npb_rollout_moments(NpbHandle *h, const npb_moments_desc_t *M, void *stream) {
  if (!h) return NPB_EINVAL;
  if (const char *why = moments_check(M)) return fail(h, NPB_EINVAL, why);
  NPB_USE_DEVICE(h);
  if (int rc = moments_room(h, "npb_rollout_moments", M->cols)) return rc;
  npb_launch_moments(M, h->mom.ws, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
/* ---- the moments across shards: a shard's part, and the combine of W parts (include/npb.h, npb_minibatch.hip) */
const char *npb_moments_shards_check(const npb_moments_desc_t *M, const double *part, const double *parts, int n_shards, int ddof, const double *out) {
  if (M) {      /* the part */
    if (const char *why = moments_check(M)) return why;
    if (!part) return "npb_rollout_moments_part: part is NULL";
    if ((uintptr_t)part & 7u) return "npb_rollout_moments_part: a misaligned part (8-byte aligned)";
    return nullptr;
  }
  if (!parts) return "npb_rollout_moments_combine: parts is NULL";
  if ((uintptr_t)parts & 7u) return "npb_rollout_moments_combine: a misaligned parts (8-byte aligned)";
  if (n_shards < 1 || n_shards > NPB_PPO_SHARDS_MAX) return "npb_rollout_moments_combine: n_shards must be 1 .. NPB_PPO_SHARDS_MAX (64)";
  if (ddof < 0) return "npb_rollout_moments_combine: ddof must be >= 0";
  if (!out) return "npb_rollout_moments_combine: out is NULL";
  if ((uintptr_t)out & 7u) return "npb_rollout_moments_combine: a misaligned out (8-byte aligned)";
  return nullptr;
}
int npb_rollout_moments_part(NpbHandle *h, const npb_moments_desc_t *M, int squares, double *part, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!M) return fail(h, NPB_EINVAL, "npb_rollout_moments_part: a NULL descriptor");
  if (const char *why = npb_moments_shards_check(M, part, nullptr, 0, 0, nullptr)) return fail(h, NPB_EINVAL, why);
  NPB_USE_DEVICE(h);
  if (int rc = moments_room(h, "npb_rollout_moments_part", M->cols)) return rc;
  npb_launch_moments_part(M, squares != 0, h->mom.ws, part, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
int npb_rollout_moments_combine(NpbHandle *h, const double *parts, int n_shards, int squares, int ddof, double *out, void *stream) {
  if (!h) return NPB_EINVAL;
  if (const char *why = npb_moments_shards_check(nullptr, nullptr, parts, n_shards, ddof, out)) return fail(h, NPB_EINVAL, why);
  NPB_USE_DEVICE(h);
  npb_launch_moments_combine(parts, n_shards, squares != 0, ddof, out, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
int npb_rollout_permutation(NpbHandle *h, int64_t N, const uint32_t *keys, int64_t first, int64_t count, int32_t *out, void *stream) {
  if (!h) return NPB_EINVAL;
  if (N < 1 || N > INT32_MAX) return fail(h, NPB_EINVAL, "npb_rollout_permutation: N must be 1 .. 2^31 - 1");
  if (count < 1) return fail(h, NPB_EINVAL, "npb_rollout_permutation: count must be >= 1");
  if (first < 0 || first > N - count) return fail(h, NPB_EINVAL, "npb_rollout_permutation: entries [first, first + count) must lie inside [0, N)");
  if (!keys || !out) return fail(h, NPB_EINVAL, "npb_rollout_permutation: NULL keys or out");
  if ((uintptr_t)out & 3u) return fail(h, NPB_EINVAL, "npb_rollout_permutation: a misaligned out: 4-byte aligned");
  NPB_USE_DEVICE(h);
  npb_launch_permutation((uint32_t)N, keys, first, count, out, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
/* every: 0 for npb_rollout_minibatch's units, else the slots of a segment (npb_rollout_minibatch_segments) */
static const char *minibatch_check(const npb_minibatch_desc_t *D, int every, int n_plants, int t, int features_cells, int n_axes, int n_extras) {
  if (!D) return "npb_rollout_minibatch: a NULL descriptor";
  if (n_plants < 1) return "npb_rollout_minibatch: n_plants must be >= 1";
  if (features_cells < 1) return "npb_rollout_minibatch: the features' stack must have cells (K * C >= 1)";
  if (n_axes < 0 || n_extras < 0) return "npb_rollout_minibatch: a negative axis or extras count";
  if (t < 1) return "npb_rollout_minibatch: nothing recorded yet (t == 0)";
  if (D->unit != NPB_MINIBATCH_TRANSITION && D->unit != NPB_MINIBATCH_PLANT && !(every && D->unit == NPB_MINIBATCH_SEGMENT))
    return "npb_rollout_minibatch: an unknown unit";
  if (D->type != NPB_ROLLOUT_F32 && D->type != NPB_ROLLOUT_F64) return "npb_rollout_minibatch: an unknown type";
  const int64_t N = D->unit == NPB_MINIBATCH_PLANT ? (int64_t)n_plants : (int64_t)(every ? t / every : t) * n_plants;
  if (D->unit != NPB_MINIBATCH_PLANT && (int64_t)t * n_plants > INT32_MAX) return "npb_rollout_minibatch: t * n_plants is beyond 2^31 - 1, what an index (int32) holds";
  if (D->count < 1) return "npb_rollout_minibatch: count must be >= 1";
  if (D->first < 0 || D->first > N - D->count) return "npb_rollout_minibatch: entries [first, first + count) must lie inside [0, N)";
  if (!D->index) return "npb_rollout_minibatch: index is NULL";
  if (D->act && n_axes == 0) return "npb_rollout_minibatch: an act output without axes (the rollout recorded no controls)";
  if (D->extra && n_extras == 0) return "npb_rollout_minibatch: an extra output without extras";
  if (D->adv_out && !D->adv) return "npb_rollout_minibatch: adv_out without adv";
  if (D->ret_out && !D->ret) return "npb_rollout_minibatch: ret_out without ret";
  if (D->moments && !D->adv_out) return "npb_rollout_minibatch: moments are set and adv_out, what they normalise, is NULL";
  if (!(D->eps >= 0.0)) return "npb_rollout_minibatch: eps must be >= 0 (a NaN is not)";
  if (D->max_blocks < 0) return "npb_rollout_minibatch: max_blocks must be >= 0";
  if (((uintptr_t)D->obs | (uintptr_t)D->act | (uintptr_t)D->extra) & 15u) return "npb_rollout_minibatch: a misaligned obs, act or extra output: 16-byte aligned";
  if ((uintptr_t)D->moments & 7u) return "npb_rollout_minibatch: misaligned moments: 8-byte aligned";
  if (((uintptr_t)D->adv | (uintptr_t)D->ret | (uintptr_t)D->adv_out | (uintptr_t)D->ret_out) & (D->type == NPB_ROLLOUT_F64 ? 7u : 3u))
    return "npb_rollout_minibatch: misaligned adv, ret, adv_out or ret_out: aligned to their element";
  if ((uintptr_t)D->index & 3u) return "npb_rollout_minibatch: a misaligned index: 4-byte aligned";
  return nullptr;
}
const char *npb_minibatch_check(const npb_minibatch_desc_t *D, int n_plants, int t, int features_cells, int n_axes, int n_extras) {
  return minibatch_check(D, 0, n_plants, t, features_cells, n_axes, n_extras);
}
const char *npb_minibatch_segments_check(const npb_minibatch_desc_t *D, int every, int n_plants, int t, int features_cells, int n_axes, int n_extras) {
  if (D && D->unit != NPB_MINIBATCH_SEGMENT) return "npb_rollout_minibatch_segments: the unit must be NPB_MINIBATCH_SEGMENT";
  if (D && t >= 1) {
    if (every < 1) return "npb_rollout_minibatch_segments: every must be >= 1";
    if (every > t) return "npb_rollout_minibatch_segments: every is beyond the recorded slots t";
    if (t % every) return "npb_rollout_minibatch_segments: t is not a multiple of every: ragged last segments are not supported";
  }
  return minibatch_check(D, every > 0 ? every : 1, n_plants, t, features_cells, n_axes, n_extras);
}
int npb_rollout_minibatch(NpbHandle *h, const npb_minibatch_desc_t *D, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->ro.n_final) return fail_who(h, "npb_rollout_minibatch", g_no_rollout);
  const npb_rollout_t &R = h->ro;
  if (const char *why = npb_minibatch_check(D, h->n_plants, R.t, R.cells, R.n_axes, R.D.n_extras)) return fail(h, NPB_EINVAL, why);
  NPB_USE_DEVICE(h);
  const npb_minibatch_src_t S = {R.D.obs, R.D.act, R.D.extra, R.t, h->n_plants, R.cells, R.n_axes, R.D.n_extras, R.obs_bytes, R.act_bytes};
  npb_launch_minibatch(&S, D, 0, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}
int npb_rollout_minibatch_segments(NpbHandle *h, const npb_minibatch_desc_t *D, int every, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->ro.n_final) return fail_who(h, "npb_rollout_minibatch_segments", g_no_rollout);
  const npb_rollout_t &R = h->ro;
  if (const char *why = npb_minibatch_segments_check(D, every, h->n_plants, R.t, R.cells, R.n_axes, R.D.n_extras)) return fail(h, NPB_EINVAL, why);
  NPB_USE_DEVICE(h);
  const npb_minibatch_src_t S = {R.D.obs, R.D.act, R.D.extra, R.t, h->n_plants, R.cells, R.n_axes, R.D.n_extras, R.obs_bytes, R.act_bytes};
  npb_launch_minibatch(&S, D, every, (hipStream_t)stream);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}

/* ---- episode streams (include/npb.h) */
const char *npb_episode_streams_check(const npb_episode_streams_desc_t *desc, int has_generators, int bank_entries) {
  if (!desc) return nullptr;
  if (!has_generators) return "npb_set_episode_streams: no generators (npb_noise_seed or npb_profile_seed first): there is no stream to restart";
  if (desc->block < 1) return "npb_set_episode_streams: block must be >= 1";
  const bool tables = desc->bank_noise_seeds || desc->bank_profile_seeds;
  if (tables && bank_entries <= 0) return "npb_set_episode_streams: bank seed tables without a start bank (npb_set_start_bank first)";
  if (tables && desc->n_bank_seeds != bank_entries) return "npb_set_episode_streams: n_bank_seeds is not the start bank's entry count";
  for (const int64_t *t : {desc->bank_noise_seeds, desc->bank_profile_seeds})
    for (int s = 0; t && s < desc->n_bank_seeds; s++)
      if (t[s] < 0 || t[s] > (int64_t)0xffffffffLL) return "npb_set_episode_streams: a bank seed is outside [0, 2^32), which numpy.random.RandomState refuses";
  return nullptr;
}

/* every plant's generators of one set back to its own seed: the seeds travel in the pos column (npb_launch_noise_seed) */
static int reseed_own(NpbHandle *h, const npb_noise_t &g, const std::vector<uint32_t> &seeds, hipStream_t st) {
  NPB_HIP(h, hipMemcpyAsync(g.pos, seeds.data(), (size_t)h->n_plants * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  npb_launch_noise_seed(g, h->n_plants, st);
  NPB_HIP(h, hipGetLastError());
  return NPB_OK;
}

int npb_set_episode_streams(NpbHandle *h, const npb_episode_streams_desc_t *desc, void *stream) {
  if (!h) return NPB_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (!desc) {      /* off: every plant's streams from its own seeds again, as npb_noise_seed / npb_profile_seed left them */
    if (!h->es_on) return NPB_OK;
    NPB_USE_DEVICE(h);
    if (h->noise) if (int rc = reseed_own(h, h->noise_g, h->noise_seeds, st)) return rc;
    if (h->prof) {
      if (int rc = reseed_own(h, h->prof_g, h->prof_seeds, st)) return rc;
      NPB_HIP(h, hipMemsetAsync(h->prof_side + (size_t)NPB_PROFILE_CARRIED * h->pitch, 0, (size_t)NPB_PROFILE_NUM_CARRIED * h->pitch * sizeof(double), st));
      h->prof_pos = 0;
    }
    NPB_HIP(h, hipStreamSynchronize(st));      /* nothing may still read the blocks when they are freed */
    (void)hipFree(h->es_mem);
    h->es_mem = nullptr; h->es_on = false; h->es_tables = false; h->es = npb_episode_streams_t{};
    return NPB_OK;
  }
  if (const char *why = npb_episode_streams_check(desc, h->noise || h->prof, h->bank ? h->bank_M : 0)) return fail(h, NPB_EINVAL, why);
  if ((h->noise && h->noise_seeds.empty()) || (h->prof && h->prof_seeds.empty()))
    return fail(h, NPB_EINVAL, "npb_set_episode_streams: the noise generators were only ever loaded (npb_noise_set_state) and have no seed to restart from: npb_noise_seed first");
  if (h->prof && h->ctl.age && h->ctl_axis[NPB_CONTROL_INPUT_POWER_SETPOINT] >= 0)
    return fail(h, NPB_EINVAL, "npb_set_episode_streams: a POWER_SETPOINT axis of the controls fills the setpoint column the profile would drive (npb_set_controls)");
  if (!h->autoreset)
    return fail(h, NPB_EINVAL, "npb_set_episode_streams: needs the autoreset (npb_set_autoreset first): the restarts are read off the episode index it keeps");
  NPB_USE_DEVICE(h);
  if (h->es_on) if (int rc = npb_set_episode_streams(h, nullptr, stream)) return rc;      /* set again: from scratch */
  const size_t n = (size_t)h->n_plants, pitch = h->pitch, block = (size_t)desc->block;
  const bool tables = desc->bank_noise_seeds || desc->bank_profile_seeds;
  const size_t M = tables ? (size_t)desc->n_bank_seeds : 0;
  /* one allocation: the doubles, then the 4-byte columns */
  const size_t doubles = (h->noise ? block * n : 0) + (h->prof ? (3 * block + 1) * n : 0);
  const size_t words = 5 * pitch + 2 * M;
  hipError_t e = hipMalloc(&h->es_mem, doubles * sizeof(double) + words * sizeof(uint32_t));
  if (e != hipSuccess) { h->es_mem = nullptr; return fail(h, NPB_EHIP, "npb_set_episode_streams: hipMalloc of the handle's blocks failed", e); }
  npb_episode_streams_t S = {};
  S.n_plants = h->n_plants; S.block = desc->block; S.pitch = pitch;
  double *d = (double *)h->es_mem;
  if (h->noise) { S.noise = h->noise_g; S.noise_rows = d; d += block * n; }
  if (h->prof) {
    S.prof = h->prof_g; S.prof_side = h->prof_side; S.steps = h->prof_steps;
    S.setpoint_rows = d; d += block * n; S.target_rows = d; d += block * n; S.draws = d; d += (block + 1) * n;
  }
  uint32_t *w = (uint32_t *)d;
  S.position = (int32_t *)w; S.rows_made = (int32_t *)(w + pitch); S.seen_index = (int32_t *)(w + 2 * pitch);
  uint32_t *own_noise = w + 3 * pitch, *own_prof = w + 4 * pitch, *bank_noise = w + 5 * pitch, *bank_prof = w + 5 * pitch + M;
  S.own_noise_seed = own_noise; S.own_profile_seed = own_prof;
  S.episode_index = h->ep_index;
  /* the 4-byte columns as the host lays them out: zeros, the plants' own seeds, the tables */
  std::vector<uint32_t> host(words, 0u);
  for (size_t p = 0; p < n; p++) {
    if (h->noise) host[3 * pitch + p] = h->noise_seeds[p];
    if (h->prof) host[4 * pitch + p] = h->prof_seeds[p];
  }
  for (size_t s = 0; s < M; s++) {
    if (desc->bank_noise_seeds) host[5 * pitch + s] = (uint32_t)desc->bank_noise_seeds[s];
    if (desc->bank_profile_seeds) host[5 * pitch + M + s] = (uint32_t)desc->bank_profile_seeds[s];
  }
  if (tables) { S.bank_entries = (int)M; S.bank_noise_seed = desc->bank_noise_seeds ? bank_noise : nullptr; S.bank_profile_seed = desc->bank_profile_seeds ? bank_prof : nullptr; }
  e = hipMemcpyAsync(w, host.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice, st);
  /* every plant begins both streams anew from its own seed, nothing drawn ahead: the first step that takes a row fills the block */
  if (e == hipSuccess) { npb_launch_episode_streams_restart(&S, S.block, S.block, nullptr, 1, nullptr, st); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipStreamSynchronize(st);      /* host is read until the copy is done */
  if (e != hipSuccess) { (void)hipFree(h->es_mem); h->es_mem = nullptr; return fail(h, NPB_EHIP, "npb_set_episode_streams: seeding the streams failed", e); }
  h->es = S; h->es_on = true; h->es_tables = tables;
  h->es_noise_cur = h->es_prof_cur = S.block;
  h->es_noise_out = desc->noise_out; h->es_setpoint_out = desc->setpoint_out; h->es_target_out = desc->target_out;
  return NPB_OK;
}

int npb_profile_get_positions(NpbHandle *h, int32_t *position, int32_t *rows_made, void *stream) {
  if (!h) return NPB_EINVAL;
  if (!h->es_on) return fail(h, NPB_EINVAL, "npb_profile_get_positions: episode streams are off (npb_set_episode_streams); npb_profile_get_state has the one position");
  if (!h->es.prof.key) return fail(h, NPB_EINVAL, "npb_profile_get_positions: no profile (npb_profile_seed before npb_set_episode_streams)");
  NPB_USE_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  if (position) NPB_HIP(h, hipMemcpyAsync(position, h->es.position, (size_t)h->n_plants * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (rows_made) NPB_HIP(h, hipMemcpyAsync(rows_made, h->es.rows_made, (size_t)h->n_plants * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  NPB_HIP(h, hipStreamSynchronize(st));
  return NPB_OK;
}

int npb_debug_touch(NpbHandle *h, void *stream) {
  if (!h) return NPB_EINVAL;
  if (h->storage != NPB_STORAGE_F64) return fail(h, NPB_EINVAL, "npb_debug_touch: fp64-storage handles only");
  NPB_USE_DEVICE(h);
  npb_launch_touch(NPB_N(h), (double *)h->f64, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, NPB_EHIP, "npb_debug_touch: kernel launch failed", e);
  return NPB_OK;
}

int npb_observe(NpbHandle *h, double *obs, void *stream) {
  if (!h || !obs) return NPB_EINVAL;
  NPB_USE_DEVICE(h);
  h->K->observe(h->params.mode, h->n_plants, NPB_N(h), h->f64, obs, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, NPB_EHIP, "npb_observe: kernel launch failed", e);
  return NPB_OK;
}

} /* extern "C" */

static npb_diag_carried_values_t diag_reference_reset_values() {
  npb_diag_carried_values_t r;
  for (int k = 0; k < NPB_DIAG_NUM_CARRIED; k++) {
    const int row = g_diag_carried[k].row;
    if (row == NPB_DIAG_COND_SJE_COMPRESSION_RATIO || row == NPB_DIAG_COND_SJE_COMPRESSION_RATIO + 1)      /* vacuum_pump.py:551-561: compression_ratio_actual is not among what reset() writes */
      r.v[k] = __builtin_nan("");
    else if (row == NPB_DIAG_STAGE_SYSTEM_EFFICIENCY)
      r.v[k] = 1.0;      /* stage_system.py:1040 (the row reads a 0 as this) */
    else
      r.v[k] = 0.0;      /* rotor_dynamics.py:576-580, :1106-1108; protection_system.py:798-802; vacuum_pump.py:555 */
  }
  return r;
}
