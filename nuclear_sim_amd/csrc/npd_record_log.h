/* npd_record_log.h -- the slot hand-out of the record logs: the maintenance event log (npd_maint_log), the episode records
 * (npb_episode_records_kernel) and the event windows (npb_event_windows_kernel).  Such a log is a uint32 cursor, a capacity and record
 * columns of the caller's.  The wanting lanes of a wave take consecutive slots in plant order through one device-scope atomic; the
 * cursor counts every wanting lane, and a slot at or past the capacity is the caller's to leave unwritten (the host's drain tells an
 * overflow by the count).  Across waves the order is whatever the atomics make it: the drains sort.  Only the reservation is here; the
 * record stores stay in their kernels, but for the maintenance event log's, which several units append to: npd_maint_log below. */
#ifndef NPD_RECORD_LOG_H
#define NPD_RECORD_LOG_H
#include "npb_kernels.h"      /* npd_maint_log_t */

struct npd_log_slots_t { uint32_t base; uint64_t rows; };      /* wave-uniform: the wave's first slot, its wanting lanes */

/* May be called under divergence: the atomic is the first ACTIVE lane's, whether or not it wants, and the base comes back through
 * readfirstlane, which reads that same lane.  Relaxed, agent scope; no atomic when no lane wants. */
__device__ __forceinline__ npd_log_slots_t npd_log_reserve(uint32_t *cursor, bool want) {
  npd_log_slots_t s = {0u, __ballot(want)};
  if (s.rows == 0) return s;
  const uint64_t active = __ballot(1);
  const bool first = __builtin_amdgcn_mbcnt_hi((uint32_t)(active >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)active, 0u)) == 0;
  uint32_t base = 0;
  if (first) base = __hip_atomic_fetch_add(cursor, (uint32_t)__popcll(s.rows), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  s.base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
  return s;
}
/* the slot of `lane`, asked by whichever lane: base + the wanting lanes below it */
__device__ __forceinline__ uint32_t npd_log_slot(npd_log_slots_t s, int lane) { return s.base + (uint32_t)__popcll(s.rows & ((1ull << lane) - 1ull)); }
/* the calling lane's own (mbcnt: no lane index needed, whatever the block's shape) */
__device__ __forceinline__ uint32_t npd_log_slot(npd_log_slots_t s) {
  return s.base + __builtin_amdgcn_mbcnt_hi((uint32_t)(s.rows >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)s.rows, 0u));
}

/* one event site of a wave, possibly inside divergent code: the lanes with `want` take slots of the log; the cursor
 * counts every event, and a slot at or past the capacity is not written */
__device__ __forceinline__ void npd_maint_log(const npd_maint_log_t &L, bool want, const npb_maint_event_t &e) {
  const npd_log_slots_t s = npd_log_reserve(L.cursor, want);
  if (!s.rows) return;
  const uint32_t slot = npd_log_slot(s);
  if (want && slot < (uint32_t)L.capacity) L.records[slot] = e;
}
/* the tail of the npb_operator_*_maint_kernel and of a rule of npb_control_orders_kernel: one record per successful order, stamped with the plant's clock t, one atomic per wave.
 * The caller guards it with `if (L.cursor)`: a run without a log (npb_set_maintenance_log) does not load the clock */
__device__ __forceinline__ void npd_maint_log_operator(const npd_maint_log_t &L, bool ok, size_t p, double t, int unit, int action, int kind, int bearing = 0) {
  npb_maint_event_t ev = {};
  ev.time = t; ev.created = t; ev.planned_start = t; ev.plant = (int32_t)p;
  ev.pump = (uint8_t)unit; ev.action = (uint8_t)action; ev.kind = (uint8_t)kind; ev.bearing = (uint8_t)bearing;
  npd_maint_log(L, ok, ev);
}
#endif
