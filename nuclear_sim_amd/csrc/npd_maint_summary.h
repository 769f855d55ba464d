/* npd_maint_summary.h -- the per-plant work-order summary (npb_set_maintenance_summary, include/npb_maint.h): the maintenance event log
 * folded into first-created / first-completed times and created / completed counts per (key, plant).  What the data-gen runner returns of a
 * finished scenario (maintenance_scenario_runner.py:431-468) and what the timing optimiser reads of a probe run (timing_optimizer.py:273-320),
 * kept on the device.  The same for either storage type: a record's time is fp64 under both (compiled once, npb_storage_free.hip).
 *
 * One launch of a fixed grid: the host does not know the cursor, so every thread reads the two device words that bound the fold and strides
 * over the records between them.  Counts move by integer atomic adds, times by an unsigned 64-bit atomic minimum on the double's bit pattern
 * (valid because every plant clock is >= +0.0: include/npb_maint.h), so the tables are a function of the set of records, not of their order.
 * The cursor and the bookkeeping words are rewritten by the last block to finish: each block takes one ticket from an atomic counter after its
 * threads have read their records, and the block that draws the last ticket writes.  No block waits for another and nothing spins. */
#ifndef NPD_MAINT_SUMMARY_H
#define NPD_MAINT_SUMMARY_H

#define NPD_SUMMARY_BLOCK 256
#define NPD_SUMMARY_MAX_BLOCKS 64
#define NPD_SUMMARY_INF_BITS 0x7ff0000000000000ull

/* the summary as the fold kernel takes it: the descriptor, the log it folds and the handle's ticket word (zero between folds) */
struct npd_maint_summary_t {
  npb_maint_summary_desc_t D;
  npd_maint_log_t L;
  uint32_t *ticket;
  int n_plants;
};

/* the catalog a record's kind belongs to; -1 for a kind this build does not know */
__device__ __forceinline__ int npd_summary_catalog_of(unsigned kind) {
  if (kind <= NPB_MAINT_EVENT_OPERATOR) return NPB_MAINT_CATALOG_FEEDWATER;
  if (kind == NPB_MAINT_EVENT_OPERATOR_TURBINE) return NPB_MAINT_CATALOG_TURBINE;
  return kind <= NPB_MAINT_EVENT_COMPONENT_COMPLETED ? NPB_MAINT_CATALOG_COMPONENT : -1;
}

__global__ __launch_bounds__(NPD_SUMMARY_BLOCK) void npb_maint_summary_fold_kernel(npd_maint_summary_t S) {
  /* the range: every thread of every block reads both words before any block can rewrite them (the writer holds the last ticket) */
  const uint32_t cursor = *(volatile const uint32_t *)S.L.cursor, folded = *(volatile const uint32_t *)S.D.folded;
  const uint32_t cap = (uint32_t)S.L.capacity;
  const uint32_t hi = cursor < cap ? cursor : cap, lo = folded < hi ? folded : hi;
  uint64_t *const first_created = (uint64_t *)S.D.first_created, *const first_completed = (uint64_t *)S.D.first_completed;
  for (uint32_t r = lo + blockIdx.x * NPD_SUMMARY_BLOCK + threadIdx.x; r < hi; r += gridDim.x * NPD_SUMMARY_BLOCK) {
    const npb_maint_event_t *e = S.L.records + r;
    const double time = e->time;
    const int plant = e->plant;
    const unsigned kind = e->kind;
    const int action = e->action, unit = e->pump;
    const int catalog = npd_summary_catalog_of(kind);
    if (time < S.D.since_minutes || plant < 0 || plant >= S.n_plants || catalog < 0) continue;
    const bool creation = (NPB_MAINT_CREATION_KINDS >> kind) & 1u;
    const uint64_t bits = (uint64_t)__double_as_longlong(time);
    for (int j = 0; j < S.D.n_keys; j++) {      /* (the keys are kernel arguments: uniform, scalar loads) */
      const npb_maint_summary_key_t K = S.D.keys[j];
      if (K.catalog != catalog || !((K.kinds >> kind) & 1u) || (K.action >= 0 && K.action != action) || (K.unit >= 0 && K.unit != unit)) continue;
      const size_t cell = (size_t)j * (size_t)S.n_plants + (size_t)plant;
      __hip_atomic_fetch_add((creation ? S.D.n_created : S.D.n_completed) + cell, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_min((creation ? first_created : first_completed) + cell, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  /* the tail: the block that draws the last ticket rewrites the words, after every block's record reads */
  __syncthreads();
  if (threadIdx.x != 0) return;
  const uint32_t ticket = __hip_atomic_fetch_add(S.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (ticket != gridDim.x - 1) return;
  const uint32_t over = cursor > cap ? cursor - cap : 0u;
  if (S.D.consume) {
    if (over) *S.D.dropped += over;
    *S.L.cursor = 0u;
    *S.D.folded = 0u;
  } else {
    *S.D.folded = hi;
    *S.D.dropped = over;
  }
  __hip_atomic_store(S.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* npb_maint_summary_clear: the rows of the plants of mask (NULL = all) back to "never" and 0, one grid row per key */
__global__ void npb_maint_summary_clear_kernel(npb_maint_summary_desc_t D, const uint8_t *__restrict__ mask, int n_plants) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (p >= n_plants || (mask && !mask[p])) return;
  const size_t cell = (size_t)j * (size_t)n_plants + (size_t)p;
  ((uint64_t *)D.first_created)[cell] = NPD_SUMMARY_INF_BITS;
  ((uint64_t *)D.first_completed)[cell] = NPD_SUMMARY_INF_BITS;
  D.n_created[cell] = 0;
  D.n_completed[cell] = 0;
}

/* the grid is fixed by the log's capacity (known to the host), never by its fill: a block per NPD_SUMMARY_BLOCK records the log can hold,
 * NPD_SUMMARY_MAX_BLOCKS at the most -- a quiet fold is one small launch */
extern "C" void npb_launch_maint_summary_fold(const npb_maint_summary_desc_t *D, npd_maint_log_t L, uint32_t *ticket, int n_plants, hipStream_t stream) {
  npd_maint_summary_t S;
  S.D = *D; S.L = L; S.ticket = ticket; S.n_plants = n_plants;
  int blocks = (L.capacity + NPD_SUMMARY_BLOCK - 1) / NPD_SUMMARY_BLOCK;
  blocks = blocks < 1 ? 1 : blocks > NPD_SUMMARY_MAX_BLOCKS ? NPD_SUMMARY_MAX_BLOCKS : blocks;
  hipLaunchKernelGGL(npb_maint_summary_fold_kernel, dim3((unsigned)blocks), dim3(NPD_SUMMARY_BLOCK), 0, stream, S);
}
extern "C" void npb_launch_maint_summary_clear(const npb_maint_summary_desc_t *D, const uint8_t *mask, int n_plants, hipStream_t stream) {
  hipLaunchKernelGGL(npb_maint_summary_clear_kernel, dim3((unsigned)((n_plants + 255) / 256), (unsigned)D->n_keys), dim3(256), 0, stream, *D, mask, n_plants);
}
#endif
