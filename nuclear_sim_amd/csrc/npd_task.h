/* npd_task.h -- the caller's reward terms and termination rules (npb_set_task, include/npb.h): behind every step each plant's task reward,
 * termination flag and cause word are formed from the end-of-step state and the step's outputs, and everything downstream that deals with
 * episodes (column statistics, event windows, episode records, the episode kernel) reads them in place of the step's reward and done.
 * nuclear_sim_amd/task.py states the evaluation in numpy; this file produces its bits: every product is rounded before its add
 * (-ffp-contract=off), the sum runs in term order, the terminal rewards follow in rule order.
 *
 * One launch behind the step, the rule and the summary fold; one thread per plant, one wave per 64 plants, consecutive lanes on
 * consecutive plants in every column read and written.  The descriptors (terms, rules) are uniform over the launch: scalar loads.  A
 * thread first asks for everything it reads -- every term's column, its second column, its previous sample, every rule's column, the
 * bookkeeping words -- and stores afterwards: at one wave per SIMD nothing else hides a load's latency (npd_event_windows.h).  The loops
 * are unrolled over the maxima with wave-uniform guards, so the arrays stay in registers.  No LDS, no atomics.  Part of
 * npb_attachments.hip, compiled for either storage type: it reads the arena. */
#ifndef NPD_TASK_H
#define NPD_TASK_H

__device__ __forceinline__ bool npd_task_beyond(double v, int direction, double limit) { return direction > 0 ? v > limit : v < limit; }

__global__ __launch_bounds__(NPB_WAVE) void npb_task_kernel(const npd_real_t *__restrict__ f64, size_t N, npb_task_t T, int n_plants,
                                                            const int32_t *__restrict__ index) {
  const size_t block_base = (size_t)blockIdx.x * NPB_WAVE;
  NPD_SEGMENT(f64, N, block_base);
  const size_t p = block_base + threadIdx.x, n = (size_t)n_plants;
  if (p >= n) return;
  /* 1. the loads, all of them before the first store */
  int32_t primed = T.primed[p];
  const int32_t seen = T.seen[p], episode = index ? index[p] : seen;
  double v[NPB_TASK_TERMS_MAX], ref[NPB_TASK_TERMS_MAX], pv[NPB_TASK_TERMS_MAX], rv[NPB_TASK_RULES_MAX];
#pragma unroll
  for (int t = 0; t < NPB_TASK_TERMS_MAX; t++) {
    v[t] = ref[t] = pv[t] = 0.0;
    if (t < T.n_terms) {
      v[t] = npd_column_read<const npb_colstat_col_t &>(f64, N, p, T.terms[t].c);
      ref[t] = T.terms[t].ref_col ? npd_column_read<const npb_colstat_col_t &>(f64, N, p, T.terms[t].r) : T.terms[t].ref;
      if (T.terms[t].prev_row >= 0) pv[t] = T.prev[(size_t)T.terms[t].prev_row * n + p];
    }
  }
#pragma unroll
  for (int r = 0; r < NPB_TASK_RULES_MAX; r++) rv[r] = r < T.n_rules ? npd_column_read<const npb_colstat_col_t &>(f64, N, p, T.rules[r].c) : 0.0;
  if (episode != seen) primed = 0;      /* restarted since the last sample (autoreset, npb_restore*, npb_reset*): the event windows' rule */
  /* 2. the terms: reward = bias + w_0 * f_0 + ..., sequentially, each product rounded before its add */
  double reward = T.bias, wf[NPB_TASK_TERMS_MAX];
#pragma unroll
  for (int t = 0; t < NPB_TASK_TERMS_MAX; t++) {
    wf[t] = 0.0;
    if (t >= T.n_terms) continue;
    const int kind = T.terms[t].kind, direction = T.terms[t].c.direction;
    const double limit = T.terms[t].c.limit, d = v[t] - ref[t];
    double f;
    if (kind == NPB_TASK_VALUE) f = v[t];
    else if (kind == NPB_TASK_ABS_ERR) f = fabs(d);
    else if (kind == NPB_TASK_SQ_ERR) f = d * d;
    else if (kind == NPB_TASK_BEYOND) f = npd_task_beyond(v[t], direction, limit) ? 1.0 : 0.0;
    else if (kind == NPB_TASK_EXCESS) f = !npd_task_beyond(v[t], direction, limit) ? 0.0 : direction > 0 ? v[t] - limit : limit - v[t];
    else if (kind == NPB_TASK_BITS) f = ((uint32_t)(int32_t)v[t] & T.terms[t].mask) != 0u ? 1.0 : 0.0;
    else f = primed ? v[t] - pv[t] : 0.0;      /* NPB_TASK_DELTA */
    wf[t] = T.terms[t].w * f;
    reward = reward + wf[t];
  }
  /* 3. the rules: levels, a bit each; the terminal rewards of those that fired behind the terms, in rule order */
  uint32_t cause = 0;
#pragma unroll
  for (int r = 0; r < NPB_TASK_RULES_MAX; r++) {
    if (r >= T.n_rules) break;
    const int mode = T.rules[r].mode;
    bool fired;
    if (mode == NPB_TASK_RULE_MODE_BITS_ANY) fired = ((uint32_t)(int32_t)rv[r] & T.rules[r].mask) != 0u;
    else if (mode == NPB_TASK_RULE_MODE_BEYOND) fired = npd_task_beyond(rv[r], T.rules[r].c.direction, T.rules[r].c.limit);
    else fired = !(fabs(rv[r]) <= __longlong_as_double(0x7fefffffffffffffll));      /* NPB_TASK_RULE_MODE_NONFINITE: DBL_MAX */
    if (fired) { cause |= 1u << r; reward = reward + T.rules[r].terminal; }
  }
  /* 4. the stores: nothing above them has stored, so no descriptor is read twice */
#pragma unroll
  for (int t = 0; t < NPB_TASK_TERMS_MAX; t++) {
    if (t >= T.n_terms) break;
    if (T.terms_out) T.terms_out[(size_t)t * n + p] = wf[t];
    if (T.terms[t].prev_row >= 0) T.prev[(size_t)T.terms[t].prev_row * n + p] = v[t];
  }
  T.reward[p] = reward;
  T.done[p] = cause != 0u ? 1 : 0;
  if (T.cause) T.cause[p] = cause;
  T.primed[p] = 1;
  T.seen[p] = episode;
}
static void NPB_LAUNCHER(task)(const void *arena, size_t npad, const npb_task_t *T, int n_plants, const int32_t *index, hipStream_t stream) {
  hipLaunchKernelGGL(npb_task_kernel, dim3((unsigned)((n_plants + NPB_WAVE - 1) / NPB_WAVE)), dim3(NPB_WAVE), 0, stream,
                     (const npd_real_t *)arena, npad, *T, n_plants, index);
}
#endif
