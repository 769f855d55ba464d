/* npd_event_windows.h -- state windows around events (npb_set_event_windows, include/npb.h): every plant keeps the last H = pre + 1 + post
 * samples of a few columns in a ring on the device; a trigger (rising bits, an increase, a limit crossed) arms a capture, and `post` steps
 * later -- or when the episode ends first -- the window goes into a record of the caller's.  nuclear_sim_amd/eventwin.py states it in
 * numpy; the window is copies, so this file produces its bits.
 *
 * One launch behind every step, one wave per 64 plants.  Ring row step % H is the same for the whole batch: every ring store, every
 * bookkeeping column and every trigger source is read and written with consecutive lanes on consecutive plants.  A wave first asks for
 * everything it reads and stores afterwards (the kernel is bound by latency, not by bytes).  The descriptors (columns,
 * triggers) are uniform over the launch: scalar loads.  A wave none of whose lanes captures ends there.  Otherwise its capturing lanes take
 * consecutive slots in plant order with one atomic add (npd_record_log.h), and for each of them in turn all 64
 * lanes copy its window: the reads walk the ring with the plant stride (one line per element, whoever reads them), the stores into
 * `values` are contiguous.  No LDS.  Part of npb_attachments.hip, compiled for either storage type: it
 * reads the arena.  The clear kernel does not: npb_storage_free.hip. */
#ifndef NPD_EVENT_WINDOWS_H
#define NPD_EVENT_WINDOWS_H

#define NPD_EVW_NAN __longlong_as_double(0x7ff8000000000000ll)

__global__ __launch_bounds__(NPB_WAVE) void npb_event_windows_kernel(const npd_real_t *__restrict__ f64, size_t N, npb_event_windows_t W, int n_plants,
                                                                     int step, const int32_t *__restrict__ index, const int32_t *__restrict__ len,
                                                                     const uint8_t *__restrict__ done, int max_steps) {
  const size_t block_base = (size_t)blockIdx.x * NPB_WAVE;
  NPD_SEGMENT(f64, N, block_base);
  const int lane = threadIdx.x;
  const size_t p = block_base + lane, n = (size_t)n_plants;
  const int H = W.pre + 1 + W.post, stride = W.n_cols + 1;
  bool capture = false, early = false;
  int32_t a_step = 0, a_n_pre = 0, a_n_post = 0, episode = 0;
  if (p < n) {
    int32_t valid = W.valid[p], due = W.due[p];      /* valid == 0: unprimed; due < 0: idle */
    if (index) {      /* 1. restarted since the last sample: an empty ring, and an armed capture abandoned */
      episode = index[p];
      if (episode != W.seen[p]) { W.seen[p] = episode; valid = 0; due = -1; }
    }
    /* 2. and 3., the loads: every recorded column, the clock, every trigger source and its previous value are asked for before the first of
     * them is stored.  At one wave per SIMD (1024 waves at 65 536 plants) nothing else hides a load's latency, and a loop that loads and
     * stores column by column pays it once per column.  Unrolled over the maxima with wave-uniform guards: the arrays stay in registers */
    double v[NPB_EVENT_WINDOW_COLS_MAX], tv[NPB_EVENT_WINDOW_TRIGGERS_MAX], pv[NPB_EVENT_WINDOW_TRIGGERS_MAX];
#pragma unroll
    for (int c = 0; c < NPB_EVENT_WINDOW_COLS_MAX; c++) v[c] = c < W.n_cols ? npd_column_read<const npb_colstat_col_t &>(f64, N, p, W.cols[c]) : 0.0;
    const double clock = NPD_F64_COL(PRIM, npb_prim_t, sim_time, 0);
#pragma unroll
    for (int t = 0; t < NPB_EVENT_WINDOW_TRIGGERS_MAX; t++) {
      tv[t] = pv[t] = 0.0;
      if (t < W.n_triggers) { tv[t] = npd_column_read<const npb_colstat_col_t &>(f64, N, p, W.triggers[t].c); pv[t] = W.prev[(size_t)t * n + p]; }
    }
    /* 2. the sample into ring row step % H */
    double *row = W.ring + (size_t)(step % H) * stride * n + p;
#pragma unroll
    for (int c = 0; c < NPB_EVENT_WINDOW_COLS_MAX; c++) if (c < W.n_cols) row[(size_t)c * n] = v[c];
    row[(size_t)W.n_cols * n] = clock;
    const bool primed = valid > 0;
    valid = valid < H ? valid + 1 : H;
    W.valid[p] = valid;
    /* 3. the triggers against the previous sample */
    uint32_t fired = 0;
#pragma unroll
    for (int t = 0; t < NPB_EVENT_WINDOW_TRIGGERS_MAX; t++) {
      if (t >= W.n_triggers) break;
      const npb_event_trigger_col_t T = W.triggers[t];
      W.prev[(size_t)t * n + p] = tv[t];
      if (!primed) continue;
      bool f;
      if (T.mode == NPB_TRIGGER_MODE_BITS_RISE) f = (((uint32_t)(int32_t)tv[t] & T.mask) & ~((uint32_t)(int32_t)pv[t] & T.mask)) != 0u;
      else if (T.mode == NPB_TRIGGER_MODE_INCREASE) f = tv[t] > pv[t];      /* (a NaN on either side compares false) */
      else f = T.c.direction > 0 ? (tv[t] > T.c.limit && !(pv[t] > T.c.limit)) : (tv[t] < T.c.limit && !(pv[t] < T.c.limit));
      if (f) fired |= 1u << t;
    }
    /* 4. arm, or count a trigger that finds the plant armed */
    if (fired) {
      if (due < 0) {
        due = step + W.post;
        W.a_step[p] = step; W.a_n_pre[p] = W.pre < valid - 1 ? W.pre : valid - 1; W.a_trigger[p] = __ffs((int)fired) - 1; W.a_fired[p] = fired;
        W.a_retriggers[p] = 0; W.a_time[p] = clock;
      } else {
        W.a_retriggers[p] += 1;
      }
    }
    /* 5. due, or the episode ends first (npb_episode_kernel's rule, behind this kernel on the same columns) */
    if (due >= 0) {
      a_step = W.a_step[p];
      if (step == due) { capture = true; a_n_post = W.post; }
      else if (len && ((done && done[p] != 0) || (max_steps > 0 && len[p] + 1 >= max_steps))) { capture = early = true; a_n_post = step - a_step; }
      if (capture) { a_n_pre = W.a_n_pre[p]; due = -1; }
    }
    W.due[p] = due;
  }
  const npd_log_slots_t s = npd_log_reserve(W.D.cursor, capture);      /* the capturing lanes' slots (npd_record_log.h) */
  if (!s.rows) return;
  const uint32_t cap = (uint32_t)W.D.capacity;
  const uint32_t slot = npd_log_slot(s);
  if (capture && slot < cap) {
    W.D.plant[slot] = (int32_t)p;
    W.D.episode[slot] = episode;
    W.D.trigger[slot] = W.a_trigger[p];
    W.D.step[slot] = a_step;
    W.D.n_pre[slot] = a_n_pre;
    W.D.n_post[slot] = a_n_post;
    W.D.flags[slot] = early ? 1 : 0;
    W.D.retriggers[slot] = W.a_retriggers[p];
    W.D.fired[slot] = W.a_fired[p];
    W.D.time[slot] = W.a_time[p];
  }
  /* the windows, one captured lane after the other, all 64 lanes copying: row k of a record is sample a_step + k - pre */
  const int cells = H * stride;
  for (uint64_t left = s.rows; left; left &= left - 1) {
    const int r = __ffsll((unsigned long long)left) - 1;
    const uint32_t slot_r = npd_log_slot(s, r);
    if (slot_r >= cap) break;      /* (slots rise with the lane: the rest did not fit either) */
    const int first = __shfl(a_step, r) - W.pre, lo = W.pre - __shfl(a_n_pre, r), hi = W.pre + __shfl(a_n_post, r);
    const double *from = W.ring + (block_base + (size_t)r);
    double *values = W.D.values + (size_t)slot_r * H * W.n_cols, *times = W.D.times + (size_t)slot_r * H;
    for (int i = lane; i < cells; i += NPB_WAVE) {
      const int k = i / stride, c = i - k * stride;
      double v = NPD_EVW_NAN;
      if (k >= lo && k <= hi) v = from[((size_t)((first + k) % H) * stride + c) * n];
      if (c < W.n_cols) values[k * W.n_cols + c] = v; else times[k] = v;
    }
  }
}
static void NPB_LAUNCHER(event_windows)(const void *arena, size_t npad, const npb_event_windows_t *W, int n_plants, int step, const int32_t *index,
                                        const int32_t *len, const uint8_t *done, int max_steps, hipStream_t stream) {
  hipLaunchKernelGGL(npb_event_windows_kernel, dim3((unsigned)((n_plants + NPB_WAVE - 1) / NPB_WAVE)), dim3(NPB_WAVE), 0, stream,
                     (const npd_real_t *)arena, npad, *W, n_plants, step, index, len, done, max_steps);
}
#endif
