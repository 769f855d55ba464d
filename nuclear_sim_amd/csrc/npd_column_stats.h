/* npd_column_stats.h -- per-plant column statistics (npb_set_column_stats, include/npb.h): one sample of each chosen column of every plant,
 * folded behind every step into min / max / sum / sum of squares / last value / first time beyond a limit / samples beyond it, per (column,
 * plant).  nuclear_sim_amd/colstats.py states the fold in numpy; this file produces its bits (sequential adds in step order, the square
 * rounded before its add: -ffp-contract=off).
 *
 * One launch, grid (ceil(n / NPD_COLSTAT_BLOCK), n_cols), a thread per (column, plant) cell, as npb_sample_kernel lays a sample out: the
 * column's descriptor is uniform over the block (scalar loads), consecutive lanes are consecutive plants, so the value and every table row
 * coalesce (a side row with a plant stride, such as an info column, costs what that stride costs).  A cell belongs to one thread and folds
 * are ordered by the stream: no atomics, no LDS.  min / max / first_beyond are stored only when they change; the plant clock is read only
 * on the step a cell first goes beyond its limit.  Part of npb_attachments.hip, compiled for either
 * storage type: it reads the arena.  The clear kernel does not: npb_storage_free.hip. */
#ifndef NPD_COLUMN_STATS_H
#define NPD_COLUMN_STATS_H

__global__ __launch_bounds__(NPD_COLSTAT_BLOCK) void npb_column_stats_fold_kernel(const npd_real_t *__restrict__ f64, size_t N, npb_column_stats_t S,
                                                                                  int n_plants) {
  const int c = blockIdx.y;
  const size_t p = (size_t)blockIdx.x * NPD_COLSTAT_BLOCK + threadIdx.x;
  if (p >= (size_t)n_plants) return;
  const npb_colstat_col_t C = S.cols[c];
  NPD_SEGMENT(f64, N, p);
  const double v = npd_column_read<npb_colstat_col_t>(f64, N, p, C);
  const size_t cell = (size_t)c * (size_t)n_plants + p;
  if (S.min && v < S.min[cell]) S.min[cell] = v;      /* (a NaN sample compares false: it replaces neither) */
  if (S.max && v > S.max[cell]) S.max[cell] = v;
  if (S.sum) S.sum[cell] = S.sum[cell] + v;
  if (S.sumsq) { const double sq = v * v; S.sumsq[cell] = S.sumsq[cell] + sq; }
  if (S.last) S.last[cell] = v;
  if (C.direction != 0 && (C.direction > 0 ? v > C.limit : v < C.limit)) {
    if (S.n_beyond) S.n_beyond[cell] += 1;
    if (S.first_beyond && S.first_beyond[cell] == NPD_COLSTAT_POS_INF)      /* the first time: the plant's clock after this step */
      S.first_beyond[cell] = NPD_F64_COL(PRIM, npb_prim_t, sim_time, 0);
  }
  if (c == 0) S.n_samples[p] += 1;
}
static void NPB_LAUNCHER(column_stats_fold)(const void *arena, size_t npad, const npb_column_stats_t *S, int n_plants, hipStream_t stream) {
  hipLaunchKernelGGL(npb_column_stats_fold_kernel, dim3((unsigned)((n_plants + NPD_COLSTAT_BLOCK - 1) / NPD_COLSTAT_BLOCK), (unsigned)S->n_cols),
                     dim3(NPD_COLSTAT_BLOCK), 0, stream, (const npd_real_t *)arena, npad, *S, n_plants);
}
#endif
