/* npd_normalizer.h -- running observation and reward normalisation (npb_set_normalizer, include/npb.h): the partials kernel of one fold and
 * the reward kernel.  nuclear_sim_amd/normalizer.py states the fold in numpy; these kernels and the finish kernel (npb_minibatch.hip,
 * which divides and takes the root under IEEE flags) produce its bits.
 *
 * Partials kernel.  One workgroup of 256 takes 256 consecutive plants: ONE group of the pinned tree (npb_minibatch.h), so the workgroup
 * count is the tree's and not a tunable.  A lane reads its plant's raw sample of up to NPD_NORM_CHUNK streams before the first of them is
 * used -- npd_column_read through NPD_SEGMENT (applied per wave: a segment is a whole number of waves), consecutive lanes on consecutive plants, sixteen loads in flight as the features kernel
 * asks for its columns; the streams' descriptors and the running shift are uniform over the launch: scalar loads.  d = x - shift and q =
 * d * d are each rounded (-ffp-contract=off); a sample counts iff q - q == 0.0, else it contributes +0.0, +0.0 and no count, and so does
 * a lane past n_plants.  There is no division and no root here, so the step's -freciprocal-math / -fapprox-func do no harm.
 * d and q of NPD_NORM_PASS streams go to LDS, 2 x 8 rows of 256 doubles, and npd_tree_groups runs the halving over all sixteen rows
 * together: eight barriers a pass, not eight a stream.  The counts go by ballot and popcount, a wave each, and through four words of LDS.
 * Row stride: a row is 256 doubles = 2 KiB = eight whole bank rows (64 banks x 4 bytes; ds_read_b64 banks modulo 64 dwords, the stores
 * modulo 32), so with a stride of 256 the rows' k-th elements all share a bank: harmless while a wave's lanes walk ONE row (half >= 64:
 * consecutive lanes on consecutive doubles), but the last levels put a wave's lanes on the same few elements of sixteen rows, sixteen ways
 * on one bank.  NPD_NORM_STRIDE = 257 moves each row by one double: the sixteen rows' first elements lie on sixteen bank pairs, and the
 * levels between meet at most two ways.  33 KiB of LDS.
 * The result is partial[3 * stream + {s1, s2, count}][group] (the count as a double: integers, exact in any order).
 * With the return stream (the last stream) the same kernel forms ret[p] = (carry ? ret * gamma : 0.0) + r, stores it, and folds it.
 *
 * Reward kernel, behind the finish, one lane per plant: norm_reward = clip(r * rscale), ended, primed, seen; frozen, when the partials
 * kernel has not run, it carries ret itself.  It reads nothing of the arena and is compiled once (npb_storage_free.hip).
 * No atomics, no scratch.
 * NOT here (include/npb.h says so too): statistics over fresh frames, per-plant statistics, an exponential moving average, half types,
 * synchronising shards on the device, BITS or setpoint-error columns. */
#ifndef NPD_NORMALIZER_H
#define NPD_NORMALIZER_H
#include "npb_minibatch.h"

#define NPD_NORM_CHUNK 16      /* streams whose samples a lane asks for together */
#define NPD_NORM_PASS 8        /* streams whose d and q stand in LDS together */

__global__ __launch_bounds__(NPD_TREE) void npb_normalizer_partials_kernel(const npd_real_t *__restrict__ f64, size_t N, npb_normalizer_t Z, int n_plants,
                                                                           const int32_t *__restrict__ index, const double *__restrict__ reward) {
  __shared__ double rows[2 * NPD_NORM_PASS * NPD_NORM_STRIDE];
  __shared__ int counted[NPD_NORM_PASS][NPD_TREE / NPB_WAVE];
  const int lane = threadIdx.x, S = Z.n_streams, C = Z.n_cols;
  const size_t block_base = (size_t)blockIdx.x * NPD_TREE;
  /* per WAVE, as the task and the features take it: a segment is a whole number of waves (npb_create: a multiple of 64), not of groups of
   * 256 -- the four waves of a workgroup may lie in four segments */
  NPD_SEGMENT(f64, N, block_base + (size_t)(lane & ~(NPB_WAVE - 1)));
  const size_t p = block_base + lane;
  const bool here = p < (size_t)n_plants;
  for (int c0 = 0; c0 < S; c0 += NPD_NORM_CHUNK) {
    double x[NPD_NORM_CHUNK];
#pragma unroll
    for (int j = 0; j < NPD_NORM_CHUNK; j++) {
      x[j] = 0.0;
      if (here && c0 + j < C) x[j] = npd_column_read<const npb_colstat_col_t &>(f64, N, p, Z.streams[c0 + j].c);
    }
    if (here && Z.reward_on && S - 1 >= c0 && S - 1 < c0 + NPD_NORM_CHUNK) {      /* the return stream: formed, stored, folded */
      const double ret = npd_normalizer_return(Z, p, index, reward[p]);
      Z.ret[p] = ret;
#pragma unroll
      for (int j = 0; j < NPD_NORM_CHUNK; j++)
        if (c0 + j == S - 1) x[j] = ret;
    }
#pragma unroll
    for (int h0 = 0; h0 < NPD_NORM_CHUNK; h0 += NPD_NORM_PASS) {
      if (c0 + h0 >= S) break;      /* (uniform) */
      __syncthreads();              /* (the rows and counts of the pass before have been read) */
#pragma unroll
      for (int j = 0; j < NPD_NORM_PASS; j++) {
        const int c = c0 + h0 + j;
        double d = 0.0, q = 0.0;
        bool counts = false;
        if (c < S) {      /* (uniform) */
          const double shift = Z.count[c] > 0.0 ? Z.mean[c] : Z.streams[c].ref0;
          d = x[h0 + j] - shift;
          q = d * d;
          counts = here && q - q == 0.0;
          if (!counts) { d = 0.0; q = 0.0; }
        }
        rows[(2 * j) * NPD_NORM_STRIDE + lane] = d;
        rows[(2 * j + 1) * NPD_NORM_STRIDE + lane] = q;
        const uint64_t who = __ballot(counts);
        if ((lane & (NPB_WAVE - 1)) == 0) counted[j][lane / NPB_WAVE] = __popcll(who);
      }
      npd_tree_groups<2 * NPD_NORM_PASS>(rows, NPD_NORM_STRIDE, lane);
      if (lane < 3 * NPD_NORM_PASS) {      /* lanes 0 .. 15: a row's sum each; 16 .. 23: a stream's count */
        const int j = lane < 2 * NPD_NORM_PASS ? lane >> 1 : lane - 2 * NPD_NORM_PASS, c = c0 + h0 + j;
        if (c < S) {
          double value;
          if (lane < 2 * NPD_NORM_PASS) value = rows[lane * NPD_NORM_STRIDE];
          else value = (double)(counted[j][0] + counted[j][1] + counted[j][2] + counted[j][3]);
          const int part = lane < 2 * NPD_NORM_PASS ? (lane & 1) : 2;
          Z.partial[(size_t)(3 * c + part) * Z.ws_stride + blockIdx.x] = value;
        }
      }
    }
  }
}
static void NPB_LAUNCHER(normalizer)(const void *arena, size_t npad, const npb_normalizer_t *Z, int n_plants, const int32_t *index, const double *reward,
                                     hipStream_t stream) {
  const dim3 grid((unsigned)((n_plants + NPD_TREE - 1) / NPD_TREE)), block(NPD_TREE);
  hipLaunchKernelGGL(npb_normalizer_partials_kernel, grid, block, 0, stream, (const npd_real_t *)arena, npad, *Z, n_plants, index, reward);
}
#endif
