/* npb_minibatch.hip -- between npb_rollout_advantages and the optimiser (include/npb.h): the advantages' moments with the order of every
 * addition pinned, a keyed permutation computed entry by entry, and the gather of one minibatch in one launch.
 * nuclear_sim_amd/rollout.py states them in numpy; this file produces its bits.  It is built with the noise generator's flags, without
 * -freciprocal-math / -fapprox-func: the divisions (mean, var, the normalisation) and the root are IEEE, and with -ffp-contract=off the
 * square is rounded before it is added.
 *
 * moments: the statement's expression tree is a serial chain down every column and then a tree of groups of 256 over the columns, so the
 *   schedule follows it: one lane per column, consecutive lanes on consecutive columns, the loads of NPD_MOMENTS_AHEAD rows issued before
 *   their additions run (as npb_rollout_advantages_kernel does with its slots); the workgroup of 256 IS one group of the tree's first
 *   level: 128 .. 1 in LDS, one partial per workgroup.  The finish kernel, one workgroup, repeats the group tree over the partials level
 *   by level and then divides (and, behind the second pass, takes the root).  The workgroup count is the tree's, not a tunable.
 * permutation: one lane per entry, the keys by value.
 * minibatch: a wave per NPD_MINIBATCH_ROWS output rows (and, for whole sequences, per slot).  Phase 1, one lane per row: the source
 *   index by the walk, then index, adv and ret with consecutive lanes on consecutive outputs.  Phase 2: the wave walks its rows, L lanes on each, the source
 *   index of a row taken by __shfl from the lane that computed it; the loads of NPD_MINIBATCH_AHEAD passes are issued before their stores.
 *   A tensor's width (16 bytes, else one element) and L are the launcher's, as npb_launch_rollout_post picks W; they are uniform in the
 *   launch, so one kernel serves every shape.  Segments of `every` slots (npb_rollout_minibatch_segments) are sequences of `every` slots whose
 *   source starts `c * every` slots down: an entry c * n_plants + p is turned into that cell once, behind the store of index.
 * No atomics, no scratch, nothing of the arena. */
#include <hip/hip_runtime.h>
#include <math.h>
#include "npb_minibatch.h"
#include "npb_kernels.h"

#define NPD_MOMENTS_AHEAD 8          /* rows whose loads are in flight before their additions run */
/* output rows a wave takes, and passes over them whose loads are in flight before their stores.  Measured on an MI355X (kernel trace,
 * 65 536 transitions of 256-byte stacks, 16-byte actions and 8-byte extras out of 8.4 M): 64 rows 17.6 us, 32 rows 15.9, 16 rows 15.9;
 * 8 passes ahead in place of 4: 17.1, 16.7, 16.5 -- the gather runs at the rate random 256-byte rows come in, not at a wave's latency */
#define NPD_MINIBATCH_ROWS 32
#define NPD_MINIBATCH_AHEAD 4
#define NPD_MINIBATCH_BLOCKS 8192    /* workgroups of 4 waves a launch has at most; the waves stride over the tiles */
#define NPD_WAVE 64

/* ---------------------------------------------------------------------------------------------------------------- moments */
/* (the tree itself: npd_tree_group and npd_tree_levels, npb_minibatch.h) */
/* SQUARES = false: col[p] = sum of (double)x[s][p]; true: of the rounded squares of (double)x[s][p] - stats[1].  partial[block] = that
 * workgroup's group of the tree; a tensor of one column has no tree: partial[0] = col[0] */
template <typename T, bool SQUARES>
__global__ __launch_bounds__(NPD_TREE) void npb_moments_columns_kernel(const T *__restrict__ x, size_t rows, size_t cols, const double *__restrict__ stats,
                                                                      double *__restrict__ partial) {
  __shared__ double s[NPD_TREE];
  const int lane = threadIdx.x;
  const size_t p = (size_t)blockIdx.x * NPD_TREE + lane;
  const double mean = SQUARES ? stats[1] : 0.0;
  double acc = 0.0;
  if (p < cols) {
    const T *col = x + p;
    for (size_t r = 0; r < rows; r += NPD_MOMENTS_AHEAD) {
      T v[NPD_MOMENTS_AHEAD];
#pragma unroll
      for (int u = 0; u < NPD_MOMENTS_AHEAD; u++) v[u] = r + u < rows ? col[(r + u) * cols] : (T)0;
#pragma unroll
      for (int u = 0; u < NPD_MOMENTS_AHEAD; u++) {
        if (r + u >= rows) continue;      /* (nothing is added for a row that is not there: not even +0.0) */
        const double w = (double)v[u];
        if (SQUARES) { const double d = w - mean; const double sq = d * d; acc = acc + sq; }
        else acc = acc + w;
      }
    }
  }
  if (cols == 1) { if (p == 0) partial[0] = acc; return; }
  s[lane] = acc;                           /* (a lane past the last column: the +0.0 the group is padded with) */
  npd_tree_group(s, lane);
  if (lane == 0) partial[blockIdx.x] = s[0];
}

/* one workgroup: the tree's further levels over ws[0 .. g), each level's values written behind the one it read; then the division.
 * SQUARES = false: out[0] = count, out[1] = total / count; true: out[2] = total / divisor, out[3] = its root */
template <bool SQUARES>
__global__ __launch_bounds__(NPD_TREE) void npb_moments_finish_kernel(double *ws, size_t g, double count, double divisor, double *__restrict__ out) {
  __shared__ double s[NPD_TREE];
  const int lane = threadIdx.x;
  const double *in = npd_tree_levels(ws, g, s, lane);
  if (lane == 0) {
    const double total = in[0];
    if (SQUARES) { const double var = total / divisor; out[2] = var; out[3] = sqrt(var); }
    else { out[0] = count; out[1] = total / divisor; }
  }
}

extern "C" size_t npb_moments_workspace(int64_t cols) {
  size_t g = ((size_t)cols + NPD_TREE - 1) / NPD_TREE, total = g;
  while (g > 1) { g = (g + NPD_TREE - 1) / NPD_TREE; total += g; }
  return total;
}

template <typename T> static void npd_moments_launch(const npb_moments_desc_t *M, double *ws, hipStream_t stream) {
  const size_t rows = (size_t)M->rows, cols = (size_t)M->cols, g = (cols + NPD_TREE - 1) / NPD_TREE;
  const double count = (double)(M->rows * M->cols), less = (double)(M->rows * M->cols - M->ddof);
  const dim3 grid((unsigned)g), block(NPD_TREE), one(1);
  const T *x = (const T *)M->src;
  hipLaunchKernelGGL((npb_moments_columns_kernel<T, false>), grid, block, 0, stream, x, rows, cols, (const double *)M->out, ws);
  hipLaunchKernelGGL((npb_moments_finish_kernel<false>), one, block, 0, stream, ws, g, count, count, M->out);
  hipLaunchKernelGGL((npb_moments_columns_kernel<T, true>), grid, block, 0, stream, x, rows, cols, (const double *)M->out, ws);
  hipLaunchKernelGGL((npb_moments_finish_kernel<true>), one, block, 0, stream, ws, g, count, less, M->out);
}
extern "C" void npb_launch_moments(const npb_moments_desc_t *M, double *ws, hipStream_t stream) {
  if (M->type == NPB_ROLLOUT_F64) npd_moments_launch<double>(M, ws, stream);
  else npd_moments_launch<float>(M, ws, stream);
}

/* ---------------------------------------------------------------------------------------------------------------- normaliser */
/* The finish of one fold of the normaliser (include/npb.h, npb_set_normalizer; nuclear_sim_amd/normalizer.py states it): one workgroup.
 * The partials kernel (npd_normalizer.h) has left, per vector v = 3 * stream + {s1, s2, the count as a double: integers, exact in any
 * order}, `groups` values at partial + v * ws_stride.  The tree's further levels run over them here as npb_moments_finish_kernel runs
 * them, but NPD_NORM_ROWS (vector, group) pairs at a time, each a row of LDS, so that a level of all vectors costs the barriers of a few
 * groups and not of 3 S of them; the row stride is npd_normalizer.h's, for its reason.  Then one lane per stream merges -- Chan's merge
 * with the batch taken around the running mean -- writes count, mean, M2 and scale, and ref and scale into the features' table entry of
 * its column, in plain C++: vector stores, which the features kernel's loads of the next launch see.  It lives in this file for its
 * flags: the divisions and the root are IEEE.  groups == 0: no batch (behind npb_set_normalizer and npb_normalizer_set_state): the table
 * follows the state */
#define NPD_NORM_ROWS 16
__global__ __launch_bounds__(NPD_TREE) void npb_normalizer_finish_kernel(npb_normalizer_t Z, int groups) {
  __shared__ double s[NPD_NORM_ROWS * NPD_NORM_STRIDE];
  const int lane = threadIdx.x, S = Z.n_streams;
  size_t at = 0;      /* where the level being read stands in every vector's workspace */
  for (size_t g = (size_t)groups; g > 1;) {
    const size_t per = (g + NPD_TREE - 1) / NPD_TREE, rows = 3 * (size_t)S * per;
    for (size_t r0 = 0; r0 < rows; r0 += NPD_NORM_ROWS) {
      __syncthreads();                     /* (the rows of the pass before have been read) */
#pragma unroll
      for (int j = 0; j < NPD_NORM_ROWS; j++) {
        const size_t r = r0 + j, v = r / per, c = r - v * per, i = c * NPD_TREE + lane;
        s[j * NPD_NORM_STRIDE + lane] = r < rows && i < g ? Z.partial[v * Z.ws_stride + at + i] : 0.0;
      }
      npd_tree_groups<NPD_NORM_ROWS>(s, NPD_NORM_STRIDE, lane);
      if (lane < NPD_NORM_ROWS && r0 + lane < rows) {
        const size_t r = r0 + lane, v = r / per, c = r - v * per;
        Z.partial[v * Z.ws_stride + at + g + c] = s[lane * NPD_NORM_STRIDE];
      }
    }
    __threadfence_block();
    __syncthreads();                       /* the level is written before the next one reads it */
    at += g; g = per;
  }
  if (lane >= S) return;
  const npb_norm_stream_t &D = Z.streams[lane];
  double count = Z.count[lane], mean = Z.mean[lane], M2 = Z.M2[lane];
  const double *mine = Z.partial + 3 * (size_t)lane * Z.ws_stride + at;
  const double cnt = groups > 0 ? mine[2 * Z.ws_stride] : 0.0;
  if (cnt > 0.0) {
    const double shift = count > 0.0 ? mean : D.ref0, s1 = mine[0], s2 = mine[Z.ws_stride];
    const double N = count + cnt;
    const double step = s1 / N;
    mean = shift + step;
    const double sum = M2 + s2, square = s1 * s1, less = square / N;
    M2 = sum - less;
    if (M2 < 0.0) M2 = 0.0;
    count = N;
    Z.count[lane] = count; Z.mean[lane] = mean; Z.M2[lane] = M2;
  }
  double ref = D.ref0, scale = D.scale0;
  if (count > 0.0) {
    const double var = M2 / count, spread = sqrt(var + Z.eps);
    ref = mean; scale = 1.0 / spread;
  }
  Z.scale[lane] = scale;
  if (D.feat_col >= 0) { Z.feat_cols[D.feat_col].ref = ref; Z.feat_cols[D.feat_col].scale = scale; }
}
extern "C" void npb_launch_normalizer_finish(const npb_normalizer_t *Z, int groups, hipStream_t stream) {
  hipLaunchKernelGGL(npb_normalizer_finish_kernel, dim3(1), dim3(NPD_TREE), 0, stream, *Z, groups);
}

/* ---------------------------------------------------------------------------------------------------------------- across shards */
/* One normaliser and one set of moments across W shards (include/npb.h, "ONE NORMALISER AND ONE SET OF ADVANTAGE MOMENTS ACROSS SHARDS";
 * normalizer.shard_delta / combine and rollout.moments_part / moments_combine state them).  They live in this file for its flags: every
 * division and the root are IEEE and no product is fused into a sum.  No atomics, no scratch, plain vector stores.
 * The delta: a lane per stream un-merges the base from the state -- Chan's merge run backwards -- into out [3][S]: count, mean, M2 */
#define NPD_SHARD_LANES 128          /* one workgroup: a lane per stream, NPB_NORM_STREAMS_MAX (65) at most */
__global__ __launch_bounds__(NPD_SHARD_LANES) void npb_normalizer_delta_kernel(const double *__restrict__ count, const double *__restrict__ mean,
                                                                              const double *__restrict__ M2, const double *__restrict__ base, int S,
                                                                              double *__restrict__ out) {
  const int c = threadIdx.x;
  if (c >= S) return;
  const double na = base[c], ma = base[S + c], Ma = base[2 * S + c], N = count[c], m = mean[c], M = M2[c];
  const double nb = N - na;
  double mb = 0.0, Mb = 0.0, n = 0.0;
  if (nb > 0.0) {
    const double ratio = na / nb, drift = m - ma, back = drift * ratio;
    mb = m + back;
    const double d = mb - ma, square = d * d, pairs = na * nb, weight = pairs / N, between = square * weight, within = M - Ma;
    Mb = within - between;
    if (Mb < 0.0) Mb = 0.0;
    n = nb;
  }
  out[c] = n; out[S + c] = mb; out[2 * S + c] = Mb;
}
/* The combine: a lane per stream starts from the base and merges the W deltas [W][3][S] in ascending shard order, a shard with nothing
 * new skipped; the result is the state AND the base.  scale and the features' table follow in npb_normalizer_finish_kernel (groups == 0) */
__global__ __launch_bounds__(NPD_SHARD_LANES) void npb_normalizer_combine_kernel(double *__restrict__ count, double *__restrict__ mean, double *__restrict__ M2,
                                                                                double *__restrict__ base, int S, const double *__restrict__ deltas, int W) {
  const int c = threadIdx.x;
  if (c >= S) return;
  double n = base[c], mu = base[S + c], M = base[2 * S + c];
  for (int w = 0; w < W; w++) {
    const double *D = deltas + (size_t)w * 3 * S;
    const double nb = D[c], mb = D[S + c], Mb = D[2 * S + c];
    if (!(nb > 0.0)) continue;
    const double N = n + nb, d = mb - mu, share = nb / N, step = d * share;
    mu = mu + step;
    const double sum = M + Mb, square = d * d, pairs = n * nb, weight = pairs / N, between = square * weight;
    M = sum + between;
    n = N;
  }
  count[c] = n; mean[c] = mu; M2[c] = M;
  base[c] = n; base[S + c] = mu; base[2 * S + c] = M;
}
extern "C" void npb_launch_normalizer_delta(const npb_normalizer_t *Z, const double *base, double *out, hipStream_t stream) {
  hipLaunchKernelGGL(npb_normalizer_delta_kernel, dim3(1), dim3(NPD_SHARD_LANES), 0, stream, (const double *)Z->count, (const double *)Z->mean,
                     (const double *)Z->M2, base, Z->n_streams, out);
}
extern "C" void npb_launch_normalizer_combine(const npb_normalizer_t *Z, double *base, const double *deltas, int n_shards, hipStream_t stream) {
  hipLaunchKernelGGL(npb_normalizer_combine_kernel, dim3(1), dim3(NPD_SHARD_LANES), 0, stream, Z->count, Z->mean, Z->M2, base, Z->n_streams, deltas,
                     n_shards);
}

/* a shard's part of the moments: one workgroup ends the tree over the partials as npb_moments_finish_kernel does and stores the count and
 * the UNDIVIDED total: part[0] = count, part[1] = total */
__global__ __launch_bounds__(NPD_TREE) void npb_moments_part_finish_kernel(double *ws, size_t g, double count, double *__restrict__ part) {
  __shared__ double s[NPD_TREE];
  const int lane = threadIdx.x;
  const double *in = npd_tree_levels(ws, g, s, lane);
  if (lane == 0) { part[0] = count; part[1] = in[0]; }
}
/* one lane: the W parts [W][2] added in ascending shard order onto 0.0, then the division npb_moments_finish_kernel makes */
__global__ __launch_bounds__(64) void npb_moments_combine_kernel(const double *__restrict__ parts, int W, int squares, double ddof, double *__restrict__ out) {
  if (threadIdx.x != 0) return;
  double C = 0.0, T = 0.0;
  for (int w = 0; w < W; w++) { C = C + parts[2 * w]; T = T + parts[2 * w + 1]; }
  if (squares) { const double less = C - ddof, var = T / less; out[2] = var; out[3] = sqrt(var); }
  else { out[0] = C; out[1] = T / C; }
}
template <typename T> static void npd_moments_part_launch(const npb_moments_desc_t *M, int squares, double *ws, double *part, hipStream_t stream) {
  const size_t rows = (size_t)M->rows, cols = (size_t)M->cols, g = (cols + NPD_TREE - 1) / NPD_TREE;
  const dim3 grid((unsigned)g), block(NPD_TREE), one(1);
  const T *x = (const T *)M->src;
  if (squares) hipLaunchKernelGGL((npb_moments_columns_kernel<T, true>), grid, block, 0, stream, x, rows, cols, (const double *)M->out, ws);
  else hipLaunchKernelGGL((npb_moments_columns_kernel<T, false>), grid, block, 0, stream, x, rows, cols, (const double *)M->out, ws);
  hipLaunchKernelGGL(npb_moments_part_finish_kernel, one, block, 0, stream, ws, g, (double)(M->rows * M->cols), part);
}
extern "C" void npb_launch_moments_part(const npb_moments_desc_t *M, int squares, double *ws, double *part, hipStream_t stream) {
  if (M->type == NPB_ROLLOUT_F64) npd_moments_part_launch<double>(M, squares, ws, part, stream);
  else npd_moments_part_launch<float>(M, squares, ws, part, stream);
}
extern "C" void npb_launch_moments_combine(const double *parts, int n_shards, int squares, int ddof, double *out, hipStream_t stream) {
  hipLaunchKernelGGL(npb_moments_combine_kernel, dim3(1), dim3(64), 0, stream, parts, n_shards, squares, (double)ddof, out);
}

/* ---------------------------------------------------------------------------------------------------------------- permutation */
struct npd_perm_t { uint32_t N, w, mask, key[NPB_MINIBATCH_ROUNDS]; };

__device__ __forceinline__ uint32_t npd_mix(uint32_t h) {      /* murmur3's 32-bit finaliser */
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}
/* entry i < N: the network, again while its result is not below N.  i < N is the caller's: the walk from any other i need not end */
__device__ __forceinline__ uint32_t npd_permute(const npd_perm_t &P, uint32_t i) {
  uint32_t x = i;
  do {
    uint32_t L = x >> P.w, R = x & P.mask;
#pragma unroll
    for (int r = 0; r < NPB_MINIBATCH_ROUNDS; r++) { const uint32_t t = L ^ (npd_mix(R ^ P.key[r]) & P.mask); L = R; R = t; }
    x = (L << P.w) | R;
  } while (x >= P.N);
  return x;
}
static npd_perm_t npd_perm(uint32_t N, const uint32_t *keys) {
  npd_perm_t P;
  uint32_t b = 0;
  while (b < 32 && ((uint64_t)(N - 1) >> b)) b++;      /* bit_length(N - 1) */
  if (b < 2) b = 2;
  P.N = N; P.w = (b + 1) / 2; P.mask = (1u << P.w) - 1u;      /* w <= 16: N - 1 < 2^31 */
  for (int r = 0; r < NPB_MINIBATCH_ROUNDS; r++) P.key[r] = keys[r];
  return P;
}

__global__ __launch_bounds__(256) void npb_permutation_kernel(npd_perm_t P, uint32_t first, uint32_t count, int32_t *__restrict__ out) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= count) return;
  out[j] = (int32_t)npd_permute(P, first + (uint32_t)j);
}
extern "C" void npb_launch_permutation(uint32_t N, const uint32_t *keys, int64_t first, int64_t count, int32_t *out, hipStream_t stream) {
  hipLaunchKernelGGL(npb_permutation_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, npd_perm(N, keys), (uint32_t)first,
                     (uint32_t)count, out);
}

/* ---------------------------------------------------------------------------------------------------------------- minibatch */
/* one gathered tensor: rows of row_bytes, `width` bytes per lane (16, or the element: 8 or 4), 1 << lanes_log2 lanes on a row; dst NULL =
 * not asked for */
struct npd_gather_t { const char *src; char *dst; uint32_t row_bytes; int width, lanes_log2; };
struct npd_minibatch_t {
  npd_perm_t perm;
  uint32_t first, count, n_plants, slots;      /* slots: 1 for transitions, t for whole sequences, every for segments */
  uint32_t every;                              /* 0, or the slots of a segment: an entry is a segment id c * n_plants + p, its source slots c * every .. */
  const void *adv, *ret; void *adv_out, *ret_out; int32_t *index;
  const double *moments; double eps; int f64;
  npd_gather_t g[3];
};

typedef uint32_t npd_b16_t __attribute__((ext_vector_type(4)));      /* 16 and 8 bytes a lane moves at once */
typedef uint32_t npd_b8_t __attribute__((ext_vector_type(2)));
template <typename V>
__device__ __forceinline__ void npd_gather_rows(const npd_gather_t &G, int idx, size_t src_base, size_t dst_base, int rows, int lane) {
  const int L = 1 << G.lanes_log2, per = NPD_WAVE >> G.lanes_log2;      /* lanes on a row, rows in a pass */
  const int sub = lane & (L - 1), mine = lane >> G.lanes_log2;
  const uint32_t pieces = G.row_bytes / (uint32_t)sizeof(V);
  for (int r0 = 0; r0 < rows; r0 += per * NPD_MINIBATCH_AHEAD) {
    const V *from[NPD_MINIBATCH_AHEAD];
    bool live[NPD_MINIBATCH_AHEAD];
#pragma unroll
    for (int u = 0; u < NPD_MINIBATCH_AHEAD; u++) {      /* every lane is here: the lane asked for its index is an active one */
      const int r = r0 + u * per + mine;
      const uint32_t source = (uint32_t)__shfl(idx, r & (NPD_WAVE - 1));
      live[u] = r < rows;
      from[u] = (const V *)(G.src + (src_base + source) * (size_t)G.row_bytes);
    }
    for (uint32_t piece = sub; piece < pieces; piece += L) {      /* (once, unless a row is longer than 64 pieces) */
      V v[NPD_MINIBATCH_AHEAD];
#pragma unroll
      for (int u = 0; u < NPD_MINIBATCH_AHEAD; u++) v[u] = from[u][piece];      /* (a row past the tile's last: some row of the source, not stored) */
#pragma unroll
      for (int u = 0; u < NPD_MINIBATCH_AHEAD; u++)
        if (live[u]) ((V *)(G.dst + (dst_base + (size_t)(r0 + u * per + mine)) * (size_t)G.row_bytes))[piece] = v[u];
    }
  }
}

template <typename T>
__device__ __forceinline__ void npd_minibatch_scalars(const npd_minibatch_t &M, size_t from, size_t to) {
  if (M.adv_out) {
    const T a = ((const T *)M.adv)[from];
    if (M.moments) {
      const double centred = (double)a - M.moments[1];
      const double spread = M.moments[3] + M.eps;
      ((T *)M.adv_out)[to] = (T)(centred / spread);
    } else ((T *)M.adv_out)[to] = a;
  }
  if (M.ret_out) ((T *)M.ret_out)[to] = ((const T *)M.ret)[from];
}

__global__ __launch_bounds__(256) void npb_minibatch_kernel(npd_minibatch_t M) {
  const int lane = threadIdx.x & (NPD_WAVE - 1);
  const size_t waves = (size_t)gridDim.x * (256 / NPD_WAVE);
  const size_t tiles_j = ((size_t)M.count + NPD_MINIBATCH_ROWS - 1) / NPD_MINIBATCH_ROWS, tiles = tiles_j * M.slots;
  for (size_t tile = (size_t)blockIdx.x * (256 / NPD_WAVE) + (threadIdx.x >> 6); tile < tiles; tile += waves) {      /* (uniform in the wave) */
    const size_t slot = tile / tiles_j, j0 = (tile - slot * tiles_j) * NPD_MINIBATCH_ROWS, j = j0 + lane;
    const size_t left = (size_t)M.count - j0;
    const int rows = left < NPD_MINIBATCH_ROWS ? (int)left : NPD_MINIBATCH_ROWS;
    const size_t src_base = slot * M.n_plants, dst_base = slot * M.count + j0;
    int idx = 0;
    if (lane < rows) {
      idx = (int)npd_permute(M.perm, M.first + (uint32_t)j);
      if (slot == 0) M.index[j] = idx;
      if (M.every) {      /* a segment id: from here on the source cell of the segment's slot 0, (c * every) * n_plants + p */
        const uint32_t c = (uint32_t)idx / M.n_plants;
        idx = (int)(c * M.every * M.n_plants + ((uint32_t)idx - c * M.n_plants));
      }
      if (M.f64) npd_minibatch_scalars<double>(M, src_base + (size_t)idx, dst_base + lane);
      else npd_minibatch_scalars<float>(M, src_base + (size_t)idx, dst_base + lane);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const npd_gather_t &G = M.g[k];
      if (!G.dst) continue;
      if (G.width == 16) npd_gather_rows<npd_b16_t>(G, idx, src_base, dst_base, rows, lane);
      else if (G.width == 8) npd_gather_rows<npd_b8_t>(G, idx, src_base, dst_base, rows, lane);
      else npd_gather_rows<uint32_t>(G, idx, src_base, dst_base, rows, lane);
    }
  }
}

/* 16 bytes per lane where every row is a whole number of them and both tensors are 16-byte aligned, else one element; L lanes on a row:
 * the smallest power of two with L * width >= the row, at most 64 */
static npd_gather_t npd_gather(const void *src, void *dst, size_t row_bytes, int element) {
  npd_gather_t G;
  G.src = (const char *)src; G.dst = src && row_bytes ? (char *)dst : nullptr; G.row_bytes = (uint32_t)row_bytes;
  G.width = row_bytes % 16 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0 ? 16 : element;
  G.lanes_log2 = 0;
  while (G.lanes_log2 < 6 && ((size_t)G.width << G.lanes_log2) < row_bytes) G.lanes_log2++;
  return G;
}
extern "C" void npb_launch_minibatch(const npb_minibatch_src_t *S, const npb_minibatch_desc_t *D, int every, hipStream_t stream) {
  const bool plant = D->unit == NPB_MINIBATCH_PLANT, segment = D->unit == NPB_MINIBATCH_SEGMENT;
  npd_minibatch_t M;
  M.perm = npd_perm(plant ? (uint32_t)S->n_plants : (uint32_t)((int64_t)(segment ? S->t / every : S->t) * S->n_plants), D->keys);
  M.first = (uint32_t)D->first; M.count = (uint32_t)D->count; M.n_plants = (uint32_t)S->n_plants; M.slots = plant ? (uint32_t)S->t : (segment ? (uint32_t)every : 1u);
  M.every = segment ? (uint32_t)every : 0u;
  M.adv = D->adv; M.ret = D->ret; M.adv_out = D->adv_out; M.ret_out = D->ret_out; M.index = D->index;
  M.moments = D->moments; M.eps = D->eps; M.f64 = D->type == NPB_ROLLOUT_F64;
  M.g[0] = npd_gather(S->obs, D->obs, (size_t)S->cells * S->obs_bytes, S->obs_bytes);
  M.g[1] = npd_gather(S->act, D->act, (size_t)S->n_axes * S->act_bytes, S->act_bytes);
  M.g[2] = npd_gather(S->extra, D->extra, (size_t)S->n_extras * sizeof(float), (int)sizeof(float));
  const size_t tiles = (((size_t)M.count + NPD_MINIBATCH_ROWS - 1) / NPD_MINIBATCH_ROWS) * M.slots, want = (tiles + 3) / 4;
  const size_t most = D->max_blocks > 0 ? (size_t)D->max_blocks : (size_t)NPD_MINIBATCH_BLOCKS;
  hipLaunchKernelGGL(npb_minibatch_kernel, dim3((unsigned)(want < most ? want : most)), dim3(256), 0, stream, M);
}
