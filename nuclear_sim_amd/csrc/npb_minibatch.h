/* npb_minibatch.h -- host-callable launchers of the pinned moments, the keyed permutation and the minibatch gather (npb_minibatch.hip;
 * internal to libnpb.so; include/npb.h states what they compute). */
#ifndef NPB_MINIBATCH_H
#define NPB_MINIBATCH_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/npb.h"
/* THE pinned tree (include/npb.h, npb_rollout_moments; rollout._tree), stated once for the moments (npb_minibatch.hip) and the normaliser
 * (npd_normalizer.h, npb_minibatch.hip): groups of NPD_TREE values, in each the upper half added onto the lower for half = 128 .. 1 */
#define NPD_TREE 256                 /* the tree's fan-in: one workgroup */
/* the LDS row stride, in doubles, of kernels that run npd_tree_groups over several rows (npd_normalizer.h says why it is odd) */
#define NPD_NORM_STRIDE (NPD_TREE + 1)
#ifdef __HIPCC__
/* one group of the tree: s[0 .. 256) -> s[0]; every lane of the workgroup calls it */
__device__ __forceinline__ void npd_tree_group(double *s, int lane) {
#pragma unroll
  for (int half = NPD_TREE / 2; half >= 1; half >>= 1) {
    __syncthreads();
    if (lane < half) s[lane] = s[lane] + s[lane + half];
  }
  __syncthreads();
}
/* the same group of VECTORS vectors at once, vector v at s + v * stride: the 256 lanes share out the VECTORS * half additions of a level
 * (a level reads [half, 2 half) and writes [0, half) of every vector: no lane reads what another writes before the next barrier), so a
 * pass over all vectors costs the eight barriers of one */
template <int VECTORS> __device__ __forceinline__ void npd_tree_groups(double *s, int stride, int lane) {
#pragma unroll
  for (int log2half = 7; log2half >= 0; log2half--) {
    const int half = 1 << log2half;
    __syncthreads();
    for (int i = lane; i < VECTORS * half; i += NPD_TREE) {
      double *v = s + (i >> log2half) * stride + (i & (half - 1));
      v[0] = v[0] + v[half];
    }
  }
  __syncthreads();
}
/* one workgroup: the tree's further levels over ws[0 .. g), g >= 1, each level's values written behind the one it read; returns where
 * the one value left stands.  s: NPD_TREE doubles of LDS */
__device__ __forceinline__ const double *npd_tree_levels(double *ws, size_t g, double *s, int lane) {
  double *in = ws;
  while (g > 1) {
    double *next = in + g;
    const size_t groups = (g + NPD_TREE - 1) / NPD_TREE;
    for (size_t c = 0; c < groups; c++) {
      const size_t i = c * NPD_TREE + lane;
      __syncthreads();                     /* (s[0] of the group before has been read) */
      s[lane] = i < g ? in[i] : 0.0;
      npd_tree_group(s, lane);
      if (lane == 0) next[c] = s[0];
    }
    __threadfence_block();
    __syncthreads();                       /* the level is written before the next one reads it */
    in = next; g = groups;
  }
  return in;
}
#endif
#ifdef __cplusplus
extern "C" {
#endif
/* the handle's workspace for the moments' partials: `cap` doubles at ws (its one allocation; NULL = none yet) */
typedef struct { double *ws; size_t cap; } npb_moments_ws_t;
/* doubles the partials of a tensor of `cols` columns take: every level of the tree, one behind the other */
size_t npb_moments_workspace(int64_t cols);
/* the four launches; ws holds at least npb_moments_workspace(M->cols) doubles */
void npb_launch_moments(const npb_moments_desc_t *M, double *ws, hipStream_t stream);
/* the moments across shards: a shard's part (one columns pass, squares != 0: around M->out[1]; part [2] = count, the undivided total;
 * M->out is not written), and the combine of n_shards parts [n_shards][2] into out[0], out[1] (squares == 0) or out[2], out[3] */
void npb_launch_moments_part(const npb_moments_desc_t *M, int squares, double *ws, double *part, hipStream_t stream);
void npb_launch_moments_combine(const double *parts, int n_shards, int squares, int ddof, double *out, hipStream_t stream);
void npb_launch_permutation(uint32_t N, const uint32_t *keys, int64_t first, int64_t count, int32_t *out, hipStream_t stream);
/* what the gather reads of the handle's rollout: its buffers, the slots recorded, the shapes and element sizes they were bound with */
typedef struct {
  const void *obs, *act, *extra;
  int t, n_plants, cells, n_axes, n_extras, obs_bytes, act_bytes;
} npb_minibatch_src_t;
/* every: the slots of a segment with D->unit == NPB_MINIBATCH_SEGMENT (S->t a multiple of it), else not read */
void npb_launch_minibatch(const npb_minibatch_src_t *S, const npb_minibatch_desc_t *D, int every, hipStream_t stream);
#ifdef __cplusplus
}
#endif
#endif
