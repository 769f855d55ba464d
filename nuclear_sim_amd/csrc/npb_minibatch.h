/* npb_minibatch.h -- host-callable launchers of the pinned moments, the keyed permutation and the minibatch gather (npb_minibatch.hip;
 * internal to libnpb.so; include/npb.h states what they compute). */
#ifndef NPB_MINIBATCH_H
#define NPB_MINIBATCH_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/npb.h"
#ifdef __cplusplus
extern "C" {
#endif
/* the handle's workspace for the moments' partials: `cap` doubles at ws (its one allocation; NULL = none yet) */
typedef struct { double *ws; size_t cap; } npb_moments_ws_t;
/* doubles the partials of a tensor of `cols` columns take: every level of the tree, one behind the other */
size_t npb_moments_workspace(int64_t cols);
/* the four launches; ws holds at least npb_moments_workspace(M->cols) doubles */
void npb_launch_moments(const npb_moments_desc_t *M, double *ws, hipStream_t stream);
void npb_launch_permutation(uint32_t N, const uint32_t *keys, int64_t first, int64_t count, int32_t *out, hipStream_t stream);
/* what the gather reads of the handle's rollout: its buffers, the slots recorded, the shapes and element sizes they were bound with */
typedef struct {
  const void *obs, *act, *extra;
  int t, n_plants, cells, n_axes, n_extras, obs_bytes, act_bytes;
} npb_minibatch_src_t;
void npb_launch_minibatch(const npb_minibatch_src_t *S, const npb_minibatch_desc_t *D, hipStream_t stream);
#ifdef __cplusplus
}
#endif
#endif
