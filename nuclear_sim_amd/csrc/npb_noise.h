/* npb_noise.h -- host-callable launchers of the heat-source noise generator (npb_noise.hip; internal to libnpb.so).
 * One MT19937 stream per plant, numpy's legacy RandomState: key [624][pitch] uint32 (word i of every plant contiguous),
 * pos / has_gauss int32 [pitch], gauss double [pitch]. */
#ifndef NPB_NOISE_H
#define NPB_NOISE_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define NPB_MT_N 624
typedef struct {
  uint32_t *key;       /* [NPB_MT_N][pitch] */
  int32_t *pos;        /* [pitch] */
  int32_t *has_gauss;  /* [pitch] */
  double *gauss;       /* [pitch] */
  size_t pitch;
} npb_noise_t;
/* bytes of one allocation holding the four arrays for `pitch` plants, and the arrays carved out of it */
size_t npb_noise_bytes(size_t pitch);
npb_noise_t npb_noise_layout(void *base, size_t pitch);
/* init_genrand: plant p's seed is read from (uint32_t *)g.pos [p] (the caller puts it there), then pos = 624, no cached gauss */
void npb_launch_noise_seed(npb_noise_t g, int n_plants, hipStream_t stream);
/* the next k standard_normal() draws of every plant into out[t * n_plants + p] */
void npb_launch_noise_fill(npb_noise_t g, int n_plants, int k, double *out, hipStream_t stream);
#ifdef __cplusplus
}
#endif
#endif
