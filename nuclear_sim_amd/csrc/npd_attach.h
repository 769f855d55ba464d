/* npd_attach.h -- the few definitions that the arena-reading half of a per-step attachment (npb_attachments.hip, once per storage
 * type) and the half that never sees an arena element (npb_storage_free.hip, compiled once) both need: neither unit includes the
 * other's headers for them. */
#ifndef NPD_ATTACH_H
#define NPD_ATTACH_H
#include "npb_kernels.h"

/* the column statistics (npd_column_stats.h): the grid of the fold and of the clear, and the empty values of a cell */
#define NPD_COLSTAT_BLOCK 256
#define NPD_COLSTAT_POS_INF __longlong_as_double(0x7ff0000000000000ll)
#define NPD_COLSTAT_NEG_INF __longlong_as_double((long long)0xfff0000000000000ull)
#define NPD_COLSTAT_NAN __longlong_as_double(0x7ff8000000000000ll)

/* W elements of a features tensor as one access: the features' walk (npd_features.h) and the rollout's copy of a stack (npd_rollout.h) */
template <typename OUT, int W> struct alignas(sizeof(OUT) * W) npd_features_vec { OUT x[W]; };

/* the normaliser (npd_normalizer.h): the discounted return of plant p behind this step's reward r -- the statement's carry, ret * gamma
 * rounded before the sum.  The partials kernel carries it; frozen, the reward kernel does */
__device__ __forceinline__ double npd_normalizer_return(const npb_normalizer_t &Z, size_t p, const int32_t *__restrict__ index, double r) {
  const int32_t seen = Z.seen[p];
  const bool carry = Z.primed[p] && (index ? index[p] : seen) == seen && !Z.ended[p];
  const double kept = Z.ret[p] * Z.gamma;
  return (carry ? kept : 0.0) + r;
}
#endif
