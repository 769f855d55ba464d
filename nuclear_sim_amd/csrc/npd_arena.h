/* npd_arena.h -- how a kernel outside the step's staging pipeline addresses the arena: the segment rule, the plain global movers of
 * a section and of a single member, the bits of a real as it is stored, and the name rule of a launcher.  For every translation unit
 * that is compiled once per storage type (npb_kernels.hip, npb_attachments.hip; DESIGN.md, "The translation units of libnpb.so"):
 * what follows depends on npd_real_t (npd_stage.h) and is the same text for both builds. */
#ifndef NPD_ARENA_H
#define NPD_ARENA_H
#include "npd_stage.h"

/* ---- segmented arena.  A handle of more than 45 056 plants keeps its arena in SEGMENTS of 16 384 plants: segment s
 * is the whole [column][plant] block of plants s * seg .. (s + 1) * seg - 1, so a launch over one segment sweeps one dense range of
 * memory (two handles of 32 768 plants step 4-6 % faster than one of 65 536 laid out column by column over all plants,
 * profiles/r3_shared_launches.txt; what makes the difference is not the launch per handle but the layout: one launch of the four-wave kernel
 * over a segmented arena is as fast, profiles/r3_segment_size.txt).  Every kernel takes
 * the arena pointer and "N", the column pitch in plants, whose upper 32 bits carry the segment size (0 = one segment); with
 *   address(column, plant p) = arena + s * seg * columns + column * seg + (p - s * seg) = [arena + s * seg * (columns - 1)] + column * seg + p
 * a kernel only has to move its base pointer once, by its plant's segment, and use the segment size as its pitch. */
#ifdef NPB_BUILD_F32
#define NPD_ARENA_COLS NPB_TOTAL_COL32
#else
#define NPD_ARENA_COLS NPB_TOTAL_COL64
#endif
#define NPD_SEGMENT(arena, N, p) do { const size_t seg__ = (size_t)(N) >> 32; (N) = (size_t)(N) & 0xffffffffu; \
    if (seg__) { (arena) += ((size_t)(p) / seg__) * seg__ * (size_t)(NPD_ARENA_COLS - 1); (N) = seg__; } } while (0)
/* launcher side: the pitch and the segment size out of a packed N */
#define NPD_NPAD(npad) ((size_t)(npad) & 0xffffffffu)
#define NPD_SEG_OF(npad) ((size_t)(npad) >> 32)

/* ---- section <-> arena movers outside the step kernel (init, observe, maintenance): plain global accesses.
 * A section struct is NF doubles (the last NO of them outputs) followed by NI int32s (include/npb_fields.h); in the
 * arena the NF - NO carried doubles take one column each and the narrow members share columns (npd_stage.h). */
__device__ __forceinline__ char *npd_gaddr(npd_real_t *arena, size_t N, size_t p, int col) {
  return (char *)(arena + (size_t)col * N + p);
}
template <int NF, int NO, int NI, typename S>
__device__ __forceinline__ void npd_load(S &s, const npd_real_t *__restrict__ arena, size_t N, size_t p, int col0) {
  double *d = reinterpret_cast<double *>(&s);
  constexpr int NC = NF - NO;
  npd_real_t *a = const_cast<npd_real_t *>(arena);
#pragma unroll
  for (int k = 0; k < NC; k++) d[k] = (double)*(const npd_real_t *)npd_gaddr(a, N, p, col0 + k);
#pragma unroll
  for (int j = 0; j < NO; j++) d[NC + j] = (double)*(const float *)(npd_gaddr(a, N, p, col0 + NC + j / NPD_NPC) + (j % NPD_NPC) * 4);
  int32_t *q = reinterpret_cast<int32_t *>(d + NF);
#pragma unroll
  for (int k = 0; k < NI; k++) q[k] = *(const int32_t *)(npd_gaddr(a, N, p, col0 + NC + (NO + k) / NPD_NPC) + ((NO + k) % NPD_NPC) * 4);
}
template <int NF, int NO, int NI, typename S>
__device__ __forceinline__ void npd_store(const S &s, npd_real_t *__restrict__ arena, size_t N, size_t p, int col0) {
  const double *d = reinterpret_cast<const double *>(&s);
  constexpr int NC = NF - NO;
#pragma unroll
  for (int k = 0; k < NC; k++) *(npd_real_t *)npd_gaddr(arena, N, p, col0 + k) = (npd_real_t)d[k];
#pragma unroll
  for (int j = 0; j < NO; j++) *(float *)(npd_gaddr(arena, N, p, col0 + NC + j / NPD_NPC) + (j % NPD_NPC) * 4) = (float)d[NC + j];
  const int32_t *q = reinterpret_cast<const int32_t *>(d + NF);
#pragma unroll
  for (int k = 0; k < NI; k++) *(int32_t *)(npd_gaddr(arena, N, p, col0 + NC + (NO + k) / NPD_NPC) + ((NO + k) % NPD_NPC) * 4) = q[k];
  if ((NO + NI) % NPD_NPC) *(int32_t *)(npd_gaddr(arena, N, p, col0 + NC + (NO + NI) / NPD_NPC) + 4) = 0; /* unused half of the last column */
}
#define NPD_LOAD(T, stype, s, inst) npd_load<NPB_##T##_NF64, NPB_##T##_NOUT, NPB_##T##_NI32, stype>(s, f64, N, p, NPD_SEC_COL(T, inst))
#define NPD_STORE(T, stype, s, inst) npd_store<NPB_##T##_NF64, NPB_##T##_NOUT, NPB_##T##_NI32, stype>(s, f64, N, p, NPD_SEC_COL(T, inst))
/* single member reads: fp64 member (carried or output) / int32 member */
template <int NC> __device__ __forceinline__ double npd_gread_real(const npd_real_t *arena, size_t N, size_t p, int col0, int idx) {
  npd_real_t *a = const_cast<npd_real_t *>(arena);
  if (idx < NC) return (double)*(const npd_real_t *)npd_gaddr(a, N, p, col0 + idx);
  const int j = idx - NC;
  return (double)*(const float *)(npd_gaddr(a, N, p, col0 + NC + j / NPD_NPC) + (j % NPD_NPC) * 4);
}
#define NPD_F64_COL(T, stype, member, inst) npd_gread_real<NPB_##T##_NCARRY>(f64, N, p, NPD_SEC_COL(T, inst), NPB_F64_SLOT(stype, member))
#define NPD_F64_COLK(T, stype, member, inst, k) npd_gread_real<NPB_##T##_NCARRY>(f64, N, p, NPD_SEC_COL(T, inst), NPB_F64_SLOT(stype, member) + (k))
#define NPD_I32_COL(T, stype, member, inst) \
  (*(const int32_t *)(npd_gaddr(const_cast<npd_real_t *>(f64), N, p, NPD_SEC_COL(T, inst) + NPB_##T##_NCARRY + (NPB_##T##_NOUT + NPB_I32_SLOT(stype, T, member)) / NPD_NPC) + \
                      ((NPB_##T##_NOUT + NPB_I32_SLOT(stype, T, member)) % NPD_NPC) * 4))

/* bit pattern of a value as it is stored (fp32 storage: after rounding to fp32) */
__device__ __forceinline__ long long npd_real_bits(double v) {
#ifdef NPB_BUILD_F32
  return (long long)__float_as_int((float)v);
#else
  return __double_as_longlong(v);
#endif
}

#ifdef NPB_BUILD_F32
#define NPB_LAUNCHER(name) npb32_launch_##name
#else
#define NPB_LAUNCHER(name) npb_launch_##name
#endif
#endif
