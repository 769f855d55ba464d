/* npb_policy.h -- host-callable launchers of the policy (npb_policy.hip; internal to libnpb.so; include/npb.h and
 * nuclear_sim_amd/policy.py state what they compute). */
#ifndef NPB_POLICY_H
#define NPB_POLICY_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/npb.h"
#ifdef __cplusplus
extern "C" {
#endif
#define NPD_POLICY_LAYERS_MAX (NPB_POLICY_HIDDEN_MAX + 1)      /* the hidden layers and the head */
/* one layer: `in` inputs (in_pad: the next multiple of 4), `out` outputs (out_pad: the next multiple of 32); its bias at theta + b, its
 * weights as the caller packed them at theta + w, and as the kernel reads them at padded + wp: Wt[in_pad][out_pad], the cells beyond `in`
 * and beyond `out` +0.0 */
typedef struct { int in, in_pad, out, out_pad; uint32_t w, b, wp; } npd_policy_layer_t;
typedef struct { int n_layers; npd_policy_layer_t layer[NPD_POLICY_LAYERS_MAX]; } npd_policy_net_t;
/* what the handle keeps of a set policy: the shapes, the caller's descriptor, and ONE device allocation (base theta): theta
 * [theta_count] | padded [padded_count] */
typedef struct {
  float *theta; float *padded;
  uint32_t theta_count, padded_count, log_std, std;      /* (log_std, std: offsets into theta) */
  npd_policy_net_t actor, critic;
  int cells, n_axes, width_max;      /* K * C; A; the widest hidden layer of either net */
  npb_policy_desc_t D;
} npb_policy_t;
/* one launch of the nets over `rows` rows of x ([rows][cells], float or double).  act != NULL: the step's launch -- actor, noise, critic,
 * every output; act == NULL: the critic alone into value (npb_policy_values) */
typedef struct {
  const void *x; int x_f64, rows;
  void *act; int act_f64;
  float *value, *logp, *extras; int n_extras, value_slot, logp_slot;
  uint64_t seed, t; uint32_t first; int deterministic;
} npd_policy_run_t;
/* the shapes of a descriptor laid out: every offset and count of *P but its pointers */
void npb_policy_layout(const npb_policy_desc_t *D, int cells, int n_axes, npb_policy_t *P);
void npb_launch_policy_repack(const npb_policy_t *P, hipStream_t stream);
void npb_launch_policy(const npb_policy_t *P, const npd_policy_run_t *R, hipStream_t stream);
/* the z of draw t ([n][A] double) and, where words != NULL, the Philox words behind it ([n][(A + 1) / 2][4] uint32) */
void npb_launch_policy_noise(const npb_policy_t *P, uint64_t t, int n_plants, double *z, uint32_t *words, hipStream_t stream);
#ifdef __cplusplus
}
#endif
#ifdef __HIPCC__
/* ---- what the step's launch (npb_policy.hip) and the gradient kernel (npb_ppo.hip) share: the tile's geometry and one layer of a net */
#define NPD_POLICY_TILE 32
#define NPD_POLICY_GROUPS 8
#define NPD_POLICY_LANES (NPD_POLICY_TILE * NPD_POLICY_GROUPS)
#define NPD_POLICY_WAVES 4
#define NPD_POLICY_AHEAD 8        /* matrix-core calls whose operands are in flight together */
#define NPD_POLICY_STRIDE (NPD_POLICY_TILE + 1)      /* the LDS row stride of every [k][plant] buffer (the header says why it is odd) */
/* one layer over the tile on the matrix cores: in[k][r] -> out[j][r] (row stride NPD_POLICY_STRIDE both), j up to the next multiple of 4
 * of the width; activation: NPB_POLICY_RELU, NPB_POLICY_TANH, or -1 for a head.  Wave `wave` takes the chunks wave, wave + 4, .. of 32
 * outputs.  v_mfma_f32_32x32x2_f32: D[i][j] = fma(A[i][k0 + 1], B[k0 + 1][j], fma(A[i][k0], B[k0][j], C[i][j])), one rounding per product:
 * the statement's chain, two k a call.  i is the plant, j the output.  Lane l gives A[i = l & 31][k = l >> 5] = in[k0 + (l >> 5)][l & 31]
 * and B[k = l >> 5][j = l & 31] = Wt[k0 + (l >> 5)][j0 + (l & 31)], and holds D[i = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)][j = l & 31] in
 * register reg of 16: its column's bias is the initial accumulator of all 16 */
typedef float npd_f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ void npd_policy_layer(const npd_policy_layer_t &L, const float *__restrict__ theta, const float *__restrict__ padded,
                                                 const float *in, float *out, int activation, int wave, int lane) {
  const int col = lane & 31, half = lane >> 5, out_pad4 = (L.out + 3) & ~3, pairs = L.in_pad >> 1;
  for (int j0 = 32 * wave; j0 < L.out_pad; j0 += 32 * NPD_POLICY_WAVES) {
    const int j = j0 + col;
    const float bias = j < L.out ? theta[L.b + j] : 0.0f;
    npd_f32x16 acc;
#pragma unroll
    for (int reg = 0; reg < 16; reg++) acc[reg] = bias;
    const float *a = in + half * NPD_POLICY_STRIDE + col;
    const float *b = padded + L.wp + (size_t)half * L.out_pad + j;
    /* the operands of NPD_POLICY_AHEAD calls are asked for before the first of them runs: a call waits for its own two loads only, and
     * the chain of dependent calls is the same chain (no call is added for padding: fma(+0, +0, acc) would turn an accumulator of -0.0) */
    int s = 0;
    for (; s + NPD_POLICY_AHEAD <= pairs; s += NPD_POLICY_AHEAD) {
      float av[NPD_POLICY_AHEAD], bv[NPD_POLICY_AHEAD];
#pragma unroll
      for (int u = 0; u < NPD_POLICY_AHEAD; u++) {
        av[u] = a[2 * (s + u) * NPD_POLICY_STRIDE];
        bv[u] = b[(size_t)(2 * (s + u)) * L.out_pad];
      }
#pragma unroll
      for (int u = 0; u < NPD_POLICY_AHEAD; u++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
    }
    for (; s < pairs; s++)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * s * NPD_POLICY_STRIDE], b[(size_t)(2 * s) * L.out_pad], acc, 0, 0, 0);
    if (j < out_pad4) {
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int plant = (reg & 3) + 8 * (reg >> 2) + 4 * half;
        float y = acc[reg];
        if (activation == NPB_POLICY_RELU) y = y > 0.0f ? y : 0.0f;
        else if (activation == NPB_POLICY_TANH) y = tanhf(y);
        out[j * NPD_POLICY_STRIDE + plant] = j < L.out ? y : 0.0f;
      }
    }
  }
}
#endif
#endif
