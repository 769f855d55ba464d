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
/* the two builds of the forward kernels and of the gradient kernel: the small one where the features stack, every hidden layer and a
 * core's width fit these; else the large one, NPB_FEATURES_CELLS_MAX and NPB_POLICY_WIDTH_MAX */
#define NPD_POLICY_SMALL_CELLS 64
#define NPD_POLICY_SMALL_WIDTH 64
static inline bool npd_policy_small(const npb_policy_t *P, int core_width /* 0: none */) {
  return P->cells <= NPD_POLICY_SMALL_CELLS && P->width_max <= NPD_POLICY_SMALL_WIDTH && core_width <= NPD_POLICY_SMALL_WIDTH;
}
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
void npb_policy_layout_at(const npb_policy_desc_t *D, int cells, int in0, int n_axes, uint32_t at, uint32_t wp, npb_policy_t *P);
void npb_launch_policy(const npb_policy_t *P, const npd_policy_run_t *R, hipStream_t stream);
/* the z of draw t ([n][A] double) and, where words != NULL, the Philox words behind it ([n][(A + 1) / 2][4] uint32) */
void npb_launch_policy_noise(const npb_policy_t *P, uint64_t t, int n_plants, double *z, uint32_t *words, hipStream_t stream);
/* ---- the recurrent core (npb_set_policy_core; npb_policy_core.hip; nuclear_sim_amd/recurrent.py states it): a GRU cell of width H in front of
 * both nets.  gate[0 .. 2]: the row blocks r, z, n of W_ih with their slices of b_ih (in = K * C, out = H); gate[3 .. 5]: those of W_hh and b_hh
 * (in = H) -- six layers of npd_policy_layer, at the front of theta and of the kernel's copy.  hidden, first, final: the caller's tensors;
 * primed, seen: the handle's bookkeeping, [n] each (base primed; NULL = no core) */
typedef struct {
  int H, gates, final_rows;
  npd_policy_layer_t gate[6];
  uint32_t theta_count, padded_count;      /* the core's own floats of theta and of the kernel's copy */
  float *hidden, *first, *final;
  int32_t *primed, *seen;
} npd_policy_core_t;
/* one launch of the recurrent kernel beside its npd_policy_run_t: h [rows][H] read; h_out: where h' goes (NULL: nowhere); first_out: where the
 * h read goes, the restart rule applied (NULL: nowhere); primed, seen, index: the restart rule's words (primed NULL: no rule, h as it is; index
 * NULL: nothing carried, a plant's index is the one seen); remember: prime the plants and remember their index; start_out: a second copy of
 * what first_out receives, the row of the stored segment states that this step begins (NULL: none; npb_policy_core_segments) */
typedef struct {
  const float *h; float *h_out, *first_out;
  int32_t *primed, *seen; const int32_t *index; int remember;
  float *start_out;
} npd_policy_core_run_t;
void npb_policy_core_layout(int H, int gates, int cells, npd_policy_core_t *C);
void npb_launch_policy_repack(const npb_policy_t *P, const npd_policy_core_t *C /* NULL: no core */, hipStream_t stream);      /* (npb_policy.hip: every layer, one launch) */
void npb_launch_policy_core(const npb_policy_t *P, const npd_policy_core_t *C, const npd_policy_run_t *R, const npd_policy_core_run_t *G, hipStream_t stream);
/* behind the rollout's post kernel: hidden[p] into final[final_row[p]] for every plant that took a row of final_obs in this slot */
void npb_launch_policy_core_final(const npd_policy_core_t *C, const int32_t *final_row, int n_plants, hipStream_t stream);
#ifdef __cplusplus
}
#endif
#ifdef __HIPCC__
/* ---- what the step's launches (npb_policy.hip, npb_policy_core.hip) and the gradient kernel (npb_ppo.hip) share: the tile's geometry, its
 * rows into LDS and one layer of a net */
#define NPD_POLICY_TILE 32
#define NPD_POLICY_GROUPS 8
#define NPD_POLICY_LANES (NPD_POLICY_TILE * NPD_POLICY_GROUPS)
#define NPD_POLICY_WAVES 4
#define NPD_POLICY_AHEAD 8        /* matrix-core calls whose operands are in flight together */
#define NPD_POLICY_STRIDE (NPD_POLICY_TILE + 1)      /* the LDS row stride of every [k][plant] buffer (the header says why it is odd) */
/* the live rows of the tile at `base`, 1 .. 32: the last tile may be ragged.  None of the three tile pieces holds a barrier: the callers
 * place theirs */
__device__ __forceinline__ int npd_policy_in_tile(size_t rows, size_t base) { return rows - base < (size_t)NPD_POLICY_TILE ? (int)(rows - base) : NPD_POLICY_TILE; }
/* +0.0 into rows k_from .. k_to - 1 of a [k][plant] buffer, all 32 plants, 256 lanes: a k extension, or the gradient kernel's whole xs */
__device__ __forceinline__ void npd_policy_tile_zero(float *buf, int k_from, int k_to, int tid) {
  for (int i = tid; i < (k_to - k_from) * NPD_POLICY_TILE; i += NPD_POLICY_LANES)
    buf[(k_from + i / NPD_POLICY_TILE) * NPD_POLICY_STRIDE + (i & (NPD_POLICY_TILE - 1))] = 0.0f;
}
/* the tile's in_tile rows of K elements, ONE contiguous run: consecutive lanes on consecutive elements, narrowed to float and transposed
 * into xs[k][row]; a cell that is not finite marks its row in bad (set, never cleared: every writer writes the same 1) */
template <typename IN>
__device__ __forceinline__ void npd_policy_tile_load(const IN *run, int in_tile, int K, float *xs, int *bad, int tid) {
  const int total = in_tile * K;
  for (int e = tid; e < total; e += NPD_POLICY_LANES) {
    const int row = e / K, k = e - row * K;
    const float v = (float)run[e];
    xs[k * NPD_POLICY_STRIDE + row] = v;
    if (!(v - v == 0.0f)) bad[row] = 1;
  }
}
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
/* a whole net: xs -> the head's outputs in head[j][r]; a, b: the two hidden buffers */
__device__ __forceinline__ void npd_policy_net(const npd_policy_net_t &N, const float *theta, const float *padded, const float *xs, float *a, float *b,
                                               float *head, int activation, int wave, int lane) {
  const float *in = xs;
  for (int l = 0; l < N.n_layers; l++) {
    const bool last = l == N.n_layers - 1;
    float *out = last ? head : (l & 1) ? b : a;
    npd_policy_layer(N.layer[l], theta, padded, in, out, last ? -1 : activation, wave, lane);
    __syncthreads();
    in = out;
  }
}
/* ---- THE CELL, stated once under the statement's names (recurrent.py: sigma, tau, cell, sigma_slope, tau_slope): what the recurrent step
 * (npb_policy_core.hip) and the sequence kernels (npb_ppo_seq.hip: the forward sweep, the backward sweep's recompute, the refresh) share.
 * Every float operation below is rounded on its own, in the statement's order */
#define NPD_CORE_SOFT 0
#define NPD_CORE_HARD 1

/* the hard S in front of its clamp; the clamp and "does it clamp at a" are the two bodies below and nowhere else */
__device__ __forceinline__ float npd_core_hard_line(float a) {
  const float q = 0.25f * a;
  return q + 0.5f;
}
__device__ __forceinline__ float npd_core_sigma(float a, int gates) {
  if (gates == NPD_CORE_HARD) {
    const float y = npd_core_hard_line(a);
    return y < 0.0f ? 0.0f : (y > 1.0f ? 1.0f : y);
  }
  const float half = 0.5f * a;
  const float t = tanhf(half);
  const float s = 0.5f * t;
  return s + 0.5f;
}
__device__ __forceinline__ bool npd_core_sigma_clamps(float a, int gates) {
  const float y = npd_core_hard_line(a);
  return gates == NPD_CORE_HARD && (y < 0.0f || y > 1.0f);
}
__device__ __forceinline__ float npd_core_tau(float a, int gates) {
  if (gates == NPD_CORE_HARD) return a < -1.0f ? -1.0f : (a > 1.0f ? 1.0f : a);
  return tanhf(a);
}
/* d * S', given npd_core_sigma_clamps(a) and s = S(a) */
__device__ __forceinline__ float npd_core_sigma_slope(float d, bool clamps, float s, int gates) {
  if (gates == NPD_CORE_HARD) {
    const float q = d * 0.25f;
    return clamps ? 0.0f : q;
  }
  const float oms = 1.0f - s;
  const float slope = s * oms;
  return d * slope;
}
/* d * T', given a and n = T(a) */
__device__ __forceinline__ float npd_core_tau_slope(float d, float a, float n, int gates) {
  if (gates == NPD_CORE_HARD) return a < -1.0f || a > 1.0f ? 0.0f : d;
  const float sq = n * n;
  const float slope = 1.0f - sq;
  return d * slope;
}
/* the forward of the cell over a tile, gate by gate, so that only H-wide buffers live in LDS: gi = W_i* xs and gh = W_h* h (two layers, one
 * barrier: they read xs and h and write apart; gh's chunks of 32 outputs start two waves on, so a cell of up to 64 cells keeps all four waves
 * busy), then 256 lanes over the H x 32 cells: r = S(gi + gh), z likewise, and for the candidate n = T(gi + r * gh), h' = n + z * (h - n) over h
 * in place (a cell is read and written by one lane).  A poisoned plant (bad) and the k extension, H up to the next multiple of 4, get +0.0.
 * Every lane of the workgroup calls it (it holds barriers, the last one behind h'); xs and h stand before the call */
__device__ __forceinline__ void npd_core_cell(const npb_policy_t &P, const npd_policy_core_t &C, const float *xs, float *h, float *gi, float *gh, float *r, float *z,
                                              const int *bad, int tid) {
  const int wave = tid >> 6, lane = tid & 63, H = C.H, H_pad = (H + 3) & ~3;
  for (int gate = 0; gate < 3; gate++) {
    npd_policy_layer(C.gate[gate], P.theta, P.padded, xs, gi, -1, wave, lane);
    npd_policy_layer(C.gate[3 + gate], P.theta, P.padded, h, gh, -1, (wave + 2) & (NPD_POLICY_WAVES - 1), lane);
    __syncthreads();
    for (int i = tid; i < H_pad * NPD_POLICY_TILE; i += NPD_POLICY_LANES) {
      const int j = i / NPD_POLICY_TILE, plant = i & (NPD_POLICY_TILE - 1), o = j * NPD_POLICY_STRIDE + plant;
      if (gate < 2) {
        const float a = gi[o] + gh[o];
        (gate ? z : r)[o] = npd_core_sigma(a, C.gates);
      } else {
        const float gated = r[o] * gh[o];
        const float a = gi[o] + gated;
        const float n = npd_core_tau(a, C.gates);
        const float hv = h[o];
        const float away = hv - n;
        const float kept = z[o] * away;
        const float next = n + kept;
        h[o] = j < H && !bad[plant] ? next : 0.0f;
      }
    }
    __syncthreads();
  }
}
/* a tile's run of H-wide rows and a [k][plant] buffer, the reading and the writing twin.  npd_seq_fill: the buffer filled whole, k up to H_pad:
 * plant `row` reads H contiguous floats at source(row), or +0.0 where it has none (beyond the tile, a plant without a source, a restarted
 * plant).  npd_core_store: the tile's in_tile rows of H floats, ONE contiguous run, out of the buffer transposed (consecutive k are 33 floats
 * apart: no bank conflict).  Consecutive lanes on consecutive elements of the run in both; no barrier in either */
template <class Source>
__device__ __forceinline__ void npd_seq_fill(float *dst, int H, int H_pad, int tid, Source source) {
  for (int e = tid; e < H_pad * NPD_POLICY_TILE; e += NPD_POLICY_LANES) {
    const int row = e / H_pad, k = e - row * H_pad;
    const float *from = source(row);
    dst[k * NPD_POLICY_STRIDE + row] = from && k < H ? from[k] : 0.0f;
  }
}
__device__ __forceinline__ void npd_core_store(float *run, const float *src, int in_tile, int H, int tid) {
  for (int e = tid; e < in_tile * H; e += NPD_POLICY_LANES) {
    const int row = e / H, k = e - row * H;
    run[e] = src[k * NPD_POLICY_STRIDE + row];
  }
}
/* ---- the noise: Philox4x32-10 and the pair of normals of one call (policy.py: philox4x32, noise_from_words) */
__device__ __forceinline__ void npd_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
  for (int round = 0; round < 10; round++) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0, hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
/* call j of plant `id` at draw t: z of axes 2j and 2j + 1 */
__device__ __forceinline__ void npd_policy_pair(uint64_t seed, uint32_t id, uint64_t t, uint32_t j, uint32_t w[4], double *z0, double *z1) {
  npd_philox4x32_10(id, (uint32_t)t, (uint32_t)(t >> 32), j, (uint32_t)seed, (uint32_t)(seed >> 32), w);
  const double u1 = (((double)w[0] * 1048576.0 + (double)(w[1] >> 12)) + 0.5) * 0x1p-52;
  const double u2 = (((double)w[2] * 1048576.0 + (double)(w[3] >> 12)) + 0.5) * 0x1p-52;
  const double r = sqrt(-2.0 * log(u1)), th = 6.283185307179586 * u2;
  *z0 = r * cos(th);
  *z1 = r * sin(th);
}
/* ---- the epilogue of a step's launch, what the MLP kernel (npb_policy.hip) and the recurrent one (npb_policy_core.hip) share: the draw,
 * then every output.  A lane is (group g = 0 .. 7, plant r = 0 .. 31) of the tile at `base`; mean[a][r] and val[r] are the heads' floats in LDS
 * (row stride NPD_POLICY_STRIDE), zs the draw's LDS, bad[r] != 0 a poisoned plant.  Every lane of the workgroup calls it (it holds a barrier). */
__device__ __forceinline__ void npd_policy_epilogue(const npb_policy_t &P, const npd_policy_run_t &R, const float *mean, const float *val, double *zs,
                                                    const int *bad, int g, int r, int in_tile, size_t base) {
  const bool live = r < in_tile;
  const size_t p = base + r;
  const float qnan = __builtin_nanf("");
  if (!R.act) {      /* npb_policy_values */
    if (g == 0 && live) R.value[p] = bad[r] ? qnan : val[r];
    return;
  }
  const int A = P.n_axes;
  if (2 * g < A) {
    double z0 = 0.0, z1 = 0.0;
    if (!R.deterministic && live) {
      uint32_t w[4];
      npd_policy_pair(R.seed, R.first + (uint32_t)p, R.t, (uint32_t)g, w, &z0, &z1);
    }
    zs[(2 * g) * NPD_POLICY_TILE + r] = z0;
    if (2 * g + 1 < NPB_CONTROLS_AXES_MAX) zs[(2 * g + 1) * NPD_POLICY_TILE + r] = z1;
  }
  __syncthreads();
  if (!live) return;
  const bool poisoned = bad[r] != 0;
  if (g < A) {
    const double scaled = (double)P.theta[P.std + g] * zs[g * NPD_POLICY_TILE + r];
    const double a = (double)mean[g * NPD_POLICY_STRIDE + r] + scaled;
    if (R.act_f64) ((double *)R.act)[p * A + g] = poisoned ? (double)qnan : a;
    else ((float *)R.act)[p * A + g] = poisoned ? qnan : (float)a;
  }
  if (g == NPD_POLICY_GROUPS - 1) {
    double lp = -((double)A * 0.9189385332046727);
    for (int a = 0; a < A; a++) {
      const double z = zs[a * NPD_POLICY_TILE + r], sq = z * z, half = 0.5 * sq;
      lp = (lp - half) - (double)P.theta[P.log_std + a];
    }
    const float value = poisoned ? qnan : val[r], logp = poisoned ? qnan : (float)lp;
    R.value[p] = value;
    R.logp[p] = logp;
    if (R.extras && R.value_slot >= 0) R.extras[p * R.n_extras + R.value_slot] = value;
    if (R.extras && R.logp_slot >= 0) R.extras[p * R.n_extras + R.logp_slot] = logp;
  }
}
#endif
#endif
