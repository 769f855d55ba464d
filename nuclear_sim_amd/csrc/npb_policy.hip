/* npb_policy.hip -- the policy on the device (npb_set_policy, include/npb.h): a diagonal-Gaussian actor and a critic, two MLPs over every
 * plant's features stack, the Gaussian draw, the log-probability and the value, in ONE launch in front of every step.
 * nuclear_sim_amd/policy.py states it in numpy; this file produces its bits (its float tanh apart, which the statement licenses): a layer
 * is bias, then fmaf(x[k], W[j][k], acc) for k ascending in float32, k extended with +0.0 cells and +0.0 weights to a multiple of 4; the
 * epilogue runs in double with every operation rounded on its own.  Built with the noise generator's flags (Makefile): no contraction, IEEE
 * division and square root, no -freciprocal-math / -fapprox-func.
 *
 * THE KERNEL THAT SHIPS RUNS ON THE MATRIX CORES: v_mfma_f32_32x32x2_f32 is exact f32, one rounding per product in k order, and the
 * relu tests hold it to the statement's bits (DESIGN.md has the v_fma_f32 chain it replaced and both times).
 * One workgroup of 256 lanes (four waves) per tile of 32 plants.
 *   1. the tile's 32 rows of x are ONE contiguous run of 32 x K*C elements: loaded with consecutive lanes on consecutive elements,
 *      narrowed to float and transposed into LDS, xs[k][r] with a row stride of 33 (consecutive lanes write consecutive k: 33 spreads them
 *      over the banks; a layer reads xs[k][r] with consecutive lanes on consecutive r).  A row beyond `rows` is neither loaded nor stored.
 *      A cell that is not finite marks its plant (a plain LDS store of 1: every writer writes the same).  The pieces are npb_policy.h's,
 *      which the recurrent kernel and the gradient kernel call too: npd_policy_in_tile, npd_policy_tile_zero, npd_policy_tile_load.
 *   2. a layer: a wave takes 32 outputs at a time (npd_policy_layer says how the operands lie): per call one LDS read of the A operand
 *      straight from xs / h, and one coalesced load of the B operand from the copy npb_policy_load made, Wt[k][j] with k and j padded
 *      with +0.0 (rows of 128 bytes a half-wave).  The bias is the initial accumulator.  The activation, then h[j][r] into LDS, the
 *      same layout and stride (a lane holds 16 plants of ONE output: its stores go 33 floats apart from its neighbour's: no conflict);
 *      outputs beyond the width, up to the next multiple of 4, are written +0.0: they are the next layer's k extension.  A barrier
 *      between layers; two hidden buffers, ping-pong; the actor first, then the critic, xs kept.  A layer narrower than 128 leaves
 *      waves without a chunk: they wait at the barrier.
 *   3. the epilogue (npd_policy_epilogue, npb_policy.h: the recurrent kernel of npb_policy_core.hip ends in the same one), a lane being
 *      (group g = 0 .. 7, plant r = 0 .. 31): group j < ceil(A / 2) draws pair j of its plant (Philox4x32-10,
 *      Box-Muller in double; npd_policy_pair, the function npb_policy_noise runs) into LDS; then group a < A forms and stores action a,
 *      and group 7 the log-probability (ascending over the axes), value and logp, and the two extras slots.  A marked plant stores THE
 *      quiet NaN everywhere.
 * LDS: the small build (npd_policy_small, npb_policy.h: K*C <= NPD_POLICY_SMALL_CELLS, widths <= NPD_POLICY_SMALL_WIDTH) 3 x 8.25 KiB and
 * the epilogue's 4.7 KiB; the large one (NPB_FEATURES_CELLS_MAX, NPB_POLICY_WIDTH_MAX) 33 + 2 x 16.5 KiB and the same -- static, beyond
 * 64 KiB, which gfx950's 160 KiB per CU allows.  No scratch, no atomics, plain vector stores.
 * npb_launch_policy_repack, the one repack there is, lays out every layer in one launch: a core's gates, the actor, the critic. */
#include <hip/hip_runtime.h>
#include <math.h>
#include "npb_policy.h"

/* ---- the noise: Philox4x32-10 and the pair of normals of one call are npb_policy.h's (npd_policy_pair): the recurrent kernel draws with them too */
__global__ __launch_bounds__(256) void npb_policy_noise_kernel(uint64_t seed, uint32_t first, uint64_t t, int n_plants, int n_axes, double *z, uint32_t *words) {
  const int J = (n_axes + 1) / 2;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n_plants * J) return;
  const size_t p = i / J;
  const int j = (int)(i - p * J);
  uint32_t w[4];
  double z0, z1;
  npd_policy_pair(seed, first + (uint32_t)p, t, (uint32_t)j, w, &z0, &z1);
  if (z) {
    z[p * n_axes + 2 * j] = z0;
    if (2 * j + 1 < n_axes) z[p * n_axes + 2 * j + 1] = z1;
  }
  if (words) {
#pragma unroll
    for (int q = 0; q < 4; q++) words[i * 4 + q] = w[q];
  }
}

/* ---- the kernel's copy of the weights, in the order the matrix cores' B operand is read: Wt[k][j], in_pad rows of out_pad floats (out_pad:
 * the width up to a multiple of 32), the cells beyond `in` and beyond `out` +0.0.  ONE launch over every layer there is: a core's six gate
 * layers, the actor's, the critic's */
typedef struct { const float *theta; float *padded; int n_layers; npd_policy_layer_t layer[6 + 2 * NPD_POLICY_LAYERS_MAX]; } npd_policy_repack_t;
__global__ __launch_bounds__(256) void npb_policy_repack_kernel(npd_policy_repack_t K) {
  const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  for (int l = 0; l < K.n_layers; l++) {
    const npd_policy_layer_t L = K.layer[l];
    const size_t total = (size_t)L.in_pad * L.out_pad;
    for (size_t i = first; i < total; i += stride) {
      const size_t k = i / L.out_pad, j = i - k * L.out_pad;
      K.padded[L.wp + i] = k < (size_t)L.in && j < (size_t)L.out ? K.theta[L.w + j * L.in + k] : 0.0f;
    }
  }
}

/* ---- the nets */
/* (one layer on the matrix cores: npd_policy_layer, npb_policy.h -- the gradient kernel, npb_ppo.hip, runs the same routine) */
/* (a whole net, layer after layer: npd_policy_net, npb_policy.h) */
template <typename IN, int KC_MAX, int H_MAX>
__global__ __launch_bounds__(NPD_POLICY_LANES) void npb_policy_kernel(npb_policy_t P, npd_policy_run_t R) {
  __shared__ float xs[KC_MAX * NPD_POLICY_STRIDE];
  __shared__ float ha[H_MAX * NPD_POLICY_STRIDE], hb[H_MAX * NPD_POLICY_STRIDE];
  __shared__ float mean[NPB_CONTROLS_AXES_MAX * NPD_POLICY_STRIDE], val[4 * NPD_POLICY_STRIDE];
  __shared__ double zs[NPB_CONTROLS_AXES_MAX * NPD_POLICY_TILE];
  __shared__ int bad[NPD_POLICY_TILE];
  const int tid = threadIdx.x, g = tid >> 5, r = tid & (NPD_POLICY_TILE - 1);
  const size_t base = (size_t)blockIdx.x * NPD_POLICY_TILE, rows = (size_t)R.rows;
  const int in_tile = npd_policy_in_tile(rows, base);
  const int KC = P.cells, KC_pad = (KC + 3) & ~3;
  /* 1. the tile's run of x into LDS, narrowed and transposed; the k extension +0.0 */
  if (tid < NPD_POLICY_TILE) bad[tid] = 0;
  npd_policy_tile_zero(xs, KC, KC_pad, tid);
  __syncthreads();
  npd_policy_tile_load((const IN *)R.x + base * (size_t)KC, in_tile, KC, xs, bad, tid);
  __syncthreads();
  /* 2. the nets */
  const int wave = tid >> 6, lane = tid & 63;
  if (R.act) npd_policy_net(P.actor, P.theta, P.padded, xs, ha, hb, mean, P.D.activation, wave, lane);
  npd_policy_net(P.critic, P.theta, P.padded, xs, ha, hb, val, P.D.activation, wave, lane);
  /* 3. the draw, then the outputs */
  npd_policy_epilogue(P, R, mean, val, zs, bad, g, r, in_tile, base);
}

/* ---- the launchers */
extern "C" void npb_policy_layout(const npb_policy_desc_t *D, int cells, int n_axes, npb_policy_t *P) { npb_policy_layout_at(D, cells, cells, n_axes, 0, 0, P); }
/* the same with the nets reading `in0` cells (a core's width) and their parameters behind `at` floats of theta and `wp` of the kernel's copy (the core's) */
extern "C" void npb_policy_layout_at(const npb_policy_desc_t *D, int cells, int in0, int n_axes, uint32_t at, uint32_t wp, npb_policy_t *P) {
  int widest = 0;
  for (int which = 0; which < 2; which++) {
    npd_policy_net_t &N = which ? P->critic : P->actor;
    const int hidden = which ? D->critic_layers : D->actor_layers;
    const int *width = which ? D->critic_width : D->actor_width;
    N.n_layers = hidden + 1;
    int in = in0;
    for (int l = 0; l <= hidden; l++) {
      npd_policy_layer_t &L = N.layer[l];
      L.in = in; L.in_pad = (in + 3) & ~3; L.out = l < hidden ? width[l] : which ? 1 : n_axes;
      L.w = at; at += (uint32_t)L.in * L.out;
      L.b = at; at += (uint32_t)L.out;
      L.out_pad = (L.out + 31) & ~31;
      L.wp = wp; wp += (uint32_t)L.in_pad * L.out_pad;
      if (l < hidden && L.out > widest) widest = L.out;
      in = L.out;
    }
  }
  P->log_std = at; P->std = at + (uint32_t)n_axes;
  P->theta_count = at + 2u * (uint32_t)n_axes;
  P->padded_count = wp;
  P->cells = cells; P->n_axes = n_axes; P->width_max = widest;
  P->D = *D;
}
extern "C" void npb_launch_policy_repack(const npb_policy_t *P, const npd_policy_core_t *C, hipStream_t stream) {
  npd_policy_repack_t K = {P->theta, P->padded, 0, {}};
  for (int l = 0; C && l < 6; l++) K.layer[K.n_layers++] = C->gate[l];
  for (int l = 0; l < P->actor.n_layers; l++) K.layer[K.n_layers++] = P->actor.layer[l];
  for (int l = 0; l < P->critic.n_layers; l++) K.layer[K.n_layers++] = P->critic.layer[l];
  const unsigned blocks = (P->padded_count + 255u) / 256u;      /* (with a core the count includes the gates' cells: the nets' lie behind them) */
  hipLaunchKernelGGL(npb_policy_repack_kernel, dim3(blocks < 64u ? blocks : 64u), dim3(256), 0, stream, K);
}
extern "C" void npb_launch_policy(const npb_policy_t *P, const npd_policy_run_t *R, hipStream_t stream) {
  const dim3 grid((unsigned)((R->rows + NPD_POLICY_TILE - 1) / NPD_POLICY_TILE)), block(NPD_POLICY_LANES);
  const bool small = npd_policy_small(P, 0);
#define NPD_POLICY_LAUNCH(IN, KC_MAX, H_MAX) hipLaunchKernelGGL((npb_policy_kernel<IN, KC_MAX, H_MAX>), grid, block, 0, stream, *P, *R)
  if (R->x_f64) { if (small) NPD_POLICY_LAUNCH(double, NPD_POLICY_SMALL_CELLS, NPD_POLICY_SMALL_WIDTH); else NPD_POLICY_LAUNCH(double, NPB_FEATURES_CELLS_MAX, NPB_POLICY_WIDTH_MAX); }
  else { if (small) NPD_POLICY_LAUNCH(float, NPD_POLICY_SMALL_CELLS, NPD_POLICY_SMALL_WIDTH); else NPD_POLICY_LAUNCH(float, NPB_FEATURES_CELLS_MAX, NPB_POLICY_WIDTH_MAX); }
#undef NPD_POLICY_LAUNCH
}
extern "C" void npb_launch_policy_noise(const npb_policy_t *P, uint64_t t, int n_plants, double *z, uint32_t *words, hipStream_t stream) {
  const size_t calls = (size_t)n_plants * ((P->n_axes + 1) / 2);
  hipLaunchKernelGGL(npb_policy_noise_kernel, dim3((unsigned)((calls + 255) / 256)), dim3(256), 0, stream, P->D.seed, (uint32_t)P->D.first_plant, t, n_plants,
                     P->n_axes, z, words);
}
