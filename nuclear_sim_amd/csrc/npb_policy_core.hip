/* npb_policy_core.hip -- the recurrent policy on the device (npb_set_policy_core, include/npb.h): a GRU cell of width H in front of the actor
 * and the critic, its hidden state carried per plant, in the ONE launch in front of every step that npb_policy.hip's kernel is without a core.
 * nuclear_sim_amd/recurrent.py states it in numpy; this file produces its bits (the float tanh of the soft gates apart, which the statement
 * licenses): the six gate pre-activations are layers of npd_policy_layer -- bias, then fmaf(x[k], W[j][k], acc) for k ascending, on the f32
 * matrix cores -- and the combines are plain float operations, each rounded on its own.  Built with the policy's flags (Makefile): no
 * contraction, IEEE division and square root.
 *
 * One workgroup of 256 lanes (four waves) per tile of 32 plants, npb_policy.hip's geometry and LDS layout: every buffer [k][plant], row
 * stride 33.
 *   1. lanes 0 .. 31 read their plant's restart words: h starts at +0.0 where the plant is unprimed or its carried episode index is not the
 *      one seen (npd_controls.h's rule); a step that acts primes the plant and remembers the index, the same lane storing what it read.
 *      The tile's rows of x and of h are ONE contiguous run each (32 x K*C and 32 x H): consecutive lanes on consecutive elements, narrowed
 *      and transposed into LDS (xs, hs); a restarted plant's column of hs is +0.0; on the rollout's slot 0 the run goes out again, as read,
 *      into `first` (and on a slot that begins a segment, npb_policy_core_segments, into that segment's row of the stored states).  The k
 *      extensions of xs and hs are +0.0.  The load of x, the zeroing and the ragged tile's row count are the MLP
 *      kernel's own (npb_policy.h: npd_policy_tile_load, npd_policy_tile_zero, npd_policy_in_tile); the load of h, with its restart
 *      mask and its store into `first`, is this file's.
 *   2. the cell, gate by gate, so that only H-wide buffers live in LDS: npb_policy.h's npd_core_cell, the one statement of it that the
 *      training kernels (npb_ppo_seq.hip) run too -- gi into ha, gh into hb, r into rs, z into zg, h' over hs in place.  Cells from H up to
 *      the next multiple of 4 are +0.0: the next layer's k extension.  A poisoned plant's h' is +0.0.
 *   3. h' goes back to the per-plant buffer as it came: the tile's run, read out of hs transposed (npb_policy.h's npd_core_store).
 *   4. the actor and the critic over hs with ha and hb as their ping-pong buffers, and the epilogue: npb_policy.h's, the MLP kernel's own.
 * npb_policy_values_hidden is the same kernel with act == NULL: the critic over GRU(x, h), nothing written back to h, primed or seen.
 * LDS, from the declarations below: (KC_MAX + 5 H_MAX) x 33 x 4 B for xs, hs, ha, hb, rs, zg, and the epilogue's 1056 + 528 + 2048 + 128 B
 * with 256 B of poison and restart words: the small build (NPD_POLICY_SMALL_CELLS, NPD_POLICY_SMALL_WIDTH; npd_policy_small with the core's
 * width, npb_policy.h) 54 576 B, the large one (NPB_FEATURES_CELLS_MAX, NPB_POLICY_WIDTH_MAX) 122 160 B, as the compiler reports them --
 * static, beyond 64 KiB, inside gfx950's 160 KiB per CU (one workgroup a CU in the large build, three in the small one).  A 3H-wide gi and
 * gh together would not fit.  57 VGPRs and 16 AGPRs, no scratch, no spills, no atomics.  The gate layers' copy for the matrix cores is laid out by the policy's
 * one repack launch (npb_launch_policy_repack, npb_policy.hip), together with the nets'. */
#include <hip/hip_runtime.h>
#include <math.h>
#include "npb_policy.h"

template <typename IN, int KC_MAX, int H_MAX>
__global__ __launch_bounds__(NPD_POLICY_LANES) void npb_policy_core_kernel(npb_policy_t P, npd_policy_core_t C, npd_policy_run_t R, npd_policy_core_run_t G) {
  __shared__ float xs[KC_MAX * NPD_POLICY_STRIDE];
  __shared__ float hs[H_MAX * NPD_POLICY_STRIDE], ha[H_MAX * NPD_POLICY_STRIDE], hb[H_MAX * NPD_POLICY_STRIDE];
  __shared__ float rs[H_MAX * NPD_POLICY_STRIDE], zg[H_MAX * NPD_POLICY_STRIDE];
  __shared__ float mean[NPB_CONTROLS_AXES_MAX * NPD_POLICY_STRIDE], val[4 * NPD_POLICY_STRIDE];
  __shared__ double zs[NPB_CONTROLS_AXES_MAX * NPD_POLICY_TILE];
  __shared__ int bad[NPD_POLICY_TILE], fresh[NPD_POLICY_TILE];
  const int tid = threadIdx.x, g = tid >> 5, r = tid & (NPD_POLICY_TILE - 1);
  const size_t base = (size_t)blockIdx.x * NPD_POLICY_TILE, rows = (size_t)R.rows;
  const int in_tile = npd_policy_in_tile(rows, base);
  const int KC = P.cells, KC_pad = (KC + 3) & ~3, H = C.H, H_pad = (H + 3) & ~3;
  /* 1. the restart words; the tile's runs of x and h into LDS, narrowed and transposed; the k extensions +0.0 */
  if (tid < NPD_POLICY_TILE) {
    int restart = 0;
    if (G.primed && tid < in_tile) {
      const size_t p = base + tid;
      const int32_t seen = G.seen[p], episode = G.index ? G.index[p] : seen;
      restart = !(G.primed[p] != 0 && episode == seen);
      if (G.remember) { G.primed[p] = 1; G.seen[p] = episode; }
    }
    bad[tid] = 0;
    fresh[tid] = restart;
  }
  npd_policy_tile_zero(xs, KC, KC_pad, tid);
  npd_policy_tile_zero(hs, H, H_pad, tid);
  __syncthreads();
  npd_policy_tile_load((const IN *)R.x + base * (size_t)KC, in_tile, KC, xs, bad, tid);
  const int h_total = in_tile * H;
  const float *h_run = G.h + base * (size_t)H;
  for (int e = tid; e < h_total; e += NPD_POLICY_LANES) {
    const int row = e / H, k = e - row * H;
    const float v = fresh[row] ? 0.0f : h_run[e];
    hs[k * NPD_POLICY_STRIDE + row] = v;
    if (G.first_out) G.first_out[base * (size_t)H + e] = v;
    if (G.start_out) G.start_out[base * (size_t)H + e] = v;
  }
  __syncthreads();
  /* 2. the cell, gate by gate (npb_policy.h) */
  const int wave = tid >> 6, lane = tid & 63;
  npd_core_cell(P, C, xs, hs, ha, hb, rs, zg, bad, tid);
  /* 3. h' back to the per-plant buffer */
  if (G.h_out) npd_core_store(G.h_out + base * (size_t)H, hs, in_tile, H, tid);
  /* 4. the nets over h', the draw and the outputs */
  if (R.act) npd_policy_net(P.actor, P.theta, P.padded, hs, ha, hb, mean, P.D.activation, wave, lane);
  npd_policy_net(P.critic, P.theta, P.padded, hs, ha, hb, val, P.D.activation, wave, lane);
  npd_policy_epilogue(P, R, mean, val, zs, bad, g, r, in_tile, base);
}

/* behind the rollout's post kernel: one wave per 64 plants, one lane per plant reads the row its plant took in this slot (-1: none); then the
 * wave copies those plants' H cells, one plant after the other, consecutive lanes on consecutive cells */
__global__ __launch_bounds__(64) void npb_policy_core_final_kernel(const float *__restrict__ hidden, float *__restrict__ final, const int32_t *__restrict__ final_row,
                                                                   int n_plants, int H, int64_t n_rows) {
  const size_t block_base = (size_t)blockIdx.x * 64;
  const int lane = threadIdx.x;
  const size_t p = block_base + lane;
  int32_t row = -1;
  if (p < (size_t)n_plants) row = final_row[p];
  if (row >= n_rows) row = -1;
  for (uint64_t left = __ballot(row >= 0); left; left &= left - 1) {
    const int r = __ffsll((unsigned long long)left) - 1;
    const float *src = hidden + (block_base + (size_t)r) * (size_t)H;
    float *dst = final + (size_t)__shfl(row, r) * (size_t)H;
    for (int i = lane; i < H; i += 64) dst[i] = src[i];
  }
}

/* ---- the launchers */
extern "C" void npb_policy_core_layout(int H, int gates, int cells, npd_policy_core_t *C) {
  uint32_t at = 0, wp = 0;
  C->H = H; C->gates = gates;
  for (int block = 0; block < 2; block++) {      /* W_ih | b_ih, then W_hh | b_hh: three row blocks of H each, r, z, n */
    const int in = block ? H : cells;
    const uint32_t w = at, b = at + 3u * (uint32_t)H * (uint32_t)in;
    at = b + 3u * (uint32_t)H;
    for (int gate = 0; gate < 3; gate++) {
      npd_policy_layer_t &L = C->gate[3 * block + gate];
      L.in = in; L.in_pad = (in + 3) & ~3; L.out = H; L.out_pad = (H + 31) & ~31;
      L.w = w + (uint32_t)gate * (uint32_t)H * (uint32_t)in;
      L.b = b + (uint32_t)gate * (uint32_t)H;
      L.wp = wp; wp += (uint32_t)L.in_pad * L.out_pad;
    }
  }
  C->theta_count = at; C->padded_count = wp;
}
extern "C" void npb_launch_policy_core(const npb_policy_t *P, const npd_policy_core_t *C, const npd_policy_run_t *R, const npd_policy_core_run_t *G, hipStream_t stream) {
  const dim3 grid((unsigned)((R->rows + NPD_POLICY_TILE - 1) / NPD_POLICY_TILE)), block(NPD_POLICY_LANES);
  const bool small = npd_policy_small(P, C->H);
#define NPD_CORE_LAUNCH(IN, KC_MAX, H_MAX) hipLaunchKernelGGL((npb_policy_core_kernel<IN, KC_MAX, H_MAX>), grid, block, 0, stream, *P, *C, *R, *G)
  if (R->x_f64) { if (small) NPD_CORE_LAUNCH(double, NPD_POLICY_SMALL_CELLS, NPD_POLICY_SMALL_WIDTH); else NPD_CORE_LAUNCH(double, NPB_FEATURES_CELLS_MAX, NPB_POLICY_WIDTH_MAX); }
  else { if (small) NPD_CORE_LAUNCH(float, NPD_POLICY_SMALL_CELLS, NPD_POLICY_SMALL_WIDTH); else NPD_CORE_LAUNCH(float, NPB_FEATURES_CELLS_MAX, NPB_POLICY_WIDTH_MAX); }
#undef NPD_CORE_LAUNCH
}
extern "C" void npb_launch_policy_core_final(const npd_policy_core_t *C, const int32_t *final_row, int n_plants, hipStream_t stream) {
  hipLaunchKernelGGL(npb_policy_core_final_kernel, dim3((unsigned)((n_plants + 63) / 64)), dim3(64), 0, stream, C->hidden, C->final, final_row, n_plants, C->H,
                     (int64_t)n_plants * C->final_rows);
}
