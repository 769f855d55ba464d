/* npd_rollout.h -- the rollout (npb_set_rollout, include/npb.h): what the policy saw, did and got for a horizon of T steps, written down
 * on the device in time-major buffers of the caller's, and the GAE advantages and returns over them in one launch.
 * nuclear_sim_amd/rollout.py states it in numpy; this file produces its bits: the recurrence runs in double with the product rounded
 * before the sum (-ffp-contract=off), the bootstrap and the carry are selects, the narrowing is the hardware's round-to-nearest-even.
 *
 * FOUR kernels, none of which touches the arena: compiled once, the same for either storage type (npb_storage_free.hip).
 * pre (in front of the controls kernel): three contiguous regions -- the features' out, the controls' in, the extras input -- into slot t
 *   in ONE launch: a flat grid-stride copy, consecutive lanes on consecutive 16-byte pieces where a region's two addresses allow (the
 *   launcher looks at them: a slot of an odd plant count x an odd cell count starts on 8 or 4 bytes), the words past the last whole piece
 *   by the first lanes.
 * post (behind features pass A, in front of the episode-records and episode kernels): one wave per 64 plants, one lane per plant.  The
 *   outcome as npb_episode_kernel decides it behind this kernel on the same columns, stated as npb_episode_records_kernel states it;
 *   reward, ended and episode of slot t with consecutive lanes on consecutive plants.  A truncated plant takes the next of ITS OWN R rows
 *   of final_obs (p * R + n_final[p]): no atomics, the assignment does not depend on the launch order.  Then the wave copies those plants'
 *   stacks, one after the other, all 64 lanes on a plant's K x C contiguous cells, 16 bytes per lane where K x C allows -- as features
 *   pass B copies a stack to `final`; no lane walks a row of its own.  A wave without a truncated plant ends after its stores.
 * cut: a byte OR into ended[t - 1] for the plants of a mask.
 * advantages: one lane per plant, backwards over the slots [0, t); every access has consecutive lanes on consecutive plants (the value
 *   column with its plant stride).  A slot's loads do not depend on the recurrence: they are issued NPD_ROLLOUT_AHEAD slots at a time --
 *   reward, ended, value, and for a truncated slot its row and that row's final value -- and only then the dependent chain of those
 *   slots runs, two multiplications and four additions per slot.  Not a scan: that would change the rounding.
 * No scratch, no atomics, no LDS. */
#ifndef NPD_ROLLOUT_H
#define NPD_ROLLOUT_H

#define NPD_ROLLOUT_AHEAD 8        /* slots whose loads are in flight before their chain runs */
#define NPD_ROLLOUT_PRE_BLOCKS 2048

/* one region of the pre kernel's launch: `bytes` (a multiple of 4) from src to dst, `width` bytes per lane (16, 8 or 4: what both
 * addresses are aligned to); bytes 0 = nothing */
typedef struct { const void *src; void *dst; size_t bytes; int width; } npb_rollout_copy_t;
struct npd_rollout_pre_t { npb_rollout_copy_t c[3]; };

template <typename V> __device__ __forceinline__ void npd_rollout_copy(const npb_rollout_copy_t &c, size_t first, size_t stride) {
  const size_t pieces = c.bytes / sizeof(V), words = c.bytes / 4u, per = sizeof(V) / 4u;
  const V *src = (const V *)c.src;
  V *dst = (V *)c.dst;
  for (size_t i = first; i < pieces; i += stride) dst[i] = src[i];
  for (size_t w = pieces * per + first; w < words; w += stride) ((uint32_t *)c.dst)[w] = ((const uint32_t *)c.src)[w];
}
__global__ __launch_bounds__(256) void npb_rollout_pre_kernel(npd_rollout_pre_t P) {
  const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const npb_rollout_copy_t &c = P.c[r];
    if (!c.bytes) continue;
    if (c.width == 16) npd_rollout_copy<uint4>(c, first, stride);
    else if (c.width == 8) npd_rollout_copy<uint2>(c, first, stride);
    else npd_rollout_copy<uint32_t>(c, first, stride);
  }
}
static npb_rollout_copy_t npd_rollout_region(const void *src, void *dst, size_t bytes) {
  const uintptr_t both = (uintptr_t)src | (uintptr_t)dst;
  return npb_rollout_copy_t{src, dst, src && dst ? bytes : 0, (both & 15u) == 0 ? 16 : (both & 7u) == 0 ? 8 : 4};
}
extern "C" void npb_launch_rollout_pre(const npb_rollout_t *R, const void *feat_out, const void *ctl_in, int n_plants, hipStream_t stream) {
  const size_t n = (size_t)n_plants, t = (size_t)R->t;
  const size_t obs = n * R->cells * R->obs_bytes, act = n * R->n_axes * R->act_bytes, extra = n * R->D.n_extras * sizeof(float);
  npd_rollout_pre_t P;
  P.c[0] = npd_rollout_region(feat_out, (char *)R->D.obs + t * obs, obs);
  P.c[1] = npd_rollout_region(ctl_in, R->D.act ? (char *)R->D.act + t * act : nullptr, act);
  P.c[2] = npd_rollout_region(R->D.extras_in, R->D.extra ? (char *)R->D.extra + t * extra : nullptr, extra);
  size_t most = 1;
  for (int r = 0; r < 3; r++) { const size_t pieces = (P.c[r].bytes + P.c[r].width - 1) / P.c[r].width; most = pieces > most ? pieces : most; }
  const size_t blocks = (most + 255) / 256;
  hipLaunchKernelGGL(npb_rollout_pre_kernel, dim3((unsigned)(blocks < NPD_ROLLOUT_PRE_BLOCKS ? blocks : NPD_ROLLOUT_PRE_BLOCKS)), dim3(256), 0, stream, P);
}

/* the post kernel's arguments: the step's columns, the carried counters (NULL without autoreset), the slot's rows of the caller's buffers
 * (already moved to slot t), and the terminal stacks */
struct npd_rollout_post_t {
  const double *reward; const uint8_t *done; const int32_t *len, *index; int max_steps, n_plants, cells, final_rows;
  double *reward_out; uint8_t *ended_out; int32_t *episode_out, *final_row_out, *n_final;
  const void *out; void *final_obs;
};
template <typename OUT, int W>
__global__ __launch_bounds__(NPB_WAVE) void npb_rollout_post_kernel(npd_rollout_post_t P) {
  typedef npd_features_vec<OUT, W> V;
  const size_t block_base = (size_t)blockIdx.x * NPB_WAVE;
  const int lane = threadIdx.x;
  const size_t p = block_base + lane;
  int32_t row = -1;
  if (p < (size_t)P.n_plants) {           /* the outcome as npb_episode_kernel decides it, behind this kernel on the same columns */
    const bool terminated = P.done[p] != 0;
    const bool truncated = P.len && P.max_steps > 0 && P.len[p] + 1 >= P.max_steps && !terminated;     /* termination wins */
    P.reward_out[p] = P.reward[p];
    P.ended_out[p] = (uint8_t)((terminated ? NPB_ROLLOUT_TERMINATED : 0) | (truncated ? NPB_ROLLOUT_TRUNCATED : 0));
    P.episode_out[p] = P.index ? P.index[p] : -1;
    if (truncated) {
      const int32_t taken = P.n_final[p];
      if (taken < P.final_rows) {         /* (always, while max_steps is what npb_step checked R against since npb_rollout_begin) */
        row = (int32_t)p * P.final_rows + taken;
        P.n_final[p] = taken + 1;
        P.final_row_out[p] = row;
      }
    }
  }
  /* the truncated plants' stacks, terminal frame included: one plant after the other, all 64 lanes on its K x C cells */
  const OUT *out = (const OUT *)P.out;
  OUT *final_obs = (OUT *)P.final_obs;
  for (uint64_t left = __ballot(row >= 0); left; left &= left - 1) {
    const int r = __ffsll((unsigned long long)left) - 1;
    const OUT *src = out + (block_base + (size_t)r) * (size_t)P.cells;
    OUT *dst = final_obs + (size_t)__shfl(row, r) * (size_t)P.cells;
    for (int i = lane * W; i < P.cells; i += NPB_WAVE * W) *(V *)(dst + i) = *(const V *)(src + i);
  }
}
/* W: 16 bytes per lane where every stack is a whole number of them and both tensors are 16-byte aligned, else one element */
extern "C" void npb_launch_rollout_post(const npb_rollout_t *R, const void *feat_out, const double *reward, const uint8_t *done, const int32_t *len,
                                        const int32_t *index, int max_steps, int n_plants, hipStream_t stream) {
  const size_t slot = (size_t)R->t * (size_t)n_plants;
  npd_rollout_post_t P;
  P.reward = reward; P.done = done; P.len = len; P.index = index; P.max_steps = max_steps; P.n_plants = n_plants; P.cells = R->cells;
  P.final_rows = R->D.final_obs ? R->D.final_rows : 0;
  P.reward_out = R->D.reward + slot; P.ended_out = R->D.ended + slot; P.episode_out = R->D.episode + slot; P.final_row_out = R->D.final_row + slot;
  P.n_final = R->n_final; P.out = feat_out; P.final_obs = R->D.final_obs;
  const dim3 grid((unsigned)((n_plants + NPB_WAVE - 1) / NPB_WAVE)), block(NPB_WAVE);
  const bool f64 = R->obs_bytes == 8;
  const bool wide = R->cells % (f64 ? 2 : 4) == 0 && (((uintptr_t)feat_out | (uintptr_t)R->D.final_obs) & 15u) == 0;
#define NPD_ROLLOUT_POST(OUT, W) hipLaunchKernelGGL((npb_rollout_post_kernel<OUT, W>), grid, block, 0, stream, P)
  if (f64) { if (wide) NPD_ROLLOUT_POST(double, 2); else NPD_ROLLOUT_POST(double, 1); }
  else { if (wide) NPD_ROLLOUT_POST(float, 4); else NPD_ROLLOUT_POST(float, 1); }
#undef NPD_ROLLOUT_POST
}

__global__ __launch_bounds__(256) void npb_rollout_cut_kernel(uint8_t *__restrict__ ended, const uint8_t *__restrict__ mask, int n_plants) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)n_plants || (mask && !mask[p])) return;
  ended[p] |= (uint8_t)NPB_ROLLOUT_CUT;
}
extern "C" void npb_launch_rollout_cut(const npb_rollout_t *R, const uint8_t *mask, int n_plants, hipStream_t stream) {
  hipLaunchKernelGGL(npb_rollout_cut_kernel, dim3((unsigned)((n_plants + 255) / 256)), dim3(256), 0, stream,
                     R->D.ended + (size_t)(R->t - 1) * (size_t)n_plants, mask, n_plants);
}

struct npd_rollout_adv_t {
  const double *reward; const uint8_t *ended; const int32_t *final_row;
  const float *value, *last_value, *final_value; int64_t value_time_stride, value_plant_stride;
  void *adv, *ret; double gamma, gl; int n_plants, t_end; int64_t n_rows;
};
template <typename OUT>
__global__ __launch_bounds__(256) void npb_rollout_advantages_kernel(npd_rollout_adv_t G) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)G.n_plants;
  if (p >= n) return;
  OUT *adv = (OUT *)G.adv, *ret = (OUT *)G.ret;
  const float *value = G.value + (int64_t)p * G.value_plant_stride;      /* (read only where G.value is set) */
  double a_next = 0.0;                                             /* A behind the slot in hand */
  double v_next = G.last_value ? (double)G.last_value[p] : 0.0;    /* the value behind it */
  for (int t = G.t_end; t > 0; t -= NPD_ROLLOUT_AHEAD) {          /* the slots t - 1, t - 2, ... of this group */
    double rw[NPD_ROLLOUT_AHEAD], fv[NPD_ROLLOUT_AHEAD];
    float vf[NPD_ROLLOUT_AHEAD];                                   /* as loaded: widened where the chain takes it, so no load is waited for here */
    unsigned e[NPD_ROLLOUT_AHEAD];
#pragma unroll
    for (int u = 0; u < NPD_ROLLOUT_AHEAD; u++) {
      const int s = t - 1 - u;
      rw[u] = fv[u] = 0.0; vf[u] = 0.0f; e[u] = 0u;
      if (s < 0) continue;
      const size_t cell = (size_t)s * n + p;
      rw[u] = G.reward[cell];
      e[u] = G.ended[cell];
      if (G.value) vf[u] = value[(int64_t)s * G.value_time_stride];
    }
    /* (the truncated slots' rows wait for `ended`: asked for only when every load above is on its way) */
#pragma unroll
    for (int u = 0; u < NPD_ROLLOUT_AHEAD; u++) {
      const int s = t - 1 - u;
      if (s < 0 || !(e[u] & NPB_ROLLOUT_TRUNCATED) || !G.final_value) continue;
      const int64_t row = G.final_row[(size_t)s * n + p];
      if (row >= 0 && row < G.n_rows) fv[u] = (double)G.final_value[row];
    }
#pragma unroll
    for (int u = 0; u < NPD_ROLLOUT_AHEAD; u++) {
      const int s = t - 1 - u;
      if (s < 0) continue;
      const size_t cell = (size_t)s * n + p;
      const double v = (double)vf[u];
      const double nv = (e[u] & (NPB_ROLLOUT_TERMINATED | NPB_ROLLOUT_CUT)) ? 0.0 : (e[u] & NPB_ROLLOUT_TRUNCATED) ? fv[u] : v_next;
      const double bootstrap = G.gamma * nv;
      const double target = rw[u] + bootstrap;
      const double delta = target - v;
      const double carry = (e[u] & 7u) ? 0.0 : a_next;
      const double carried = G.gl * carry;
      const double a = delta + carried;
      if (adv) adv[cell] = (OUT)a;
      if (ret) ret[cell] = (OUT)(a + v);
      a_next = a;
      v_next = v;
    }
  }
}
extern "C" void npb_launch_rollout_advantages(const npb_rollout_t *R, const npb_rollout_advantages_desc_t *A, double gl, int n_plants, hipStream_t stream) {
  npd_rollout_adv_t G;
  G.reward = R->D.reward; G.ended = R->D.ended; G.final_row = R->D.final_row;
  G.value = A->value; G.last_value = A->last_value; G.final_value = A->final_value;
  G.value_time_stride = A->value_time_stride; G.value_plant_stride = A->value_plant_stride;
  G.adv = A->adv; G.ret = A->ret; G.gamma = A->gamma; G.gl = gl; G.n_plants = n_plants; G.t_end = R->t;
  G.n_rows = (int64_t)n_plants * (R->D.final_obs ? R->D.final_rows : 0);
  const dim3 grid((unsigned)((n_plants + 255) / 256)), block(256);
  if (A->out_type == NPB_ROLLOUT_F64) hipLaunchKernelGGL(npb_rollout_advantages_kernel<double>, grid, block, 0, stream, G);
  else hipLaunchKernelGGL(npb_rollout_advantages_kernel<float>, grid, block, 0, stream, G);
}
#endif
