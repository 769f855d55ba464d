/* npb_ppo.hip -- training the policy on the device (npb_policy_grad, npb_policy_adam, include/npb.h): the clipped surrogate loss of one
 * minibatch, its gradient through both MLPs, the gradient's clipping and one Adam step.  nuclear_sim_amd/ppo.py states it in numpy; this
 * file produces its bits for a relu net fed the device's own ratio (the float tanh, and the double exp of the ratio and of std, are the
 * statement's licensed differences).  Built with the noise generator's flags (Makefile): no contraction, IEEE division and square root.
 *
 * THE GRADIENT KERNEL: one workgroup of 256 lanes (four waves) runs one CHAIN of rows_per_chain rows, tile of 32 rows after tile, and a
 * launch's workgroups stride over the chains; a chain's sums are the same whichever workgroup runs it and whenever.  Per tile:
 *   1. the tile's rows of obs into LDS as the step's launch lays them, xs[k][row] with a row stride of 33; a row beyond count, and a
 *      skipped row (a feature, an action, logp_old, adv or ret that is not finite), reads as +0.0 everywhere.  The zeroing and the load
 *      are the step's (npb_policy.h: npd_policy_tile_zero, npd_policy_tile_load, its float or double instance picked once a tile).
 *   2. the actor forward by the step's own layer routine (npd_policy_layer, npb_policy.h), every hidden activation kept in LDS, h[l][k][row].
 *   3. the per-row epilogue in double, a lane a row: the head's seeds dmean[a][row] as floats into LDS, the per-row doubles (dls, the
 *      losses' terms) into LDS, logp_new and ratio out.
 *   4. the actor backward, from the head down.  dW (npd_ppo_dw): v_mfma_f32_32x32x2_f32 with the output index j as the row of D, the input
 *      index k as its column and the tile's ROWS as the k dimension, two rows a call in ascending order: the statement's chain.  A wave
 *      takes blocks of 32 x 32 of a layer's W; the accumulator of a block is the chain's own row of the partials workspace, in theta's
 *      layout: loaded as the C operand (+0.0 in the chain's first tile), sixteen calls, stored with plain vector stores -- a lane holds one
 *      k of 16 j, so a half-wave stores 128 contiguous bytes.  db: a lane an output, the 32 rows added in order.  back (npd_ppo_back): the
 *      row as the row of D, k as its column, j as the k dimension; theta's own row-major W[j][k] IS the B operand, consecutive lanes on
 *      consecutive k; then the activation's derivative from h, and delta'[k][row] into the other of two LDS buffers.
 *   5. the critic the same way, its hidden activations over the actor's: forward, the value's seed and loss (with clip_vf > 0 the
 *      clipped branch: the larger of the two squares and its own derivative), the four terms of explained_variance, backward.
 *   6. the per-row doubles of the tile added in row order onto the chain's running sums, a lane a quantity.
 * No atomics, nothing depends on the launch order, no scratch.  LDS: the small build (npd_policy_small, npb_policy.h: K*C <=
 * NPD_POLICY_SMALL_CELLS, widths <= NPD_POLICY_SMALL_WIDTH) 6 x 8.25 KiB and 6 KiB; the large one 33 + 5 x 16.5 KiB and the same, 122 KiB
 * of gfx950's 160.
 * THE REDUCE KERNEL: a lane a parameter: its partials widened and added in ascending chain order, narrowed once; log_std's from the dls
 * sums; then the first level of the pinned tree over the squares.  THE FINISH KERNEL, one workgroup: the tree's further levels, the norm,
 * the scale, the statistics, and with a gate armed (kl_limit > 0) the gate: one lane ORs approx_kl > kl_limit into the training block's
 * stopped word and counts an applied update, with ordinary stores.  THE ADAM KERNEL: a lane a parameter, and log_std's lane refreshes
 * std; its gated twin reads the stopped word first and stores nothing when it is set.
 * ACROSS SHARDS (npb_policy_shard_sums, npb_policy_apply_shards): the update cut where the double sums end.  The gradient kernel divides
 * its seeds by R.n, (double)count of a plain call and (double)count_total of a shard's.  THE SHARD REDUCE KERNEL: a lane an entry of the
 * shard's vector: the reduce kernel's ascending sum over the chains, stored as the double it is.  THE COMBINE KERNEL: a lane a parameter:
 * the shards' entries added in ascending shard order onto 0.0, narrowed once, then as the reduce kernel.  The finish kernel's second
 * instance reads the 18 totals' rows out of the shards' vectors and divides by count_total; the plain instance is the code it was. */
#include <hip/hip_runtime.h>
#include <math.h>
#include "npb_ppo.h"
#include "npb_minibatch.h"

template <int KC_MAX, int H_MAX>
__global__ __launch_bounds__(NPD_POLICY_LANES) void npb_ppo_grad_kernel(npb_policy_t P, npd_ppo_run_t R) {
  __shared__ float xs[KC_MAX * NPD_POLICY_STRIDE];
  __shared__ float hid[NPB_POLICY_HIDDEN_MAX][H_MAX * NPD_POLICY_STRIDE];
  __shared__ float da[H_MAX * NPD_POLICY_STRIDE], db[H_MAX * NPD_POLICY_STRIDE];
  __shared__ float head[NPB_CONTROLS_AXES_MAX * NPD_POLICY_STRIDE];
  __shared__ double rowv[NPD_PPO_ROWVALS * NPD_POLICY_TILE];
  __shared__ int bad[NPD_POLICY_TILE];
  const npb_ppo_desc_t &D = R.D;
  const int tid = threadIdx.x, A = P.n_axes, KC = P.cells, KC_pad = (KC + 3) & ~3;
  const size_t count = (size_t)D.count, rpc = (size_t)D.rows_per_chain;
  const double n = R.n;
  for (size_t chain = blockIdx.x; chain < (size_t)R.n_chains; chain += gridDim.x) {
    float *prow = R.partials + chain * R.floats;
    double running = 0.0;      /* lane q < NPD_PPO_ROWVALS: the chain's sum of per-row double q */
    for (size_t base = chain * rpc; base < (chain + 1) * rpc && base < count; base += NPD_POLICY_TILE) {
      const bool first = base == chain * rpc;
      const int in_tile = npd_policy_in_tile(count, base);
      /* 1. the rows: +0.0 everywhere, then the tile's run of obs, then the skipped rows back to +0.0 */
      __syncthreads();      /* (the tile before is done with every buffer) */
      npd_policy_tile_zero(xs, 0, KC_pad, tid);
      for (int i = tid; i < NPD_PPO_ROWVALS * NPD_POLICY_TILE; i += NPD_POLICY_LANES) rowv[i] = 0.0;
      if (tid < NPD_POLICY_TILE) {
        int b = 0;
        if (tid < in_tile) {
          const size_t p = base + tid;
          const double old = (double)D.logp_old[p], adv = npd_ppo_load(D.adv, D.adv_type, p), ret = npd_ppo_load(D.ret, D.adv_type, p);
          b = !(old - old == 0.0) || !(adv - adv == 0.0) || !(ret - ret == 0.0);
          if (R.M.clip_vf > 0.0) { const float vo = R.M.value_old[p]; b |= !(vo - vo == 0.0f); }
          for (int a = 0; a < A; a++) { const double x = npd_ppo_load(D.act, D.act_type, p * A + a); b |= !(x - x == 0.0); }
        }
        bad[tid] = b;
      }
      __syncthreads();
      if (D.obs_type) npd_policy_tile_load((const double *)D.obs + base * KC, in_tile, KC, xs, bad, tid);
      else npd_policy_tile_load((const float *)D.obs + base * KC, in_tile, KC, xs, bad, tid);
      __syncthreads();
      for (int i = tid; i < KC * NPD_POLICY_TILE; i += NPD_POLICY_LANES)
        if (bad[i & 31]) xs[(i >> 5) * NPD_POLICY_STRIDE + (i & 31)] = 0.0f;
      __syncthreads();
      const bool live = tid < in_tile, skipped = tid < NPD_POLICY_TILE && bad[tid & 31] != 0;
      const size_t p = base + tid;
      /* 2 .. 4. the actor */
      npd_ppo_net<H_MAX>(P.actor, P, xs, hid, head, da, db, prow, first, tid, nullptr, [&]() { npd_ppo_seeds_actor(P, D, n, head, da, rowv, tid, live, skipped, p); });
      /* 5. the critic */
      npd_ppo_net<H_MAX>(P.critic, P, xs, hid, head, da, db, prow, first, tid, nullptr, [&]() { npd_ppo_seeds_critic(P, D, R.M, n, head, da, rowv, tid, live, skipped, p); });
      /* 6. the tile's per-row doubles onto the chain's sums, rows ascending */
      if (tid < NPD_PPO_ROWVALS)
        for (int r = 0; r < NPD_POLICY_TILE; r++) running = running + rowv[tid * NPD_POLICY_TILE + r];
    }
    if (tid < NPD_PPO_ROWVALS) R.chain_stats[chain * NPD_PPO_ROWVALS + tid] = running;
  }
}

/* a lane a parameter: the ascending sum over the chains, narrowed once; log_std's gradient from the dls sums; std's 0; and the first level
 * of the pinned tree over the squares of every entry but std's (a workgroup IS a group of 256) */
__global__ __launch_bounds__(NPD_TREE) void npb_ppo_reduce_kernel(npb_policy_t P, npd_ppo_run_t R, npb_ppo_t O) {
  __shared__ double s[NPD_TREE];
  const int lane = threadIdx.x;
  const size_t e = (size_t)blockIdx.x * NPD_TREE + lane;
  float g = 0.0f;
  if (e < P.log_std) {
    double sum = 0.0;
    for (int c = 0; c < R.n_chains; c++) sum = sum + (double)R.partials[(size_t)c * R.floats + e];
    g = (float)sum;
  } else if (e < P.std) {
    double sum = 0.0;
    for (int c = 0; c < R.n_chains; c++) sum = sum + R.chain_stats[(size_t)c * NPD_PPO_ROWVALS + (e - P.log_std)];
    g = (float)(sum - R.D.ent_coef);
  }
  if (e < P.theta_count) O.grad[e] = g;
  s[lane] = e < P.std ? (double)g * (double)g : 0.0;
  npd_tree_group(s, lane);
  if (lane == 0 && (size_t)blockIdx.x * NPD_TREE < P.std) O.tree[blockIdx.x] = s[0];
}

/* a shard's vector (npb_policy_shard_sums): a lane an entry, the reduce kernel's ascending sums over the chains stored as doubles: the
 * weights' and biases' from the partials, then the NPD_PPO_ROWVALS per-row sums.  Plain vector stores */
__global__ __launch_bounds__(NPD_TREE) void npb_ppo_shard_reduce_kernel(npb_policy_t P, npd_ppo_run_t R, double *__restrict__ out) {
  const size_t e = (size_t)blockIdx.x * NPD_TREE + threadIdx.x;
  if (e >= (size_t)P.log_std + NPD_PPO_ROWVALS) return;
  double sum = 0.0;
  if (e < P.log_std) for (int c = 0; c < R.n_chains; c++) sum = sum + (double)R.partials[(size_t)c * R.floats + e];
  else for (int c = 0; c < R.n_chains; c++) sum = sum + R.chain_stats[(size_t)c * NPD_PPO_ROWVALS + (e - P.log_std)];
  out[e] = sum;
}

/* the combine (npb_policy_apply_shards): a lane a parameter: its entry of every shard's vector added in ascending shard order onto 0.0,
 * narrowed once (dls[a] sits at log_std[a]'s own index of the vector; its lane subtracts ent_coef first); std's 0; and the first level
 * of the pinned tree, as the reduce kernel */
__global__ __launch_bounds__(NPD_TREE) void npb_ppo_combine_kernel(npb_policy_t P, npd_ppo_run_t R, npb_ppo_t O) {
  __shared__ double s[NPD_TREE];
  const int lane = threadIdx.x;
  const size_t e = (size_t)blockIdx.x * NPD_TREE + lane;
  float g = 0.0f;
  if (e < P.std) {
    double sum = 0.0;
    for (int w = 0; w < R.n_shards; w++) sum = sum + R.shards[(size_t)w * R.shard_len + e];
    g = e < P.log_std ? (float)sum : (float)(sum - R.ent_coef);
  }
  if (e < P.theta_count) O.grad[e] = g;
  s[lane] = e < P.std ? (double)g * (double)g : 0.0;
  npd_tree_group(s, lane);
  if (lane == 0 && (size_t)blockIdx.x * NPD_TREE < P.std) O.tree[blockIdx.x] = s[0];
}

/* one workgroup: the tree's further levels, the norm, the scale over every entry but std's, the statistics (the chains' sums first, a
 * lane a quantity, so that no two of them wait for each other inside one wave), the gate */
template <bool SHARDS>
__global__ __launch_bounds__(NPD_TREE) void npb_ppo_finish_kernel(npb_policy_t P, npd_ppo_run_t R, npb_ppo_t O) {
  __shared__ double s[NPD_TREE], sums[NPD_PPO_ROWVALS];
  const int lane = threadIdx.x;
  const double *in = npd_tree_levels(O.tree, ((size_t)P.std + NPD_TREE - 1) / NPD_TREE, s, lane);
  const double norm = sqrt(in[0]);
  /* every per-row quantity's sum over the chains, ascending, a lane a quantity: one pass of coalesced loads, the waves beyond the first
   * already scaling */
  if (lane < NPD_PPO_ROWVALS) {
    double sum = 0.0;
    if (SHARDS) for (int w = 0; w < R.n_shards; w++) sum = sum + R.shards[(size_t)w * R.shard_len + P.log_std + lane];
    else for (int c = 0; c < R.n_chains; c++) sum = sum + R.chain_stats[(size_t)c * NPD_PPO_ROWVALS + lane];
    sums[lane] = sum;
  }
  if (R.D.max_grad_norm > 0.0) {
    const double bound = norm + 1e-6, ratio = R.D.max_grad_norm / bound, scale = ratio < 1.0 ? ratio : 1.0;
    for (size_t e = lane; e < P.std; e += NPD_TREE) O.grad[e] = (float)((double)O.grad[e] * scale);
  }
  __syncthreads();
  const double n = SHARDS ? R.n : (double)R.D.count;
  if (lane == 0) O.stats[0] = sums[NPD_PPO_POLICY_LOSS] / n;
  else if (lane == 1) O.stats[1] = sums[NPD_PPO_VALUE_LOSS] / n;
  else if (lane == 2) {
    double sum = 0.0;
    for (int a = 0; a < P.n_axes; a++) { const double t = (double)P.theta[P.log_std + a] + 0.5; sum = sum + (t + 0.9189385332046727); }
    O.stats[2] = sum;
  } else if (lane == 3) O.stats[3] = sums[NPD_PPO_KL] / n;
  else if (lane == 4) O.stats[4] = sums[NPD_PPO_CLIPPED] / n;
  else if (lane == 5) O.stats[5] = sums[NPD_PPO_SKIPPED];
  else if (lane == 6) O.stats[6] = norm;
  else if (lane == 7) O.stats[7] = n;
  else if (lane == 8) O.more[0] = sums[NPD_PPO_VF_CLIPPED] / n;
  else if (lane == 9) {      /* explained_variance from the four pinned sums over the rows that were not skipped */
    const double m = n - sums[NPD_PPO_SKIPPED];
    double ev = (double)__builtin_nanf("");
    if (m >= 1.0) {
      const double mr = sums[NPD_PPO_RET] / m, md = sums[NPD_PPO_DIFF] / m, er = sums[NPD_PPO_RET2] / m, ed = sums[NPD_PPO_DIFF2] / m;
      const double mr2 = mr * mr, md2 = md * md, vr = er - mr2, vd = ed - md2;
      if (vr > 0.0) { const double q = vd / vr; ev = 1.0 - q; }
    }
    O.more[1] = ev;
  } else if (lane == 10) {      /* the gate: one lane, ordinary stores */
    double applied = 1.0, stopped = 0.0;
    if (R.M.kl_limit > 0.0) {
      const double kl = sums[NPD_PPO_KL] / n;
      const bool stop = O.gate[NPD_PPO_GATE_STOPPED] != 0u || kl > R.M.kl_limit;
      O.gate[NPD_PPO_GATE_STOPPED] = stop ? 1u : 0u;
      if (!stop) O.gate[NPD_PPO_GATE_APPLIED] = O.gate[NPD_PPO_GATE_APPLIED] + 1u;
      applied = stop ? 0.0 : 1.0; stopped = stop ? 1.0 : 0.0;
    }
    O.more[2] = applied; O.more[3] = stopped;
  }
}

/* Adam, a lane a parameter, std's slots apart: in double, every operation rounded on its own, each result narrowed once; log_std's lane
 * then refreshes std = (float)exp((double)log_std') */
__device__ __forceinline__ void npd_ppo_adam(const npb_policy_t &P, const npb_ppo_t &O, double step_size, double root, double b1, double c1, double b2, double c2,
                                             double eps) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= P.std) return;
  const double g = (double)O.grad[e];
  const double m_keep = b1 * (double)O.m[e], m_new = c1 * g;
  const float m = (float)(m_keep + m_new);
  const double gg = g * g, v_keep = b2 * (double)O.v[e], v_new = c2 * gg;
  const float v = (float)(v_keep + v_new);
  const double rt = sqrt((double)v), scaled = rt / root, denom = scaled + eps, dir = (double)m / denom, move = step_size * dir;
  const float t = (float)((double)P.theta[e] - move);
  O.m[e] = m; O.v[e] = v; P.theta[e] = t;
  if (e >= P.log_std) P.theta[e + P.n_axes] = (float)exp((double)t);
}
__global__ __launch_bounds__(256) void npb_ppo_adam_kernel(npb_policy_t P, npb_ppo_t O, double step_size, double root, double b1, double c1, double b2, double c2,
                                                           double eps) {
  npd_ppo_adam(P, O, step_size, root, b1, c1, b2, c2, eps);
}
/* the same behind the gate: an update that is not applied stores nothing */
__global__ __launch_bounds__(256) void npb_ppo_adam_gated_kernel(npb_policy_t P, npb_ppo_t O, double step_size, double root, double b1, double c1, double b2,
                                                                 double c2, double eps) {
  if (O.gate[NPD_PPO_GATE_STOPPED] != 0u) return;
  npd_ppo_adam(P, O, step_size, root, b1, c1, b2, c2, eps);
}

extern "C" void npb_launch_ppo_grad(const npb_policy_t *P, const npb_ppo_t *O, const npb_ppo_desc_t *D, const npb_ppo_more_t *M, double n, double *out,
                                    hipStream_t stream) {
  const npd_ppo_run_t R = npd_ppo_run(O, D, M, (int)(((int64_t)D->count + D->rows_per_chain - 1) / D->rows_per_chain), n);
  const int cap = D->max_blocks > 0 ? D->max_blocks : 2048;
  const dim3 grid((unsigned)(R.n_chains < cap ? R.n_chains : cap)), block(NPD_POLICY_LANES);
  if (npd_policy_small(P, 0)) hipLaunchKernelGGL((npb_ppo_grad_kernel<NPD_POLICY_SMALL_CELLS, NPD_POLICY_SMALL_WIDTH>), grid, block, 0, stream, *P, R);
  else hipLaunchKernelGGL((npb_ppo_grad_kernel<NPB_FEATURES_CELLS_MAX, NPB_POLICY_WIDTH_MAX>), grid, block, 0, stream, *P, R);
  npb_launch_ppo_reduce(P, O, &R, out, stream);
}
void npb_launch_ppo_reduce(const npb_policy_t *P, const npb_ppo_t *O, const npd_ppo_run_t *R, double *out, hipStream_t stream) {
  if (out) {
    const size_t L = (size_t)P->log_std + NPD_PPO_ROWVALS;
    hipLaunchKernelGGL(npb_ppo_shard_reduce_kernel, dim3((unsigned)((L + NPD_TREE - 1) / NPD_TREE)), dim3(NPD_TREE), 0, stream, *P, *R, out);
    return;
  }
  hipLaunchKernelGGL(npb_ppo_reduce_kernel, dim3((P->theta_count + NPD_TREE - 1) / NPD_TREE), dim3(NPD_TREE), 0, stream, *P, *R, *O);
  hipLaunchKernelGGL(npb_ppo_finish_kernel<false>, dim3(1), dim3(NPD_TREE), 0, stream, *P, *R, *O);
}
extern "C" void npb_launch_ppo_combine(const npb_policy_t *P, const npb_ppo_t *O, const npb_ppo_shards_t *S, hipStream_t stream) {
  npd_ppo_run_t R = {};
  R.D.max_grad_norm = S->max_grad_norm; R.M.kl_limit = S->kl_limit;
  R.n = (double)S->count_total; R.ent_coef = S->ent_coef;
  R.shards = S->sums; R.shard_len = (size_t)P->log_std + NPD_PPO_ROWVALS; R.n_shards = S->n_shards;
  hipLaunchKernelGGL(npb_ppo_combine_kernel, dim3((P->theta_count + NPD_TREE - 1) / NPD_TREE), dim3(NPD_TREE), 0, stream, *P, R, *O);
  hipLaunchKernelGGL(npb_ppo_finish_kernel<true>, dim3(1), dim3(NPD_TREE), 0, stream, *P, R, *O);
}
extern "C" void npb_launch_ppo_adam(const npb_policy_t *P, const npb_ppo_t *O, double lr, double b1, double b2, double eps, int gated, hipStream_t stream) {
  /* (formed here and not by the caller: this file's flags keep the host's division IEEE too) */
  const double step = (double)O->step, step_size = lr / (1.0 - pow(b1, step)), root = sqrt(1.0 - pow(b2, step));
  const dim3 grid((P->std + 255u) / 256u), block(256);
  if (gated) hipLaunchKernelGGL(npb_ppo_adam_gated_kernel, grid, block, 0, stream, *P, *O, step_size, root, b1, 1.0 - b1, b2, 1.0 - b2, eps);
  else hipLaunchKernelGGL(npb_ppo_adam_kernel, grid, block, 0, stream, *P, *O, step_size, root, b1, 1.0 - b1, b2, 1.0 - b2, eps);
}
