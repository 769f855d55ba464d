/* npb_ppo.h -- host-callable launchers of the policy's training step (npb_ppo.hip; internal to libnpb.so; include/npb.h and
 * nuclear_sim_amd/ppo.py state what they compute). */
#ifndef NPB_PPO_H
#define NPB_PPO_H
#include "npb_policy.h"
#ifdef __cplusplus
extern "C" {
#endif
#define NPD_PPO_ROWVALS 18      /* per-row doubles a chain sums: dls[a] at a (< 8), then the slots below */
enum { NPD_PPO_POLICY_LOSS = 8, NPD_PPO_KL = 9, NPD_PPO_CLIPPED = 10, NPD_PPO_SKIPPED = 11, NPD_PPO_VALUE_LOSS = 12,
       NPD_PPO_VF_CLIPPED = 13, NPD_PPO_RET = 14, NPD_PPO_RET2 = 15, NPD_PPO_DIFF = 16, NPD_PPO_DIFF2 = 17 };
/* what the policy attachment keeps for training, allocated on first use.  ONE allocation (base stats): stats [NPB_PPO_STATS] | more
 * [NPB_PPO_STATS_MORE] | the gate's two words, stopped and applied | tree [tree_count] doubles | grad | m | v, [floats] each (theta's
 * layout, theta_count up to a multiple of 4).  A second one, grown on demand (base chain_stats): every chain's row of per-row sums
 * [chains][NPD_PPO_ROWVALS] doubles | every chain's row of partials [chains][floats].  armed, step0: the host's half of the gate, between
 * npb_policy_train_begin and npb_policy_train_end */
enum { NPD_PPO_GATE_STOPPED = 0, NPD_PPO_GATE_APPLIED = 1 };
typedef struct {
  double *stats, *tree; float *grad, *m, *v; size_t floats, tree_count;
  uint64_t step;
  double *chain_stats; float *partials; size_t chains;
  double *more; uint32_t *gate;
  int armed; uint64_t step0;
  float *hseq; size_t hseq_floats;      /* the sequence kernel's h' [t][plants][H], an allocation of its own, grown on demand (npb_policy_grad_seq) */
} npb_ppo_t;
/* the gradient of one minibatch: the gradient kernel (a workgroup a chain), the ascending sum over the chains, the finish.  O holds
 * room for ceil(count / rows_per_chain) chains.  M (NULL = every option off): value-loss clipping, and with kl_limit > 0 the finish ORs
 * the gate on O->gate.  n: the seeds' divisor, (double)D->count or a shard's (double)count_total.  out == NULL: the reduce into the handle's
 * grad, stats and more.  out != NULL (npb_policy_shard_sums): one shard's sums instead, a lane an entry of out [P->log_std + NPD_PPO_ROWVALS]
 * doubles: the ascending sum over the chains, not narrowed; O's grad, stats, more and gate are not touched */
void npb_launch_ppo_grad(const npb_policy_t *P, const npb_ppo_t *O, const npb_ppo_desc_t *D, const npb_ppo_more_t *M, double n, double *out, hipStream_t stream);
/* one Adam step on P->theta from O->grad, O->step the step it is (already advanced): step_size = lr / (1 - b1^step) and root = sqrt(1 -
 * b2^step) are formed on the host, in double.  gated: the launch reads O->gate's stopped word and stores nothing when it is set */
void npb_launch_ppo_adam(const npb_policy_t *P, const npb_ppo_t *O, double lr, double b1, double b2, double eps, int gated, hipStream_t stream);
/* the combine (npb_policy_apply_shards, npb_policy_combine_shards): a lane a parameter adds S->sums' rows in ascending order onto 0.0,
 * narrows once and takes the tree's first level; then the finish over the 18 totals with n = count_total, S->kl_limit > 0 ORing the gate */
void npb_launch_ppo_combine(const npb_policy_t *P, const npb_ppo_t *O, const npb_ppo_shards_t *S, hipStream_t stream);
/* the gradient over whole sequences through the recurrent core (npb_ppo_seq.hip; npb_policy_grad_seq, npb_policy_shard_sums_seq; n and out as above): D's tensors
 * time-major [S->t][S->plants][...], D->rows_per_chain the PLANTS of a chain; O holds room for ceil(plants / rows_per_chain) chains and
 * O->hseq for t * plants * H floats.  G (NULL: whole sequences): the sequences are segments of S->t slots, S->index their ids c * n_plants + p,
 * S->first the stored states [G->chunks * n_plants][H] (npb_policy_grad_segments) */
void npb_launch_ppo_grad_seq(const npb_policy_t *P, const npd_policy_core_t *C, const npb_ppo_t *O, const npb_ppo_desc_t *D, const npb_ppo_more_t *M,
                             const npb_ppo_seq_t *S, const npb_ppo_segments_t *G, double n, double *out, hipStream_t stream);
/* the refresh of the stored states (npb_policy_segment_starts): the forward sweep over the rollout's t recorded slots from C->first under the
 * current theta; rows 1 .. t / every - 1 of starts [t / every][n_plants][H] receive the state read in front of slot c * every */
void npb_launch_segment_starts(const npb_policy_t *P, const npd_policy_core_t *C, const void *obs, int obs_f64, int t, int n_plants, int every,
                               const int32_t *episode, const uint8_t *ended, float *starts, hipStream_t stream);
#ifdef __cplusplus
}
#endif
#ifdef __HIPCC__
/* ---- what the two gradient kernels share (npb_ppo.hip: rows; npb_ppo_seq.hip: whole sequences through the recurrent core), each stated once:
 * the run's descriptor, dW and db of a layer onto the chain's partials, the back through a layer, the per-row epilogues, one net of a tile */
typedef struct {
  npb_ppo_desc_t D;
  npb_ppo_more_t M;                    /* every option off: {NULL, 0.0, 0.0} */
  int n_chains;
  float *partials; size_t floats;      /* [n_chains][floats] */
  double *chain_stats;                 /* [n_chains][NPD_PPO_ROWVALS] */
  double n;                            /* the seeds' divisor: (double)D.count, or a shard's (double)count_total */
  const double *shards; size_t shard_len; int n_shards;      /* the combine's: [n_shards][shard_len], shard_len = P.log_std + NPD_PPO_ROWVALS */
  double ent_coef;                     /* the combine's (a plain call's is D.ent_coef) */
} npd_ppo_run_t;

__device__ __forceinline__ double npd_ppo_load(const void *x, int f64, size_t i) { return f64 ? ((const double *)x)[i] : (double)((const float *)x)[i]; }

/* a layer's dW and db of this tile onto the chain's partials: delta[j][row], hin[k][row] (row stride NPD_POLICY_STRIDE both).  Lane l gives
 * A[j = l & 31][row = l >> 5] and B[row = l >> 5][k = l & 31] and holds D[j = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)][k = l & 31].  A block's
 * cells beyond the layer's out or in read whatever LDS holds there and are neither loaded nor stored: D[j][k] depends on row j of A and
 * column k of B alone */
__device__ __forceinline__ void npd_ppo_dw(const npd_policy_layer_t &L, float *__restrict__ prow, bool first, const float *delta, const float *hin, int tid) {
  const int wave = tid >> 6, lane = tid & 63, col = lane & 31, half = lane >> 5;
  const int kb = (L.in + 31) >> 5, blocks = (L.out_pad >> 5) * kb;
  for (int b = wave; b < blocks; b += NPD_POLICY_WAVES) {
    const int j0 = 32 * (b / kb), k0 = 32 * (b % kb), k = k0 + col;
    npd_f32x16 acc;
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int j = j0 + (reg & 3) + 8 * (reg >> 2) + 4 * half;
      acc[reg] = !first && j < L.out && k < L.in ? prow[L.w + (size_t)j * L.in + k] : 0.0f;
    }
    const float *a = delta + (j0 + col) * NPD_POLICY_STRIDE + half;
    const float *h = hin + k * NPD_POLICY_STRIDE + half;
#pragma unroll
    for (int s = 0; s < NPD_POLICY_TILE / 2; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * s], h[2 * s], acc, 0, 0, 0);
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int j = j0 + (reg & 3) + 8 * (reg >> 2) + 4 * half;
      if (j < L.out && k < L.in) prow[L.w + (size_t)j * L.in + k] = acc[reg];
    }
  }
  if (tid < L.out) {
    float acc = first ? 0.0f : prow[L.b + tid];
    const float *d = delta + tid * NPD_POLICY_STRIDE;
#pragma unroll
    for (int r = 0; r < NPD_POLICY_TILE; r++) acc = acc + d[r];      /* fmaf(delta, 1.0f, acc) */
    prow[L.b + tid] = acc;
  }
}

/* the chain of one block of 32 inputs k through a layer: acc[row][k] = fmaf(delta[row][j], W[j][k], acc) for j ascending, two j a call, j up to
 * the next multiple of 4 of the layer's width (the producer of delta wrote +0.0 there; W reads as +0.0 there).  Lane l gives A[row = l & 31]
 * [j = l >> 5] and B[j = l >> 5][k = l & 31] = theta's W[j][k] and holds D[row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)][k = l & 31].  The
 * accumulator comes in and goes out: a chain over several layers' rows (the cell's W_hh: three row blocks) carries it from one to the next.
 * An accumulator that started at +0.0 is never -0.0, so the calls of a width's extension change no bit of it */
__device__ __forceinline__ npd_f32x16 npd_ppo_chain(const npd_policy_layer_t &L, const float *__restrict__ theta, const float *delta, npd_f32x16 acc, int k, int col,
                                                    int half) {
  const int pairs = ((L.out + 3) & ~3) >> 1;
  const float *a = delta + half * NPD_POLICY_STRIDE + col;
  for (int s = 0; s < pairs; s++) {
    const int j = 2 * s + half;
    const float w = j < L.out && k < L.in ? theta[L.w + (size_t)j * L.in + k] : 0.0f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * s * NPD_POLICY_STRIDE], w, acc, 0, 0, 0);
  }
  return acc;
}

/* delta'[k][row] of the layer below: back[row][k] = npd_ppo_chain from +0.0, then the derivative of the activation that made h[k][row].
 * k up to the next multiple of 4 of the layer's in is written +0.0: the k extension of the back below */
__device__ __forceinline__ void npd_ppo_back(const npd_policy_layer_t &L, const float *__restrict__ theta, const float *delta, float *out, const float *h,
                                             int activation, int tid) {
  const int wave = tid >> 6, lane = tid & 63, col = lane & 31, half = lane >> 5;
  for (int k0 = 32 * wave; k0 < L.in; k0 += 32 * NPD_POLICY_WAVES) {
    const int k = k0 + col;
    npd_f32x16 acc;
#pragma unroll
    for (int reg = 0; reg < 16; reg++) acc[reg] = 0.0f;
    acc = npd_ppo_chain(L, theta, delta, acc, k, col, half);
    if (k < L.in_pad) {
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * half;
        const float hv = h[k * NPD_POLICY_STRIDE + row];
        float y = acc[reg];
        if (activation == NPB_POLICY_RELU) y = hv > 0.0f ? y : 0.0f;
        else { const float sq = hv * hv; const float slope = 1.0f - sq; y = y * slope; }
        out[k * NPD_POLICY_STRIDE + row] = k < L.in ? y : 0.0f;
      }
    }
  }
}

/* the back with no derivative behind it, added onto what out holds: out[k][row] = out[k][row] + back[row][k], the chain from +0.0 over the rows
 * of N layers of one `in`, in order (N = 1: a net's first layer, whose input h' is no activation; N = 3: the cell's W_hh, delta_h's three
 * blocks).  zero != NULL: out[k][row] = +0.0 where zero[row] (the carry of a plant that restarted).  k < in only */
template <int N>
__device__ __forceinline__ void npd_ppo_back_onto(const npd_policy_layer_t *const (&L)[N], const float *const (&delta)[N], const float *__restrict__ theta, float *out,
                                                  const int *zero, int tid) {
  const int wave = tid >> 6, lane = tid & 63, col = lane & 31, half = lane >> 5, in = L[0]->in;
  for (int k0 = 32 * wave; k0 < in; k0 += 32 * NPD_POLICY_WAVES) {
    const int k = k0 + col;
    npd_f32x16 acc;
#pragma unroll
    for (int reg = 0; reg < 16; reg++) acc[reg] = 0.0f;
#pragma unroll
    for (int i = 0; i < N; i++) acc = npd_ppo_chain(*L[i], theta, delta[i], acc, k, col, half);
    if (k < in) {
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * half;
        const float sum = out[k * NPD_POLICY_STRIDE + row] + acc[reg];
        out[k * NPD_POLICY_STRIDE + row] = zero && zero[row] ? 0.0f : sum;
      }
    }
  }
}

/* the per-row epilogues, a lane a row of the tile (tid < 32; every lane may call), what both gradient kernels (npb_ppo.hip, npb_ppo_seq.hip) run
 * behind a net's forward pass.  p: the row's index into the minibatch's tensors; live: the row exists; skipped: it is a skipped row; n: the
 * seeds' divisor.  head[a][row]: the net's outputs; da[a][row]: the head's delta, written here (+0.0 up to the next multiple of 4); rowv
 * [q][row]: the per-row doubles, zeroed by the caller.  The actor's: the seeds dmean, dls, the policy loss' terms, logp_new and ratio out */
__device__ __forceinline__ void npd_ppo_seeds_actor(const npb_policy_t &P, const npb_ppo_desc_t &D, double n, const float *head, float *da, double *rowv, int tid,
                                                    bool live, bool skipped, size_t p) {
  const int A = P.n_axes;
  const double qnan = (double)__builtin_nanf("");
  const int A4 = (A + 3) & ~3;
  if (tid >= NPD_POLICY_TILE) return;
  for (int a = 0; a < A4; a++) da[a * NPD_POLICY_STRIDE + tid] = 0.0f;
  if (!live) return;
  if (skipped) {
    rowv[NPD_PPO_SKIPPED * NPD_POLICY_TILE + tid] = 1.0;
    if (D.logp_new) D.logp_new[p] = (float)qnan;
    if (D.ratio) D.ratio[p] = qnan;
    return;
  }
  double d[NPB_CONTROLS_AXES_MAX];
  double lp = -((double)A * 0.9189385332046727);
  for (int a = 0; a < A; a++) {
    const double diff = npd_ppo_load(D.act, D.act_type, p * A + a) - (double)head[a * NPD_POLICY_STRIDE + tid];
    d[a] = diff / (double)P.theta[P.std + a];
    const double sq = d[a] * d[a], hf = 0.5 * sq;
    lp = (lp - hf) - (double)P.theta[P.log_std + a];
  }
  const double lr = lp - (double)D.logp_old[p], r = exp(lr), adv = npd_ppo_load(D.adv, D.adv_type, p);
  const double lo = 1.0 - D.clip, hi = 1.0 + D.clip;
  const bool clipped = (adv > 0.0 && r > hi) || (adv < 0.0 && r < lo);
  const double ar = adv * r, c = clipped ? 0.0 : -ar;
  for (int a = 0; a < A; a++) {
    const double cd = c * d[a], q = cd / (double)P.theta[P.std + a], seed = q / n;
    da[a * NPD_POLICY_STRIDE + tid] = (float)seed;
    const double sq = d[a] * d[a], less = sq - 1.0, t = c * less;
    rowv[a * NPD_POLICY_TILE + tid] = t / n;
  }
  const double rc = r < lo ? lo : (r > hi ? hi : r), second = rc * adv;
  rowv[NPD_PPO_POLICY_LOSS * NPD_POLICY_TILE + tid] = -(second < ar ? second : ar);
  const double rm = r - 1.0;
  rowv[NPD_PPO_KL * NPD_POLICY_TILE + tid] = rm - lr;
  rowv[NPD_PPO_CLIPPED * NPD_POLICY_TILE + tid] = clipped ? 1.0 : 0.0;
  if (D.logp_new) D.logp_new[p] = (float)lp;
  if (D.ratio) D.ratio[p] = r;
}
/* the critic's: the value's seed and loss (with clip_vf > 0 the clipped branch), the four terms of explained_variance, value_new out */
__device__ __forceinline__ void npd_ppo_seeds_critic(const npb_policy_t &P, const npb_ppo_desc_t &D, const npb_ppo_more_t &M, double n, const float *head, float *da,
                                                     double *rowv, int tid, bool live, bool skipped, size_t p) {
  const double qnan = (double)__builtin_nanf("");
  if (tid >= NPD_POLICY_TILE) return;
  for (int a = 0; a < 4; a++) da[a * NPD_POLICY_STRIDE + tid] = 0.0f;
  if (!live) return;
  const float v = head[tid];
  if (D.value_new) D.value_new[p] = skipped ? (float)qnan : v;
  if (skipped) return;
  const double ret = npd_ppo_load(D.ret, D.adv_type, p), diff = (double)v - ret, sq = diff * diff;
  double seed = diff, lsq = sq;
  if (M.clip_vf > 0.0) {      /* the max form: the larger of the two squares, and its own derivative */
    const double c = M.clip_vf, vo = (double)M.value_old[p], dvo = (double)v - vo;
    const double dc = dvo < -c ? -c : (dvo > c ? c : dvo), vc = vo + dc, diffc = vc - ret, sqc = diffc * diffc;
    const bool use = sqc > sq, out = dvo < -c || dvo > c;
    seed = use ? (out ? 0.0 : diffc) : diff;
    lsq = use ? sqc : sq;
    rowv[NPD_PPO_VF_CLIPPED * NPD_POLICY_TILE + tid] = out ? 1.0 : 0.0;
  }
  const double scaled = D.vf_coef * seed;
  da[tid] = (float)(scaled / n);
  rowv[NPD_PPO_VALUE_LOSS * NPD_POLICY_TILE + tid] = 0.5 * lsq;
  rowv[NPD_PPO_RET * NPD_POLICY_TILE + tid] = ret;
  rowv[NPD_PPO_RET2 * NPD_POLICY_TILE + tid] = ret * ret;
  rowv[NPD_PPO_DIFF * NPD_POLICY_TILE + tid] = diff;
  rowv[NPD_PPO_DIFF2 * NPD_POLICY_TILE + tid] = sq;
}

/* one net of the tile: forward with every hidden activation kept (hid[l]), then `seeds` (a lane a row; it writes the head's delta into d0
 * and ends with the barrier that publishes it), then backward onto the chain's partials.  dh != NULL (the sequence kernel, whose nets read the
 * cell's h'): the first layer's back, no derivative, is added onto dh[k][row] */
template <int H_MAX, class Seeds>
__device__ __forceinline__ void npd_ppo_net(const npd_policy_net_t &N, const npb_policy_t &P, const float *xs, float (*hid)[H_MAX * NPD_POLICY_STRIDE], float *head,
                                            float *d0, float *d1, float *prow, bool first, int tid, float *dh, Seeds seeds) {
  const int wave = tid >> 6, lane = tid & 63, last = N.n_layers - 1;
  for (int l = 0; l <= last; l++) {
    npd_policy_layer(N.layer[l], P.theta, P.padded, l ? hid[l - 1] : xs, l == last ? head : hid[l], l == last ? -1 : P.D.activation, wave, lane);
    __syncthreads();
  }
  seeds();
  __syncthreads();
  for (int l = last; l >= 0; l--) {
    const npd_policy_layer_t &L = N.layer[l];
    npd_ppo_dw(L, prow, first, d0, l ? hid[l - 1] : xs, tid);
    if (l) npd_ppo_back(L, P.theta, d0, d1, hid[l - 1], P.D.activation, tid);
    else if (dh) { const npd_policy_layer_t *const layers[1] = {&L}; const float *const deltas[1] = {d0}; npd_ppo_back_onto<1>(layers, deltas, P.theta, dh, nullptr, tid); }
    __syncthreads();
    float *t = d0; d0 = d1; d1 = t;
  }
}
/* the run of a gradient call: the chains' workspace of O, the seeds' divisor n; n_chains: ceil(count / rows_per_chain), or a sequence call's chains */
static inline npd_ppo_run_t npd_ppo_run(const npb_ppo_t *O, const npb_ppo_desc_t *D, const npb_ppo_more_t *M, int n_chains, double n) {
  npd_ppo_run_t R = {};
  R.D = *D;
  if (M) R.M = *M;
  R.n_chains = n_chains;
  R.partials = O->partials; R.floats = O->floats; R.chain_stats = O->chain_stats;
  R.n = n;
  return R;
}
/* behind a gradient kernel that filled R's chains (npb_ppo.hip).  out == NULL: the ascending sums over the chains, the norm, the scale, the
 * statistics, the gate, into O; out != NULL: a shard's vector of the sums, and O is left alone */
void npb_launch_ppo_reduce(const npb_policy_t *P, const npb_ppo_t *O, const npd_ppo_run_t *R, double *out, hipStream_t stream);
#endif
#endif
