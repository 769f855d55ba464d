/* npb_ppo_seq.hip -- training the recurrent policy through time on the device (npb_policy_grad_seq, npb_policy_shard_sums_seq, include/npb.h):
 * PPO's loss over a minibatch of whole sequences and its gradient through both MLPs, through the GRU cell and through time.
 * nuclear_sim_amd/recurrent.py (gradient, shard_sums) states it in numpy; this file produces its bits for hard gates and relu nets fed the
 * device's own ratio (the float tanh and the double exp are the statement's licensed differences).  Built with npb_ppo.hip's flags (Makefile):
 * no contraction, IEEE division and square root.  The reduce, finish, Adam, shard and combine kernels are npb_ppo.hip's: they work on theta's
 * flat layout, and the core's parameters are its front.
 *
 * THE GRADIENT KERNEL: one workgroup of 256 lanes (four waves) runs one CHAIN of rows_per_chain PLANTS with all their t slots, tile of 32
 * plants after tile; a launch's workgroups stride over the chains.  The geometry and the LDS layout are the policy's: every buffer
 * [k][plant], row stride 33.  The minibatch is time-major, [t][plants][...]; a plant's restart words and its state in front of slot 0 are
 * read from the rollout's own tensors through the minibatch's index: episode and ended [T][n_plants], first [n_plants][H].  An index outside
 * 0 .. n_plants - 1 makes every cell of that plant a skipped, poisoned cell, and nothing is read through it.  Per tile, two sweeps:
 *   FORWARD, s ascending: the step kernel's cell, the ONE statement of it both call (npb_policy.h's npd_core_cell: gate by gate),
 *   h carried in LDS, +0.0 where the plant restarted in front of s (an episode change, or the cut bit of ended[s - 1]) and behind a poisoned
 *   cell; h'_s goes to the handle's workspace [t][plants][H] (or the caller's hidden).  Only h' is stored: the backward sweep recomputes the
 *   gates, which gives the same bits and keeps the workspace at t * plants * H floats.  It keeps a buffer assignment of its own (it needs gi_n
 *   and gh_n apart, and the flags), but S, T, the clamp test and the slopes d * S' and d * T' are npb_policy.h's (npd_core_sigma, npd_core_tau,
 *   npd_core_sigma_clamps, npd_core_sigma_slope, npd_core_tau_slope: recurrent.py's names), so a gate is changed in one place.
 *   BACKWARD, s descending, the carry dh in LDS (+0.0 behind the last slot):
 *     the nets, one after the other (npb_ppo.h's npd_ppo_net, the row-wise kernel's own): h'_s from the workspace, forward with the
 *     activations kept, the per-row epilogue (npd_ppo_seeds_actor, npd_ppo_seeds_critic), dW / db onto the chain's partials, back; the first
 *     layer's back has no derivative behind it and is added onto dh: dh' = (carry + back_actor) + back_critic.
 *     the cell: h_s (first, or h'_(s-1) from the workspace, the restart applied) and x_s (a poisoned cell's +0.0) into LDS; the gates again,
 *     r into b2, z into b3, n into b4, gh_n into b5, and for hard gates the three clamped-branch flags of a cell as a small number in b6;
 *     then a lane a cell, in place: dar over r, daz over z, dan over n, dghn over gh_n, direct = dh' * z over dh (all +0.0 on a poisoned
 *     cell); dW / db of the six gate layers onto the partials (delta_i = [dar | daz | dan] with x, delta_h = [dar | daz | dghn] with h); and
 *     the carry: dh = direct + back(delta_h, W_hh), ONE chain over W_hh's 3H rows, the accumulator carried through the three blocks as the
 *     matrix core's C operand (npd_ppo_back_onto<3>), +0.0 where the plant restarted in front of s.
 *   The per-row doubles of a slot are added in plant order onto the chain's running sums, a lane a quantity.
 * A chain's rows therefore enter every sum in the statement's order: tiles ascending, within a tile s descending, within a slot the plants
 * ascending.  No atomics, nothing depends on the launch order, no scratch.
 * LDS, from the declarations below: xs (K*C x 33 floats), seven H-wide buffers (H_MAX x 33 floats each; H_MAX covers the core and both nets'
 * widths), the head's 1056 B, the per-row doubles' 4608 B, four words a plant: the small build (npd_policy_small with the core's width)
 * 8448 + 7 x 8448 + 6176 = 73 760 B, the large one 33 792 + 7 x 16 896 + 6176 = 158 240 B of gfx950's 160 KiB (one workgroup a CU), and 128 B
 * more for word0 (below): 73 888 / 158 368 B as the compiler reports them.  Its other figures (-Rpass-analysis=kernel-resource-usage added to the Makefile's
 * own line for this file: -O3 -ffp-contract=off -fno-fast-math; the scalar spills move with the flags and with every
 * textual move of the code, every other figure stays), small / large build: 256 / 256 VGPRs, 40 / 40 AGPRs, no scratch, no VGPR spills, and 466 / 464 of the descriptors' scalars spilled from SGPRs into
 * VGPR lanes (the row-wise kernel: 133 / 129) -- no memory traffic, but a workgroup is alone on its CU in the small build too.  No atomics.
 * No shape is refused: both builds fit.  Measured on an MI355X
 * (tools/recurrent_train_cost.py): one update of t = 128 through a cell of 64 and (64, 64) nets, 19.5 ms at 2 048 plants, 20.4 ms at 4 096, 29.8 ms at 8 192.  The
 * nets' phase and the cell's phase alias the seven buffers: b0 the carry; b1 h' then h; b2 .. b4 the nets' hidden activations then r, z, n;
 * b5, b6 the nets' two delta buffers then gh_n and the flags.
 *
 * TRUNCATED SEGMENTS (npb_policy_grad_segments and its companions; Q.chunks > 0) run the same kernel: a sequence is a segment of S.t = every
 * slots, its index a segment id g = c * n_plants + p.  The only differences are in the tile's decode (lanes 0 .. 31, once a tile): g outside
 * 0 .. chunks * n_plants - 1 poisons the sequence and nothing is read through it; src[] keeps g, the row of S.first (the stored states
 * [chunks * n_plants][H]); word0[] keeps (c * every) * n_plants + p, the cell of local slot 0 in episode and ended, so that local slot s > 0
 * reads its restart words at rollout rows c * every + s and c * every + s - 1.  No word in front of local slot 0 is read (that restart is in
 * the stored state), and the carry out of local slot 0 goes nowhere: that is the truncation.  Whole sequences have word0 = src = the plant.
 * THE REFRESH (npb_policy_segment_starts; npb_segment_starts_kernel) is the forward sweep alone -- npd_seq_forward, the one piece of code
 * both kernels call -- over the rollout's own tensors, one workgroup per tile of 32 plants, serial in t; the state in front of slot c * every
 * goes into row c of the stored states for c >= 1.  Five H-wide buffers and xs: 50 944 / 118 528 B of LDS, 105 / 78 VGPRs, 16 AGPRs, no
 * scratch, no VGPR spills (38 / 38 scalars into VGPR lanes), no atomics. */
#include <hip/hip_runtime.h>
#include <math.h>
#include "npb_ppo.h"

#define NPD_SEQ_CUT 4      /* NPB_ROLLOUT_CUT */

/* what the sequence kernel takes beside npd_ppo_run_t: the caller's descriptor and the workspace of h' */
typedef struct {
  npb_ppo_seq_t S;
  float *hseq;      /* [t][plants][H] */
  int chunks;       /* 0: whole sequences, index a plant; > 0: segments of S.t slots, index a segment id c * n_plants + p with c < chunks */
} npd_ppo_seq_run_t;
/* what the refresh of the stored states takes (npb_policy_segment_starts): the rollout's own tensors, no minibatch */
typedef struct {
  const void *obs; int obs_f64;      /* [t][n_plants][K * C] */
  int t, n_plants, every;
  const int32_t *episode; const uint8_t *ended;      /* [t][n_plants] */
  const float *first;      /* [n_plants][H] */
  float *starts;           /* [t / every][n_plants][H]: rows 1 .. are written */
} npd_seq_starts_t;

/* THE FORWARD SWEEP of one tile, s ascending, what the gradient kernel and the refresh of the stored states share: h in b1, the step kernel's
 * cell (npb_policy.h's npd_core_cell: gi into b2, gh into b3, r into b4, z into b5).  obs: slot s of the tile is in_tile rows of KC cells at cell (s * rows +
 * base); words(s), lanes 0 .. 31: fresh and bad of the slot; first_of(row): the state in front of slot 0; front(s): h_s stands in b1, the
 * restart applied, and is only read until the cell has run; behind(s): h'_s stands in b1.  xs is zero beyond KC on entry */
template <class Words, class First, class Front, class Behind>
__device__ __forceinline__ void npd_seq_forward(const npb_policy_t &P, const npd_policy_core_t &C, const void *obs, int obs_f64, size_t rows, size_t base, int in_tile,
                                                int T, float *xs, float *b1, float *b2, float *b3, float *b4, float *b5, int *bad, const int *fresh, int tid,
                                                Words words, First first_of, Front front, Behind behind) {
  const int KC = P.cells, H = C.H, H_pad = (H + 3) & ~3;
  for (int s = 0; s < T; s++) {
    if (tid < NPD_POLICY_TILE) words(s);
    __syncthreads();
    const size_t cell0 = (size_t)s * rows + base;
    if (obs_f64) npd_policy_tile_load((const double *)obs + cell0 * KC, in_tile, KC, xs, bad, tid);
    else npd_policy_tile_load((const float *)obs + cell0 * KC, in_tile, KC, xs, bad, tid);
    if (s == 0) npd_seq_fill(b1, H, H_pad, tid, first_of);
    else
      for (int i = tid; i < H_pad * NPD_POLICY_TILE; i += NPD_POLICY_LANES)
        if (fresh[i & (NPD_POLICY_TILE - 1)]) b1[(i / NPD_POLICY_TILE) * NPD_POLICY_STRIDE + (i & (NPD_POLICY_TILE - 1))] = 0.0f;
    __syncthreads();
    front(s);
    npd_core_cell(P, C, xs, b1, b2, b3, b4, b5, bad, tid);
    behind(s);
  }
}

template <int KC_MAX, int H_MAX>
__global__ __launch_bounds__(NPD_POLICY_LANES) void npb_ppo_seq_kernel(npb_policy_t P, npd_policy_core_t C, npd_ppo_run_t R, npd_ppo_seq_run_t Q) {
  __shared__ float xs[KC_MAX * NPD_POLICY_STRIDE];
  __shared__ float buf[7][H_MAX * NPD_POLICY_STRIDE];
  __shared__ float head[NPB_CONTROLS_AXES_MAX * NPD_POLICY_STRIDE];
  __shared__ double rowv[NPD_PPO_ROWVALS * NPD_POLICY_TILE];
  __shared__ int bad[NPD_POLICY_TILE], fresh[NPD_POLICY_TILE], skip[NPD_POLICY_TILE], src[NPD_POLICY_TILE], word0[NPD_POLICY_TILE];
  float *const b0 = buf[0], *const b1 = buf[1], *const b2 = buf[2], *const b3 = buf[3], *const b4 = buf[4], *const b5 = buf[5], *const b6 = buf[6];
  const npb_ppo_desc_t &D = R.D;
  const npb_ppo_seq_t &S = Q.S;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, A = P.n_axes, KC = P.cells, KC_pad = (KC + 3) & ~3, H = C.H, H_pad = (H + 3) & ~3;
  const int T = S.t;
  const size_t plants = (size_t)S.plants, ppc = (size_t)D.rows_per_chain, n_plants = (size_t)S.n_plants;
  const double n = R.n;
  for (size_t chain = blockIdx.x; chain < (size_t)R.n_chains; chain += gridDim.x) {
    float *prow = R.partials + chain * R.floats;
    double running = 0.0;      /* lane q < NPD_PPO_ROWVALS: the chain's sum of per-row double q */
    for (size_t base = chain * ppc; base < (chain + 1) * ppc && base < plants; base += NPD_POLICY_TILE) {
      const int in_tile = npd_policy_in_tile(plants, base);
      __syncthreads();      /* (the tile before is done with every buffer) */
      /* the tile's sequences of the rollout: src the row of `first` (a plant, or a segment id c * n_plants + p), -1 beyond the tile and for
       * an index outside the rollout's; word0 the restart word of local slot 0 in episode and ended: column p of row 0, or of row c * t */
      if (tid < NPD_POLICY_TILE) {
        int64_t from = -1, at = 0;
        if (tid < in_tile) {
          from = S.index ? (int64_t)S.index[base + tid] : (int64_t)(base + tid);
          if (from < 0 || from >= (int64_t)(Q.chunks ? Q.chunks : 1) * (int64_t)n_plants) from = -1;
          else if (Q.chunks) { const int64_t c = from / (int64_t)n_plants; at = c * T * (int64_t)n_plants + (from - c * (int64_t)n_plants); }
          else at = from;
        }
        src[tid] = (int)from; word0[tid] = (int)at;
      }
      npd_policy_tile_zero(xs, 0, KC_pad, tid);      /* (once a tile: every slot's load overwrites the same cells) */
      __syncthreads();
      /* the restart in front of slot s and the poison a plant starts a slot with, lanes 0 .. 31 */
      auto words = [&](int s) {
        const int from = src[tid];
        int restart = 0;
        if (from >= 0 && s > 0) {
          const size_t now = (size_t)s * n_plants + (size_t)word0[tid], before = now - n_plants;
          restart = S.episode[now] != S.episode[before] || (S.ended[before] & NPD_SEQ_CUT) != 0;
        }
        fresh[tid] = restart;
        bad[tid] = from < 0;
      };
      auto first_of = [&](int row) -> const float * { return src[row] >= 0 ? S.first + (size_t)src[row] * H : nullptr; };
      /* ---- the forward sweep (npd_seq_forward): h'_s into the workspace */
      npd_seq_forward(P, C, D.obs, D.obs_type, plants, base, in_tile, T, xs, b1, b2, b3, b4, b5, bad, fresh, tid, words, first_of, [](int) {},
                      [&](int s) { npd_core_store(Q.hseq + ((size_t)s * plants + base) * H, b1, in_tile, H, tid); });
      /* ---- the backward sweep */
      __syncthreads();
      npd_policy_tile_zero(b0, 0, H_pad, tid);
      for (int s = T - 1; s >= 0; s--) {
        const bool first = base == chain * ppc && s == T - 1;
        const size_t cell0 = (size_t)s * plants + base, p = cell0 + tid;
        __syncthreads();      /* (the slot behind is done with every buffer, and the forward sweep's h' are this workgroup's to read) */
        for (int i = tid; i < NPD_PPO_ROWVALS * NPD_POLICY_TILE; i += NPD_POLICY_LANES) rowv[i] = 0.0;
        if (tid < NPD_POLICY_TILE) {
          words(s);
          int b = 0;
          if (tid < in_tile) {
            const double old = (double)D.logp_old[p], adv = npd_ppo_load(D.adv, D.adv_type, p), ret = npd_ppo_load(D.ret, D.adv_type, p);
            b = !(old - old == 0.0) || !(adv - adv == 0.0) || !(ret - ret == 0.0);
            if (R.M.clip_vf > 0.0) { const float vo = R.M.value_old[p]; b |= !(vo - vo == 0.0f); }
            for (int a = 0; a < A; a++) { const double x = npd_ppo_load(D.act, D.act_type, p * A + a); b |= !(x - x == 0.0); }
          }
          skip[tid] = b;
        }
        __syncthreads();
        if (D.obs_type) npd_policy_tile_load((const double *)D.obs + cell0 * KC, in_tile, KC, xs, bad, tid);
        else npd_policy_tile_load((const float *)D.obs + cell0 * KC, in_tile, KC, xs, bad, tid);
        const float *hp = Q.hseq + cell0 * H;
        npd_seq_fill(b1, H, H_pad, tid, [&](int row) -> const float * { return row < in_tile ? hp + (size_t)row * H : nullptr; });
        __syncthreads();
        for (int i = tid; i < KC * NPD_POLICY_TILE; i += NPD_POLICY_LANES)
          if (bad[i & 31]) xs[(i >> 5) * NPD_POLICY_STRIDE + (i & 31)] = 0.0f;      /* (read by the cell's phase, behind the nets' barriers) */
        const bool live = tid < in_tile, skipped = tid < NPD_POLICY_TILE && (bad[tid & 31] != 0 || skip[tid & 31] != 0);
        /* the nets over h'_s: hidden activations b2 .. b4, deltas b5 and b6, the first layers' backs onto the carry */
        npd_ppo_net<H_MAX>(P.actor, P, b1, buf + 2, head, b5, b6, prow, first, tid, b0, [&]() { npd_ppo_seeds_actor(P, D, n, head, b5, rowv, tid, live, skipped, p); });
        npd_ppo_net<H_MAX>(P.critic, P, b1, buf + 2, head, b5, b6, prow, first, tid, b0, [&]() { npd_ppo_seeds_critic(P, D, R.M, n, head, b5, rowv, tid, live, skipped, p); });
        if (tid < NPD_PPO_ROWVALS)
          for (int r = 0; r < NPD_POLICY_TILE; r++) running = running + rowv[tid * NPD_POLICY_TILE + r];
        /* the cell: h_s into b1, the gates again */
        if (s == 0) npd_seq_fill(b1, H, H_pad, tid, first_of);
        else {
          const float *hb = Q.hseq + (cell0 - plants) * H;
          npd_seq_fill(b1, H, H_pad, tid, [&](int row) -> const float * { return row < in_tile && !fresh[row] ? hb + (size_t)row * H : nullptr; });
        }
        __syncthreads();
        npd_policy_layer(C.gate[0], P.theta, P.padded, xs, b2, -1, wave, lane);
        npd_policy_layer(C.gate[3], P.theta, P.padded, b1, b6, -1, (wave + 2) & (NPD_POLICY_WAVES - 1), lane);
        __syncthreads();
        for (int i = tid; i < H_pad * NPD_POLICY_TILE; i += NPD_POLICY_LANES) {
          const int o = (i / NPD_POLICY_TILE) * NPD_POLICY_STRIDE + (i & (NPD_POLICY_TILE - 1));
          const float a = b2[o] + b6[o];
          b2[o] = npd_core_sigma(a, C.gates);
          b6[o] = npd_core_sigma_clamps(a, C.gates) ? 1.0f : 0.0f;
        }
        __syncthreads();
        npd_policy_layer(C.gate[1], P.theta, P.padded, xs, b3, -1, wave, lane);
        npd_policy_layer(C.gate[4], P.theta, P.padded, b1, b4, -1, (wave + 2) & (NPD_POLICY_WAVES - 1), lane);
        __syncthreads();
        for (int i = tid; i < H_pad * NPD_POLICY_TILE; i += NPD_POLICY_LANES) {
          const int o = (i / NPD_POLICY_TILE) * NPD_POLICY_STRIDE + (i & (NPD_POLICY_TILE - 1));
          const float a = b3[o] + b4[o];
          b3[o] = npd_core_sigma(a, C.gates);
          if (npd_core_sigma_clamps(a, C.gates)) b6[o] = b6[o] + 2.0f;
        }
        __syncthreads();
        npd_policy_layer(C.gate[2], P.theta, P.padded, xs, b4, -1, wave, lane);
        npd_policy_layer(C.gate[5], P.theta, P.padded, b1, b5, -1, (wave + 2) & (NPD_POLICY_WAVES - 1), lane);
        __syncthreads();
        /* a lane a cell: the candidate, then the cell backwards, in place */
        for (int i = tid; i < H_pad * NPD_POLICY_TILE; i += NPD_POLICY_LANES) {
          const int j = i / NPD_POLICY_TILE, plant = i & (NPD_POLICY_TILE - 1), o = j * NPD_POLICY_STRIDE + plant;
          const float r = b2[o], z = b3[o], ghn = b5[o], h = b1[o], dh = b0[o];
          const int flags = (int)b6[o];
          const float gated = r * ghn;
          const float an = b4[o] + gated;
          const float nn = npd_core_tau(an, C.gates);
          const float u = h - nn;
          const float omz = 1.0f - z;
          const float dn = dh * omz;
          const float dz = dh * u;
          const float direct = dh * z;
          const float dan = npd_core_tau_slope(dn, an, nn, C.gates);
          const float dr = dan * ghn;
          const float daz = npd_core_sigma_slope(dz, (flags & 2) != 0, z, C.gates);
          const float dar = npd_core_sigma_slope(dr, (flags & 1) != 0, r, C.gates);
          const float dghn = dan * r;
          const bool dead = j >= H || bad[plant] != 0;
          b2[o] = dead ? 0.0f : dar;
          b3[o] = dead ? 0.0f : daz;
          b4[o] = dead ? 0.0f : dan;
          b5[o] = dead ? 0.0f : dghn;
          b0[o] = dead ? 0.0f : direct;
        }
        __syncthreads();
        npd_ppo_dw(C.gate[0], prow, first, b2, xs, tid);
        npd_ppo_dw(C.gate[1], prow, first, b3, xs, tid);
        npd_ppo_dw(C.gate[2], prow, first, b4, xs, tid);
        npd_ppo_dw(C.gate[3], prow, first, b2, b1, tid);
        npd_ppo_dw(C.gate[4], prow, first, b3, b1, tid);
        npd_ppo_dw(C.gate[5], prow, first, b5, b1, tid);
        const npd_policy_layer_t *const layers[3] = {&C.gate[3], &C.gate[4], &C.gate[5]};
        const float *const deltas[3] = {b2, b3, b5};
        npd_ppo_back_onto<3>(layers, deltas, P.theta, b0, fresh, tid);
      }
    }
    if (tid < NPD_PPO_ROWVALS) R.chain_stats[chain * NPD_PPO_ROWVALS + tid] = running;
  }
}

/* THE REFRESH OF THE STORED STATES (npb_policy_segment_starts): the forward sweep alone over the rollout's own tensors, one workgroup per tile
 * of 32 plants, serial in t; the state read in front of slot c * every, the restart applied, goes into row c of starts for c >= 1 */
template <int KC_MAX, int H_MAX>
__global__ __launch_bounds__(NPD_POLICY_LANES) void npb_segment_starts_kernel(npb_policy_t P, npd_policy_core_t C, npd_seq_starts_t G) {
  __shared__ float xs[KC_MAX * NPD_POLICY_STRIDE];
  __shared__ float buf[5][H_MAX * NPD_POLICY_STRIDE];
  __shared__ int bad[NPD_POLICY_TILE], fresh[NPD_POLICY_TILE];
  const int tid = threadIdx.x, KC_pad = (P.cells + 3) & ~3, H = C.H;
  const size_t n_plants = (size_t)G.n_plants, base = (size_t)blockIdx.x * NPD_POLICY_TILE;
  const int in_tile = npd_policy_in_tile(n_plants, base);
  npd_policy_tile_zero(xs, 0, KC_pad, tid);
  __syncthreads();
  auto words = [&](int s) {
    int restart = 0;
    if (tid < in_tile && s > 0) {
      const size_t now = (size_t)s * n_plants + base + tid, before = now - n_plants;
      restart = G.episode[now] != G.episode[before] || (G.ended[before] & NPD_SEQ_CUT) != 0;
    }
    fresh[tid] = restart;
    bad[tid] = tid >= in_tile;
  };
  auto first_of = [&](int row) -> const float * { return row < in_tile ? G.first + (base + row) * H : nullptr; };
  npd_seq_forward(P, C, G.obs, G.obs_f64, n_plants, base, in_tile, G.t, xs, buf[0], buf[1], buf[2], buf[3], buf[4], bad, fresh, tid, words, first_of, [&](int s) {
    if (s == 0 || s % G.every) return;
    npd_core_store(G.starts + ((size_t)(s / G.every) * n_plants + base) * H, buf[0], in_tile, H, tid);
  }, [](int) {});
}

/* ---- the launchers */
extern "C" void npb_launch_ppo_grad_seq(const npb_policy_t *P, const npd_policy_core_t *C, const npb_ppo_t *O, const npb_ppo_desc_t *D, const npb_ppo_more_t *M,
                                        const npb_ppo_seq_t *S, const npb_ppo_segments_t *G, double n, double *out, hipStream_t stream) {
  const npd_ppo_run_t R = npd_ppo_run(O, D, M, (int)(((int64_t)S->plants + D->rows_per_chain - 1) / D->rows_per_chain), n);
  npd_ppo_seq_run_t Q = {};
  Q.S = *S; Q.hseq = S->hidden ? S->hidden : O->hseq; Q.chunks = G ? G->chunks : 0;
  const int cap = D->max_blocks > 0 ? D->max_blocks : 2048;
  const dim3 grid((unsigned)(R.n_chains < cap ? R.n_chains : cap)), block(NPD_POLICY_LANES);
  if (npd_policy_small(P, C->H)) hipLaunchKernelGGL((npb_ppo_seq_kernel<NPD_POLICY_SMALL_CELLS, NPD_POLICY_SMALL_WIDTH>), grid, block, 0, stream, *P, *C, R, Q);
  else hipLaunchKernelGGL((npb_ppo_seq_kernel<NPB_FEATURES_CELLS_MAX, NPB_POLICY_WIDTH_MAX>), grid, block, 0, stream, *P, *C, R, Q);
  npb_launch_ppo_reduce(P, O, &R, out, stream);
}
extern "C" void npb_launch_segment_starts(const npb_policy_t *P, const npd_policy_core_t *C, const void *obs, int obs_f64, int t, int n_plants, int every,
                                          const int32_t *episode, const uint8_t *ended, float *starts, hipStream_t stream) {
  const npd_seq_starts_t G = {obs, obs_f64, t, n_plants, every, episode, ended, C->first, starts};
  const dim3 grid((unsigned)((n_plants + NPD_POLICY_TILE - 1) / NPD_POLICY_TILE)), block(NPD_POLICY_LANES);
  if (npd_policy_small(P, C->H)) hipLaunchKernelGGL((npb_segment_starts_kernel<NPD_POLICY_SMALL_CELLS, NPD_POLICY_SMALL_WIDTH>), grid, block, 0, stream, *P, *C, G);
  else hipLaunchKernelGGL((npb_segment_starts_kernel<NPB_FEATURES_CELLS_MAX, NPB_POLICY_WIDTH_MAX>), grid, block, 0, stream, *P, *C, G);
}
