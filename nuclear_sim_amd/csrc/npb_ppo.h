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
} npb_ppo_t;
/* the gradient of one minibatch: the gradient kernel (a workgroup a chain), the ascending sum over the chains, the finish.  O holds
 * room for ceil(count / rows_per_chain) chains.  M (NULL = every option off): value-loss clipping, and with kl_limit > 0 the finish ORs
 * the gate on O->gate */
void npb_launch_ppo_grad(const npb_policy_t *P, const npb_ppo_t *O, const npb_ppo_desc_t *D, const npb_ppo_more_t *M, hipStream_t stream);
/* one Adam step on P->theta from O->grad, O->step the step it is (already advanced): step_size = lr / (1 - b1^step) and root = sqrt(1 -
 * b2^step) are formed on the host, in double.  gated: the launch reads O->gate's stopped word and stores nothing when it is set */
void npb_launch_ppo_adam(const npb_policy_t *P, const npb_ppo_t *O, double lr, double b1, double b2, double eps, int gated, hipStream_t stream);
/* one shard's sums (npb_policy_shard_sums): the gradient kernel with the seeds' divisor (double)count_total, then a lane an entry of out
 * [P->log_std + NPD_PPO_ROWVALS] doubles: the ascending sum over the chains, not narrowed.  O's grad, stats, more and gate are not touched */
void npb_launch_ppo_shard_sums(const npb_policy_t *P, const npb_ppo_t *O, const npb_ppo_desc_t *D, const npb_ppo_more_t *M, int64_t count_total, double *out,
                               hipStream_t stream);
/* the combine (npb_policy_apply_shards, npb_policy_combine_shards): a lane a parameter adds S->sums' rows in ascending order onto 0.0,
 * narrows once and takes the tree's first level; then the finish over the 18 totals with n = count_total, S->kl_limit > 0 ORing the gate */
void npb_launch_ppo_combine(const npb_policy_t *P, const npb_ppo_t *O, const npb_ppo_shards_t *S, hipStream_t stream);
#ifdef __cplusplus
}
#endif
#endif
