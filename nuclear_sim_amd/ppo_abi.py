"""include/npb.h npb_ppo_more_t: the options of one training update of the policy (npb_policy_grad_more, npb_policy_update_more) as the
binding passes them.  tests/test_ppo_options_abi.py holds the layout to the compiler's."""
import ctypes

PPO_STATS_MORE = 4                                                     # NPB_PPO_STATS_MORE (ppo.STATS_MORE)


class NpbPpoMore(ctypes.Structure):
    """npb_ppo_more_t: the rollout's old values with clip_vf (0 = off), and the gate's kl_limit (0 = this update has no gate)"""
    _fields_ = [("value_old", ctypes.c_void_p), ("clip_vf", ctypes.c_double), ("kl_limit", ctypes.c_double)]


# npb_ppo_shards_t: the shards' vectors of one update across shards (npb_policy_apply_shards, npb_policy_combine_shards).
# tests/test_ppo_shards_abi.py holds the layout to the compiler's.
PPO_SHARD_ROWS = 18                                                    # NPB_PPO_SHARD_ROWS (ppo.SHARD_ROWS)
PPO_SHARDS_MAX = 64                                                    # NPB_PPO_SHARDS_MAX (ppo.SHARDS_MAX)


class NpbPpoShards(ctypes.Structure):
    """npb_ppo_shards_t: the device [n_shards][L] doubles in shard order, the rows of the whole update, and the combine's ent_coef,
    max_grad_norm (0 = off) and kl_limit (0 = no gate)"""
    _fields_ = [("sums", ctypes.c_void_p), ("n_shards", ctypes.c_int), ("count_total", ctypes.c_int64), ("ent_coef", ctypes.c_double),
                ("max_grad_norm", ctypes.c_double), ("kl_limit", ctypes.c_double)]
