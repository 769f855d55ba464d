"""include/npb.h npb_ppo_more_t: the options of one training update of the policy (npb_policy_grad_more, npb_policy_update_more) as the
binding passes them.  tests/test_ppo_options_abi.py holds the layout to the compiler's."""
import ctypes

PPO_STATS_MORE = 4                                                     # NPB_PPO_STATS_MORE (ppo.STATS_MORE)


class NpbPpoMore(ctypes.Structure):
    """npb_ppo_more_t: the rollout's old values with clip_vf (0 = off), and the gate's kl_limit (0 = this update has no gate)"""
    _fields_ = [("value_old", ctypes.c_void_p), ("clip_vf", ctypes.c_double), ("kl_limit", ctypes.c_double)]
