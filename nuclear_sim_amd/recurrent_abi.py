"""include/npb.h npb_policy_core_t: a GRU cell in front of both nets of the policy (npb_set_policy_core; nuclear_sim_amd/recurrent.py) as the
binding passes it, npb_ppo_seq_t, where a minibatch of whole sequences came from (npb_policy_grad_seq), and npb_ppo_segments_t, which makes
those sequences truncated segments (npb_policy_grad_segments).  tests/test_recurrent_abi.py, tests/test_recurrent_train_abi.py and
tests/test_segments_abi.py hold the layouts to the compiler's."""
import ctypes

POLICY_GATES = {"soft": 0, "hard": 1}                                  # NPB_POLICY_GATES_SOFT / NPB_POLICY_GATES_HARD (recurrent.GATES)


class NpbPolicyCore(ctypes.Structure):
    """npb_policy_core_t: the width, the gates, the caller's hidden, first and final tensors and final's rows per plant"""
    _fields_ = [("width", ctypes.c_int), ("gates", ctypes.c_int), ("hidden", ctypes.c_void_p), ("first", ctypes.c_void_p),
                ("final", ctypes.c_void_p), ("final_rows", ctypes.c_int)]


class NpbPpoSeq(ctypes.Structure):
    """npb_ppo_seq_t: slots and sequences, the minibatch's index, the rollout's plants and its episode, ended and first tensors, and
    the optional output of the states h'"""
    _fields_ = [("t", ctypes.c_int), ("plants", ctypes.c_int), ("index", ctypes.c_void_p), ("n_plants", ctypes.c_int), ("episode", ctypes.c_void_p),
                ("ended", ctypes.c_void_p), ("first", ctypes.c_void_p), ("hidden", ctypes.c_void_p)]


class NpbPpoSegments(ctypes.Structure):
    """npb_ppo_segments_t: the slots of a segment and the segments a plant's recorded slots are cut into"""
    _fields_ = [("every", ctypes.c_int), ("chunks", ctypes.c_int)]
