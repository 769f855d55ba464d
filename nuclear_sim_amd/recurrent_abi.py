"""include/npb.h npb_policy_core_t: a GRU cell in front of both nets of the policy (npb_set_policy_core; nuclear_sim_amd/recurrent.py) as the
binding passes it.  tests/test_recurrent_abi.py holds the layout to the compiler's."""
import ctypes

POLICY_GATES = {"soft": 0, "hard": 1}                                  # NPB_POLICY_GATES_SOFT / NPB_POLICY_GATES_HARD (recurrent.GATES)


class NpbPolicyCore(ctypes.Structure):
    """npb_policy_core_t: the width, the gates, the caller's hidden, first and final tensors and final's rows per plant"""
    _fields_ = [("width", ctypes.c_int), ("gates", ctypes.c_int), ("hidden", ctypes.c_void_p), ("first", ctypes.c_void_p),
                ("final", ctypes.c_void_p), ("final_rows", ctypes.c_int)]
