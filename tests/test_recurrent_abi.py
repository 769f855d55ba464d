"""CPU: the recurrent policy on the device -- a GRU cell in front of actor and critic, its hidden state carried per plant
(npb_set_policy_core and its companions) -- is declared by include/npb.h, exported by libnpb.so and bound; the binding lays
npb_policy_core_t out as a C compiler does (the compiled probe prints sizeof and every offsetof); the library's own check, which needs no
handle and reads no device memory, accepts a valid core and names every refusal the header lists; the parameter count is the statement's.
No compute calls.  NPB_VERSION stays where it was and npb_policy_desc_t keeps its layout: the entry points are detected by name."""
import ctypes

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib, recurrent

ENTRY_POINTS = ("npb_set_policy_core", "npb_policy_core_check", "npb_policy_core_count", "npb_policy_values_hidden", "npb_policy_core_get_state",
                "npb_policy_core_set_state")
A4 = 0x7000       # "device addresses" the check only looks at: never dereferenced
CELLS, AXES = 15, 3


def test_header_declares_the_entry_points_and_states_the_cell():
    text = abi.header_text()
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_VERSION") == 154
    for words in ("W_ih[3H][K * C] | b_ih[3H] | W_hh[3H][H] | b_hh[3H]", "h'[j] = n[j] + z[j] * (h[j] - n[j])", "n[j] = T(gi[2H + j] + r[j] * gh[2H + j])",
                  "y = 0.25f * a + 0.5f", "S(a) = 0.5f * tanh(0.5f * a) + 0.5f", "critic(GRU(final_obs[row], final[row]))", "bootstraps from +0.0",
                  "training through time is not built".capitalize(), "LSTM cells"):
        assert words in text, words
    assert "recurrent nets;" not in text      # the policy section's "Not here" no longer lists them


def test_library_exports_and_binding_declares_them():
    abi.check_entry_points(ENTRY_POINTS, [("npb_set_policy_core", None, None, None), ("npb_policy_values_hidden", None, None, 0, 0, None, None, None),
                                          ("npb_policy_core_get_state", None, None, None, None, None),
                                          ("npb_policy_core_set_state", None, None, None, None, None)])


def test_the_binding_lays_the_core_out_as_the_compiler_does_and_leaves_the_descriptor_alone():
    structs = {"npb_policy_core_t": _lib.NpbPolicyCore, "npb_policy_desc_t": _lib.NpbPolicyDesc}
    got, values = abi.probe(structs, ["NPB_POLICY_GATES_SOFT", "NPB_POLICY_GATES_HARD"])
    assert got == abi.layout(structs)
    assert values == [_lib.POLICY_GATES["soft"], _lib.POLICY_GATES["hard"]] and _lib.POLICY_GATES == recurrent.GATES
    assert ctypes.sizeof(_lib.NpbPolicyDesc) == 96      # what it was before there was a core: 9 ints, padded, then 56 bytes
    assert recurrent.CORE_MAX == _lib.POLICY_WIDTH_MAX


class _Core:
    """a valid core: 33 wide, hard gates, all three tensors, two rows of final per plant"""

    def __init__(self):
        self.d = d = _lib.NpbPolicyCore()
        d.width, d.gates, d.hidden, d.first, d.final, d.final_rows = 33, 1, A4, A4 + 0x100, A4 + 0x200, 2


def _why(D, n=70, cells=CELLS):
    return abi.why(abi.library().npb_policy_core_check, ctypes.byref(D.d), n, cells)


def _desc(actor=(33, 17), critic=(7,)):
    d = _lib.NpbPolicyDesc()
    d.actor_layers, d.critic_layers, d.activation = len(actor), len(critic), 0
    for l, w in enumerate(actor):
        d.actor_width[l] = w
    for l, w in enumerate(critic):
        d.critic_width[l] = w
    d.value, d.logp, d.value_slot, d.logp_slot = A4, A4 + 4, -1, -1
    return d


def test_the_check_accepts_valid_cores_and_null_and_counts_the_parameters():
    L = abi.library()
    assert _why(_Core()) is None
    assert L.npb_policy_core_check(None, 70, CELLS) is None
    for change, kw in ((abi.set_members(width=1), {}), (abi.set_members(width=128), {}), (abi.set_members(gates=0), {}), (abi.set_members(first=None), {}),
                       (abi.set_members(final=None, final_rows=0), {}), (abi.set_members(), {"n": 1, "cells": 256}), (abi.set_members(), {"cells": 1})):
        D = _Core(); change(D)
        assert _why(D, **kw) is None, kw
    d = _desc()
    assert L.npb_policy_core_count(ctypes.byref(d), ctypes.byref(_Core().d), CELLS, AXES) == recurrent.theta_size(CELLS, AXES, (33, 17), (7,), 33)
    D = _Core(); D.d.width = 128
    assert L.npb_policy_core_count(ctypes.byref(_desc((128,), (1,))), ctypes.byref(D.d), 256, 8) == recurrent.theta_size(256, 8, (128,), (1,), 128)
    assert L.npb_policy_core_count(ctypes.byref(d), None, CELLS, AXES) == L.npb_policy_count(ctypes.byref(d), CELLS, AXES)      # no core: the policy's
    assert L.npb_policy_core_count(None, ctypes.byref(_Core().d), CELLS, AXES) == 0


REFUSALS = [
    ("n_plants", abi.set_members(), {"n": 0}, "n_plants must be >= 1"),
    ("no features", abi.set_members(), {"cells": 0}, "1 .. NPB_FEATURES_CELLS_MAX (256) cells"),
    ("too many cells", abi.set_members(), {"cells": 257}, "1 .. NPB_FEATURES_CELLS_MAX (256) cells"),
    ("no width", abi.set_members(width=0), {}, "the core must be 1 .. NPB_POLICY_WIDTH_MAX (128) wide"),
    ("too wide", abi.set_members(width=129), {}, "the core must be 1 .. NPB_POLICY_WIDTH_MAX (128) wide"),
    ("gates", abi.set_members(gates=2), {}, "unknown gates"),
    ("NULL hidden", abi.set_members(hidden=None), {}, "NULL hidden"),
    ("negative final_rows", abi.set_members(final_rows=-1), {}, "final_rows must be >= 0"),
    ("final without rows", abi.set_members(final_rows=0), {}, "final goes with final_rows > 0"),
    ("rows without final", abi.set_members(final=None), {}, "final goes with final_rows > 0"),
    ("rows beyond int32", abi.set_members(final_rows=2 ** 31 // 70 + 1), {}, "beyond what the rollout's final_row (int32) holds"),
    ("misaligned hidden", abi.set_members(hidden=A4 + 2), {}, "misaligned hidden, first or final"),
    ("misaligned first", abi.set_members(first=A4 + 1), {}, "misaligned hidden, first or final"),
    ("misaligned final", abi.set_members(final=A4 + 3), {}, "misaligned hidden, first or final"),
]


@pytest.mark.parametrize("what, change, kw, reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_check_names_every_refusal(what, change, kw, reason):
    abi.check_refusal(_Core, _why, "npb_set_policy_core: ", what, change, reason, kw)
