"""CPU: the policy on the device -- an MLP actor-critic with Gaussian sampling between the features and the controls' input, and K steps in
one call (npb_set_policy and its companions) -- is declared by include/npb.h, exported by libnpb.so and bound; the binding lays the
descriptor out as a C compiler does (a small compiled probe prints sizeof and every offsetof); the library's own check, which needs no
handle and reads no device memory, accepts a valid descriptor and names every refusal the header lists; the parameter count is the
statement's.  No compute calls.

The header keeps NPB_VERSION where the suites of the entry-point groups before this one pin it: the new entry points are detected by name."""
import ctypes

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

ENTRY_POINTS = ("npb_set_policy", "npb_policy_check", "npb_policy_count", "npb_policy_load", "npb_policy_values", "npb_policy_noise",
                "npb_policy_get_state", "npb_policy_set_state", "npb_collect")
A4 = 0x7000       # "device addresses" the check only looks at: never dereferenced
CELLS, AXES = 15, 3


def test_header_declares_the_entry_points_the_maxima_and_the_rules_of_the_road():
    text = abi.header_text()
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_POLICY_HIDDEN_MAX") == 3
    assert abi.define("NPB_POLICY_WIDTH_MAX") == 128
    assert abi.define("NPB_VERSION") == 154
    for words in ("acc = fmaf(x[k], W[j][k], acc)", "extended with +0.0 cells and +0.0 weights to a multiple of 4", "A subnormal result or accumulator is outside the contract",
                  "the device takes no exponential", "Philox4x32-10", "(first_plant + p, t & 0xffffffff, t >> 32, j)", "(w0 * 2^20 + (w1 >> 12) + 0.5) * 2^-52",
                  "6.283185307179586", "0.9189385332046727", "the density of the UNROUNDED action", "THE quiet NaN in every output", "v_mfma_f32_32x32x2_f32",
                  "no synchronisation for a device source", "Not here: a shared trunk", "noise that restarts with the episode",
                  # the tails of the sections that used to name this as missing now point here, and keep what their own suites pin
                  "K steps in\n * one call.", "its npb_collect runs K steps in one call", "have the policy's section below"):
        assert words in text, words


def test_library_exports_and_binding_declares_them():
    abi.check_entry_points(ENTRY_POINTS, [("npb_set_policy", None, None), ("npb_policy_load", None, None, 0, None),
                                          ("npb_policy_values", None, None, 0, 0, None, None), ("npb_policy_noise", None, 0, None, None, None),
                                          ("npb_policy_get_state", None, None), ("npb_policy_set_state", None, 0),
                                          ("npb_collect", None, 1, None, None, None, None, None, None)])


def test_the_binding_lays_the_descriptor_out_as_the_compiler_does():
    from nuclear_sim_amd import policy
    structs = {"npb_policy_desc_t": _lib.NpbPolicyDesc}
    got, values = abi.probe(structs, ["NPB_POLICY_RELU", "NPB_POLICY_TANH", "NPB_POLICY_HIDDEN_MAX", "NPB_POLICY_WIDTH_MAX"])
    assert got == abi.layout(structs)
    assert values == [_lib.POLICY_ACTIVATIONS["relu"], _lib.POLICY_ACTIVATIONS["tanh"], _lib.POLICY_HIDDEN_MAX, _lib.POLICY_WIDTH_MAX]
    assert _lib.POLICY_ACTIVATIONS == policy.ACTIVATIONS and (_lib.POLICY_HIDDEN_MAX, _lib.POLICY_WIDTH_MAX) == (policy.HIDDEN_MAX, policy.WIDTH_MAX) == (3, 128)


class _Desc:
    """a valid descriptor: actor (33, 17), critic (7,), tanh, both outputs and both slots of three extras"""

    def __init__(self):
        self.d = d = _lib.NpbPolicyDesc()
        d.actor_layers, d.critic_layers, d.activation = 2, 1, 1
        d.actor_width[0], d.actor_width[1], d.critic_width[0] = 33, 17, 7
        d.seed, d.first_plant = 2 ** 64 - 1, 40
        d.value, d.logp, d.extras_in, d.n_extras, d.value_slot, d.logp_slot = A4, A4 + 4, A4 + 16, 3, 0, 2


def _why(D, n=70, cells=CELLS, axes=AXES):
    return abi.why(abi.library().npb_policy_check, ctypes.byref(D.d), n, cells, axes)


def _set(**members):
    def change(D):
        for name, value in members.items():
            if isinstance(value, tuple):
                getattr(D.d, name[:-1])[int(name[-1])] = value[0]
            else:
                setattr(D.d, name, value)
    return change


def test_the_check_accepts_valid_policies_and_null_and_counts_the_parameters():
    from nuclear_sim_amd import policy
    assert _why(_Desc()) is None
    assert abi.library().npb_policy_check(None, 70, CELLS, AXES) is None
    for change, kw in ((_set(actor_layers=3, actor_width2=(128,)), {}), (_set(actor_layers=1, actor_width0=(1,)), {}), (_set(activation=0), {}),
                       (_set(extras_in=None, value_slot=-1, logp_slot=-1, n_extras=0), {}), (_set(value_slot=-1), {}), (_set(deterministic=1), {}),
                       (_set(first_plant=2 ** 32 - 70), {}), (_set(), {"n": 1, "cells": 256, "axes": 8}), (_set(), {"cells": 1, "axes": 1})):
        D = _Desc(); change(D)
        assert _why(D, **kw) is None, kw
    assert abi.library().npb_policy_count(ctypes.byref(_Desc().d), CELLS, AXES) == policy.theta_size(CELLS, AXES, (33, 17), (7,))
    D = _Desc(); _set(actor_layers=3, actor_width2=(128,), critic_layers=3, critic_width1=(64,), critic_width2=(5,))(D)
    assert abi.library().npb_policy_count(ctypes.byref(D.d), 256, 8) == policy.theta_size(256, 8, (33, 17, 128), (7, 64, 5))
    assert abi.library().npb_policy_count(None, CELLS, AXES) == 0


REFUSALS = [
    ("n_plants", _set(), {"n": 0}, "n_plants must be >= 1"),
    ("no features", _set(), {"cells": 0}, "a policy needs features"),
    ("too many cells", _set(), {"cells": 257}, "1 .. NPB_FEATURES_CELLS_MAX (256) cells"),
    ("no controls", _set(), {"axes": 0}, "a policy needs controls"),
    ("too many axes", _set(), {"axes": 9}, "axis count must be 1 .. NPB_CONTROLS_AXES_MAX (8)"),
    ("no actor layers", _set(actor_layers=0), {}, "1 .. NPB_POLICY_HIDDEN_MAX (3) hidden layers"),
    ("too many critic layers", _set(critic_layers=4), {}, "1 .. NPB_POLICY_HIDDEN_MAX (3) hidden layers"),
    ("a zero actor width", _set(actor_width1=(0,)), {}, "a hidden layer of the actor must be 1 .. NPB_POLICY_WIDTH_MAX (128) wide"),
    ("too wide a critic", _set(critic_width0=(129,)), {}, "a hidden layer of the critic must be 1 .. NPB_POLICY_WIDTH_MAX (128) wide"),
    ("activation", _set(activation=2), {}, "an unknown activation"),
    ("negative first_plant", _set(first_plant=-1), {}, "first_plant must be >= 0"),
    ("first_plant beyond the word", _set(first_plant=2 ** 32 - 69), {}, "first_plant + n_plants <= 2^32"),
    ("NULL value", _set(value=None), {}, "NULL value or logp"),
    ("NULL logp", _set(logp=None), {}, "NULL value or logp"),
    ("misaligned value", _set(value=A4 + 2), {}, "misaligned value or logp"),
    ("misaligned logp", _set(logp=A4 + 1), {}, "misaligned value or logp"),
    ("a slot without extras_in", _set(extras_in=None, logp_slot=-1), {}, "a value or logp slot without extras_in"),
    ("extras_in without a count", _set(n_extras=0), {}, "an extras count outside 1 .. NPB_ROLLOUT_EXTRAS_MAX (8)"),
    ("too many extras", _set(n_extras=9), {}, "an extras count outside 1 .. NPB_ROLLOUT_EXTRAS_MAX (8)"),
    ("a slot beyond the extras", _set(logp_slot=3), {}, "a value or logp slot outside -1 .. E - 1"),
    ("a slot below -1", _set(value_slot=-2), {}, "a value or logp slot outside -1 .. E - 1"),
    ("both in one slot", _set(value_slot=2), {}, "value and logp in the same slot"),
    ("misaligned extras_in", _set(extras_in=A4 + 18), {}, "a misaligned extras_in"),
]


@pytest.mark.parametrize("what, change, kw, reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_check_names_every_refusal(what, change, kw, reason):
    abi.check_refusal(_Desc, _why, "npb_set_policy: ", what, change, reason, kw)
