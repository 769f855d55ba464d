"""CPU: the rollout -- trajectories recorded on the device and their GAE advantages (npb_set_rollout and its companions) -- is declared by
include/npb.h, exported by libnpb.so and bound; the binding lays both descriptors out as a C compiler does (a small compiled probe prints
sizeof and every offsetof); the library's own check, which needs no handle and reads no device memory, accepts a valid descriptor and names
every refusal the header lists.  No compute calls.

The header keeps NPB_VERSION where the suites of the entry-point groups before this one pin it: the new entry points are detected by name."""
import ctypes

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

ENTRY_POINTS = ("npb_set_rollout", "npb_rollout_check", "npb_rollout_begin", "npb_rollout_steps", "npb_rollout_cut", "npb_rollout_advantages")
STRUCTS = {"npb_rollout_desc_t": _lib.NpbRolloutDesc, "npb_rollout_advantages_desc_t": _lib.NpbRolloutAdvantagesDesc}
A16 = 0x7000       # "device addresses" the check only looks at: never dereferenced
CELLS, AXES = 12, 3


def test_header_declares_the_entry_points_the_maxima_and_the_rules_of_the_road():
    text = abi.header_text()
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_ROLLOUT_HORIZON_MAX") == 4096
    assert abi.define("NPB_ROLLOUT_EXTRAS_MAX") == 8
    assert abi.define("NPB_VERSION") == 154
    for words in ("termination wins", "the rollout does not wrap silently", "R is derived, not tuned", "ceil(T / max_episode_steps)",
                  "carry is a select, not a product with 1 - done", "the value of the TERMINAL state", "every operation rounded on its own",
                  "the recurrence is not restated as a scan", "No atomics", "are not stored: their bootstrap is 0",
                  "Not here: advantage normalisation", "minibatch shuffling", "a checkpoint of a half-filled rollout", "half types", "V-trace",
                  "rollouts without features"):
        assert words in text, words


def test_library_exports_and_binding_declares_them():
    abi.check_entry_points(ENTRY_POINTS, [("npb_set_rollout", None, None), ("npb_rollout_begin", None, None), ("npb_rollout_steps", None),
                                          ("npb_rollout_cut", None, None, None), ("npb_rollout_advantages", None, None, None)])


def test_the_binding_lays_the_descriptors_out_as_the_compiler_does():
    from nuclear_sim_amd import rollout
    got, values = abi.probe(STRUCTS, ["NPB_ROLLOUT_TERMINATED", "NPB_ROLLOUT_TRUNCATED", "NPB_ROLLOUT_CUT", "NPB_ROLLOUT_F32", "NPB_ROLLOUT_F64"])
    B, D = _lib.ROLLOUT_BITS, _lib.ROLLOUT_DTYPES
    assert got == abi.layout(STRUCTS) and values == [B["terminated"], B["truncated"], B["cut"], D["float32"], D["float64"]]
    assert (B["terminated"], B["truncated"], B["cut"]) == (rollout.TERMINATED, rollout.TRUNCATED, rollout.CUT) == (1, 2, 4)
    assert (_lib.ROLLOUT_HORIZON_MAX, _lib.ROLLOUT_EXTRAS_MAX) == (rollout.HORIZON_MAX, rollout.EXTRAS_MAX) == (4096, 8)


class _Desc:
    """a valid descriptor: 16 slots, 2 extras, 4 rows per plant, every buffer given"""

    def __init__(self):
        self.d = d = _lib.NpbRolloutDesc()
        d.horizon, d.n_extras, d.final_rows = 16, 2, 4
        d.extras_in, d.obs, d.act, d.extra, d.final_obs = A16, A16 + 16, A16 + 32, A16 + 48, A16 + 64
        d.reward, d.ended, d.episode, d.final_row = A16 + 8, A16 + 1, A16 + 4, A16 + 12


def _why(D, n=70, cells=CELLS, axes=AXES):
    return abi.why(abi.library().npb_rollout_check, ctypes.byref(D.d), n, cells, axes)


_set = abi.set_members


def test_the_check_accepts_valid_rollouts_and_null():
    assert _why(_Desc()) is None
    assert abi.library().npb_rollout_check(None, 70, CELLS, AXES) is None
    for change, kw in ((_set(horizon=1), {}), (_set(horizon=4096), {}), (_set(n_extras=8), {}), (_set(act=None), {"axes": 0}),
                       (_set(n_extras=0, extras_in=None, extra=None), {}), (_set(final_rows=0, final_obs=None), {}),
                       (_set(final_rows=0), {}), (_set(), {"n": 1, "cells": 1, "axes": 8})):
        D = _Desc(); change(D)
        assert _why(D, **kw) is None, kw


REFUSALS = [
    ("n_plants", _set(), {"n": 0}, "n_plants must be >= 1"),
    ("no features", _set(), {"cells": 0}, "a rollout needs features"),
    ("no horizon", _set(horizon=0), {}, "horizon must be 1 .. NPB_ROLLOUT_HORIZON_MAX (4096)"),
    ("too long a horizon", _set(horizon=4097), {}, "horizon must be 1 .. NPB_ROLLOUT_HORIZON_MAX (4096)"),
    ("negative extras", _set(n_extras=-1), {}, "extras count must be 0 .. NPB_ROLLOUT_EXTRAS_MAX (8)"),
    ("too many extras", _set(n_extras=9), {}, "extras count must be 0 .. NPB_ROLLOUT_EXTRAS_MAX (8)"),
    ("act without axes", _set(), {"axes": 0}, "an act buffer without axes"),
    ("axes without act", _set(act=None), {}, "the act buffer is NULL"),
    ("negative final_rows", _set(final_rows=-1), {}, "final_rows must be >= 0"),
    ("rows beyond int32", _set(final_rows=4096), {"n": 1 << 20}, "beyond what final_row (int32) holds"),
    ("rows without final_obs", _set(final_obs=None), {}, "final_rows > 0 and final_obs is NULL"),
    ("NULL obs", _set(obs=None), {}, "NULL obs, reward, ended, episode or final_row"),
    ("NULL reward", _set(reward=None), {}, "NULL obs, reward, ended, episode or final_row"),
    ("NULL ended", _set(ended=None), {}, "NULL obs, reward, ended, episode or final_row"),
    ("NULL episode", _set(episode=None), {}, "NULL obs, reward, ended, episode or final_row"),
    ("NULL final_row", _set(final_row=None), {}, "NULL obs, reward, ended, episode or final_row"),
    ("extras without their input", _set(extras_in=None), {}, "extras without their input"),
    ("extras without their buffer", _set(extra=None), {}, "extras without their input (extras_in) or their buffer (extra)"),
    ("misaligned obs", _set(obs=A16 + 8), {}, "misaligned obs, act, extras_in, extra or final_obs"),
    ("misaligned act", _set(act=A16 + 4), {}, "misaligned obs, act, extras_in, extra or final_obs"),
    ("misaligned extras_in", _set(extras_in=A16 + 4), {}, "misaligned obs, act, extras_in, extra or final_obs"),
    ("misaligned extra", _set(extra=A16 + 8), {}, "misaligned obs, act, extras_in, extra or final_obs"),
    ("misaligned final_obs", _set(final_obs=A16 + 12), {}, "misaligned obs, act, extras_in, extra or final_obs"),
    ("misaligned reward", _set(reward=A16 + 4), {}, "a misaligned reward buffer"),
    ("misaligned episode", _set(episode=A16 + 2), {}, "misaligned episode or final_row"),
    ("misaligned final_row", _set(final_row=A16 + 1), {}, "misaligned episode or final_row"),
]


@pytest.mark.parametrize("what, change, kw, reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_check_names_every_refusal(what, change, kw, reason):
    abi.check_refusal(_Desc, _why, "npb_set_rollout: ", what, change, reason, kw)
