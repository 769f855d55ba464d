"""CPU: training one policy across shards (npb_policy_shard_sums, npb_policy_apply_shards and their companions) is declared by
include/npb.h, exported by libnpb.so and bound in one group; the binding lays npb_ppo_shards_t out as a C compiler does (a small compiled
probe prints sizeof and every offsetof); the library's own check, which needs no handle and reads no device memory, accepts a valid
descriptor and names every refusal the header lists; what the existing suites pin of the ABI is untouched.  No compute calls."""
import ctypes

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib, ppo, ppo_abi

ENTRY_POINTS = ("npb_ppo_shard_count", "npb_ppo_shards_check", "npb_policy_shard_sums", "npb_policy_apply_shards", "npb_policy_combine_shards")
A8 = 0x7000       # a "device address" the check only looks at: never dereferenced
THETA, AXES = 1000, 3


def _section():
    text = abi.header_text()
    return text[text.index("TRAINING ONE POLICY ACROSS SHARDS"):]


def test_header_declares_the_entry_points_and_states_the_layout_and_the_formulas():
    """Fails without the feature: the header declares none of them"""
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_PPO_SHARD_ROWS") == 18 == len(ppo.SHARD_ROWS) == _lib.PPO_SHARD_ROWS == ppo_abi.PPO_SHARD_ROWS
    assert abi.define("NPB_PPO_SHARDS_MAX") == 64 == ppo.SHARDS_MAX == _lib.PPO_SHARDS_MAX == ppo_abi.PPO_SHARDS_MAX
    assert abi.define("NPB_VERSION") == 154 and abi.define("NPB_PPO_STATS") == 8 and abi.define("NPB_PPO_STATS_MORE") == 4
    text = " ".join(_section().split())
    for words in ("theta_count - 2 * n_axes + NPB_PPO_SHARD_ROWS", "up to where log_std starts",
                  "policy_loss 8, kl 9, clipped 10, skipped 11, value_loss 12, vf_clipped 13, ret 14, ret2 15, diff 16, diff2 17",
                  "dmean[a] = (float)(((c * d[a]) / std[a]) / (double)count_total)", "dls[a] = (c * (d[a] * d[a] - 1.0)) / (double)count_total",
                  "total[e] = 0.0; for w ascending total[e] = total[e] + sums[w][e]", "grad(log_std[a]) = (float)(total_dls[a] - ent_coef)",
                  "npb_policy_update_more, bit for bit", "the gate on the GLOBAL approx_kl", "NPB_VERSION stays 154", "8 * L bytes",
                  "no atomics and no scratch"):
        assert words in text, words
    not_here = text[text.index("Not here:"):]
    not_here = not_here[:not_here.index("*/")]
    for words in ("synchronising the running normaliser between shards", "advantage moments over all", "different numbers of updates",
                  "overlapping the exchange", "more than one device"):
        assert words in not_here, words
    # and the training section no longer says that the exchange is missing
    whole = abi.header_text()
    training = whole[whole.index("Not here: a shared trunk, learning-rate schedules"):]
    assert "exchange between devices" not in training[:training.index("\n *\n")]


def test_library_exports_and_binding_declares_them_in_one_group():
    abi.check_entry_points(ENTRY_POINTS, [("npb_policy_shard_sums", None, None, None, 10, None, None), ("npb_policy_apply_shards", None, None, 1e-3, 0.9, 0.999, 1e-5, None),
                                          ("npb_policy_combine_shards", None, None, None)])
    group = dict(_lib.ENTRY_POINTS)["npb_policy_shard_sums"]
    assert set(group) == set(ENTRY_POINTS)      # one group, detected by name
    L = abi.library()
    for theta, axes in ((THETA, AXES), (19, 1), (5000000, 8)):
        assert L.npb_ppo_shard_count(theta, axes) == ppo.shard_size(theta, axes) == theta - 2 * axes + 18


def test_the_binding_lays_the_descriptor_out_as_the_compiler_does():
    assert _lib.NpbPpoShards is ppo_abi.NpbPpoShards
    structs = {"npb_ppo_shards_t": _lib.NpbPpoShards, "npb_ppo_more_t": _lib.NpbPpoMore, "npb_ppo_desc_t": _lib.NpbPpoDesc}
    got, values = abi.probe(structs, ["NPB_PPO_SHARD_ROWS", "NPB_PPO_SHARDS_MAX", "NPB_VERSION"])
    assert got == abi.layout(structs) and values == [18, 64, 154]
    assert [f[0] for f in _lib.NpbPpoShards._fields_] == ["sums", "n_shards", "count_total", "ent_coef", "max_grad_norm", "kl_limit"]
    assert [f[0] for f in _lib.NpbPpoMore._fields_] == ["value_old", "clip_vf", "kl_limit"]      # untouched


def _shards(**members):
    s = _lib.NpbPpoShards()
    s.sums, s.n_shards, s.count_total, s.ent_coef, s.max_grad_norm, s.kl_limit = A8, 3, 199, 0.01, 0.5, 0.03
    for name, value in members.items():
        setattr(s, name, value)
    return s


def _why(s, count=THETA, axes=AXES):
    return abi.why(abi.library().npb_ppo_shards_check, None if s is None else ctypes.byref(s), count, axes)


def test_the_check_accepts_a_valid_descriptor():
    assert _why(_shards()) is None
    for members in (dict(n_shards=1), dict(n_shards=64), dict(count_total=1), dict(count_total=2 ** 53), dict(ent_coef=0.0), dict(ent_coef=-0.5),
                    dict(max_grad_norm=0.0), dict(kl_limit=0.0), dict(kl_limit=1e-12), dict(sums=A8 + 8)):
        assert _why(_shards(**members)) is None, members
    assert _why(_shards(), count=19, axes=8) is None and _why(_shards(), count=3, axes=1) is None


REFUSALS = [
    ("NULL sums", dict(sums=None), "sums is NULL"),
    ("misaligned sums", dict(sums=A8 + 4), "a misaligned sums"),
    ("no shards", dict(n_shards=0), "n_shards must be 1 .. NPB_PPO_SHARDS_MAX"),
    ("negative shards", dict(n_shards=-1), "n_shards must be 1 .. NPB_PPO_SHARDS_MAX"),
    ("65 shards", dict(n_shards=65), "n_shards must be 1 .. NPB_PPO_SHARDS_MAX"),
    ("count_total 0", dict(count_total=0), "count_total must be 1 .. 2^53"),
    ("negative count_total", dict(count_total=-5), "count_total must be 1 .. 2^53"),
    ("count_total beyond 2^53", dict(count_total=2 ** 53 + 1), "count_total must be 1 .. 2^53"),
    ("NaN ent_coef", dict(ent_coef=float("nan")), "ent_coef must be finite"),
    ("infinite ent_coef", dict(ent_coef=float("-inf")), "ent_coef must be finite"),
    ("NaN max_grad_norm", dict(max_grad_norm=float("nan")), "max_grad_norm must be finite and >= 0"),
    ("infinite max_grad_norm", dict(max_grad_norm=float("inf")), "max_grad_norm must be finite and >= 0"),
    ("negative max_grad_norm", dict(max_grad_norm=-0.5), "max_grad_norm must be finite and >= 0"),
    ("negative kl_limit", dict(kl_limit=-1e-3), "kl_limit must be finite and >= 0"),
    ("infinite kl_limit", dict(kl_limit=float("inf")), "kl_limit must be finite and >= 0"),
    ("NaN kl_limit", dict(kl_limit=float("nan")), "kl_limit must be finite and >= 0"),
]


@pytest.mark.parametrize("what, members, reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_check_names_every_refusal(what, members, reason):
    why = _why(_shards(**members))
    assert why is not None and why.startswith("npb_policy_apply_shards: ") and reason in why, (what, why)


def test_the_check_refuses_a_null_descriptor_and_a_theta_with_no_weights_and_the_header_lists_them():
    assert "a NULL descriptor" in _why(None)
    assert "axis count" in _why(_shards(), axes=0) and "axis count" in _why(_shards(), axes=9)
    assert "leaves no weights" in _why(_shards(), count=6, axes=3)
    text = " ".join(_section().split())
    listed = text[text.index("npb_ppo_shards_check(shards, count, n_axes): the host-only validator"):]
    listed = listed[:listed.index("One exchange moves")]
    for words in ("a NULL descriptor or NULL sums", "sums misaligned for a double", "n_shards outside 1 .. NPB_PPO_SHARDS_MAX (64)", "count_total < 1 * or beyond 2^53",
                  "an ent_coef or max_grad_norm that is not finite, or max_grad_norm < 0", "a kl_limit that is negative or not finite"):
        assert words in listed, words
    refused = text[text.index("npb_policy_shard_sums(h, desc, more, count_total, out, stream)"):]
    for words in ("count_total < desc->count", "NULL or misaligned out", "kl_limit > 0"):
        assert words in refused[:refused.index("npb_policy_apply_shards(h, shards, lr")], words
