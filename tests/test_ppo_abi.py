"""CPU: training the policy on the device (npb_policy_grad and its companions) is declared by include/npb.h, exported by libnpb.so and
bound; the binding lays the descriptor out as a C compiler does (a small compiled probe prints sizeof and every offsetof); the library's
own check, which needs no handle and reads no device memory, accepts a valid descriptor and names every refusal the header lists.  No
compute calls."""
import ctypes

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

ENTRY_POINTS = ("npb_ppo_check", "npb_policy_grad", "npb_policy_adam", "npb_policy_update", "npb_policy_get_grad", "npb_policy_get_stats",
                "npb_policy_get_theta", "npb_policy_optimizer_get_state", "npb_policy_optimizer_set_state")
A8 = 0x7000       # "device addresses" the check only looks at: never dereferenced
CELLS, AXES = 15, 3


def test_header_declares_the_entry_points_and_states_the_contract():
    text = abi.header_text()
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_PPO_STATS") == 8
    assert abi.define("NPB_VERSION") == 154
    for words in ("c = clipped ? 0.0 : -(adv * r)", "every comparison strict", "dmean[a] = (float)(((c * d[a]) / std[a]) / count)",
                  "added in ascending\n * chain order onto 0.0 and narrowed once", "grad(log_std[a]) = (float)(sum dls[a] - ent_coef)",
                  "max_grad_norm / (norm + 1e-6)", "theta' = theta - step_size * (m' / (sqrt(v') / root + eps))", "is SKIPPED",
                  "v_mfma_f32_32x32x2_f32), a workgroup a chain, no atomics", "nuclear_sim_amd/ppo.py"):
        assert words in text, words


def test_library_exports_and_binding_declares_them():
    from nuclear_sim_amd import ppo
    abi.check_entry_points(ENTRY_POINTS, [("npb_policy_grad", None, None, None), ("npb_policy_adam", None, 1e-3, 0.9, 0.999, 1e-5, None),
                                          ("npb_policy_update", None, None, 1e-3, 0.9, 0.999, 1e-5, None), ("npb_policy_get_grad", None, None, None),
                                          ("npb_policy_get_stats", None, None, None), ("npb_policy_get_theta", None, None, None),
                                          ("npb_policy_optimizer_get_state", None, None, None, None, None),
                                          ("npb_policy_optimizer_set_state", None, None, None, 0, None)])
    assert _lib.PPO_STATS == len(ppo.STATS) == 8


def test_the_binding_lays_the_descriptor_out_as_the_compiler_does():
    structs = {"npb_ppo_desc_t": _lib.NpbPpoDesc}
    got, values = abi.probe(structs, ["NPB_PPO_STATS"])
    assert got == abi.layout(structs) and values == [_lib.PPO_STATS]


def _desc(**members):
    """a valid descriptor: 300 rows of double obs, float act and float adv, every output, chains of 64"""
    d = _lib.NpbPpoDesc()
    d.obs, d.obs_type, d.act, d.act_type, d.logp_old, d.adv, d.ret, d.adv_type, d.count = A8, 1, A8 + 8, 0, A8 + 16, A8 + 24, A8 + 32, 0, 300
    d.logp_new, d.value_new, d.ratio = A8 + 40, A8 + 44, A8 + 48
    d.clip, d.vf_coef, d.ent_coef, d.max_grad_norm, d.rows_per_chain, d.max_blocks = 0.2, 0.5, 0.01, 0.5, 64, 0
    for name, value in members.items():
        setattr(d, name, value)
    return d


def _why(d, cells=CELLS, axes=AXES):
    return abi.why(abi.library().npb_ppo_check, ctypes.byref(d), cells, axes)


def test_the_check_accepts_valid_descriptors():
    assert _why(_desc()) is None
    for members in (dict(logp_new=None, value_new=None, ratio=None), dict(count=1), dict(rows_per_chain=32), dict(rows_per_chain=4096), dict(max_grad_norm=0.0),
                    dict(ent_coef=-0.5, vf_coef=0.0), dict(max_blocks=7), dict(obs_type=0, act_type=1, adv_type=1), dict(clip=0.999), dict(clip=1e-9)):
        assert _why(_desc(**members)) is None, members
    assert _why(_desc(), cells=256, axes=8) is None and _why(_desc(), cells=1, axes=1) is None


REFUSALS = [
    ("NULL obs", dict(obs=None), {}, "obs is NULL"),
    ("NULL act", dict(act=None), {}, "act is NULL"),
    ("NULL logp_old", dict(logp_old=None), {}, "logp_old is NULL"),
    ("NULL adv", dict(adv=None), {}, "adv is NULL"),
    ("NULL ret", dict(ret=None), {}, "ret is NULL"),
    ("obs type", dict(obs_type=2), {}, "an unknown obs type"),
    ("act type", dict(act_type=-1), {}, "an unknown act type"),
    ("adv type", dict(adv_type=2), {}, "an unknown adv type"),
    ("no rows", dict(count=0), {}, "count must be >= 1"),
    ("negative rows", dict(count=-5), {}, "count must be >= 1"),
    ("chains of 0", dict(rows_per_chain=0), {}, "rows_per_chain must be a positive multiple of 32"),
    ("chains of 48", dict(rows_per_chain=48), {}, "rows_per_chain must be a positive multiple of 32"),
    ("negative chains", dict(rows_per_chain=-32), {}, "rows_per_chain must be a positive multiple of 32"),
    ("clip 0", dict(clip=0.0), {}, "clip must lie inside (0, 1)"),
    ("clip 1", dict(clip=1.0), {}, "clip must lie inside (0, 1)"),
    ("clip NaN", dict(clip=float("nan")), {}, "clip must lie inside (0, 1)"),
    ("vf_coef infinite", dict(vf_coef=float("inf")), {}, "vf_coef and ent_coef must be finite"),
    ("ent_coef NaN", dict(ent_coef=float("nan")), {}, "vf_coef and ent_coef must be finite"),
    ("negative max_grad_norm", dict(max_grad_norm=-1.0), {}, "max_grad_norm must be finite and >= 0"),
    ("infinite max_grad_norm", dict(max_grad_norm=float("inf")), {}, "max_grad_norm must be finite and >= 0"),
    ("negative max_blocks", dict(max_blocks=-1), {}, "max_blocks must be >= 0"),
    ("misaligned double obs", dict(obs=A8 + 4), {}, "a misaligned obs, act, logp_old, adv or ret"),
    ("misaligned act", dict(act=A8 + 2), {}, "a misaligned obs, act, logp_old, adv or ret"),
    ("misaligned double ret", dict(adv_type=1, ret=A8 + 36), {}, "a misaligned obs, act, logp_old, adv or ret"),
    ("misaligned ratio", dict(ratio=A8 + 44), {}, "a misaligned logp_new, value_new (4-byte aligned) or ratio (8-byte aligned)"),
    ("misaligned logp_new", dict(logp_new=A8 + 41), {}, "a misaligned logp_new, value_new (4-byte aligned) or ratio (8-byte aligned)"),
    ("no cells", {}, {"cells": 0}, "1 .. NPB_FEATURES_CELLS_MAX (256) cells"),
    ("too many axes", {}, {"axes": 9}, "1 .. NPB_CONTROLS_AXES_MAX (8)"),
]


@pytest.mark.parametrize("what, members, kw, reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_check_names_every_refusal(what, members, kw, reason):
    why = _why(_desc(**members), **kw)
    assert why is not None and why.startswith("npb_policy_grad: ") and reason in why, (what, why)


def test_a_null_descriptor_is_refused_by_name():
    assert abi.library().npb_ppo_check(None, CELLS, AXES).decode() == "npb_policy_grad: a NULL descriptor"
