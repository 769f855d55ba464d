"""CPU: the options of the policy's training step (npb_policy_grad_more and its companions: value-loss clipping, the target_kl gate, more
statistics) are declared by include/npb.h, exported by libnpb.so and bound; the binding lays npb_ppo_more_t out as a C compiler does (a
small compiled probe prints sizeof and every offsetof); the library's own check, which needs no handle and reads no device memory, accepts
valid options and names every refusal the header lists; what the existing suites pin of the ABI is untouched.  No compute calls."""
import ctypes

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib, ppo, ppo_abi

ENTRY_POINTS = ("npb_ppo_more_check", "npb_policy_grad_more", "npb_policy_update_more", "npb_policy_train_begin", "npb_policy_train_end",
                "npb_policy_get_stats_more")
A8 = 0x7000       # a "device address" the check only looks at: never dereferenced


def test_header_declares_the_entry_points_and_states_the_contract():
    """Fails without the feature: the header declares none of them"""
    text = abi.header_text()
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_PPO_STATS_MORE") == 4 == len(ppo.STATS_MORE) == _lib.PPO_STATS_MORE == ppo_abi.PPO_STATS_MORE
    assert abi.define("NPB_PPO_STATS") == 8 == len(ppo.STATS) == _lib.PPO_STATS and abi.define("NPB_VERSION") == 154
    for words in ("dc = dvo < -clip_vf ? -clip_vf : (dvo > clip_vf ? clip_vf : dvo)", "use = sqc > sq (strict)", "out = dvo < -clip_vf or dvo > clip_vf (strict)",
                  "dv = (float)((vf_coef * (use ? (out ? 0.0 : diffc) : diff)) / count)", "vr = S_rr / m - (S_r / m) * (S_r / m)",
                  "explained_variance = 1.0 - vd / vr", "stopped' = stopped or (approx_kl > kl_limit)", "a NaN approx_kl does not stop",
                  "THE ONE READ-BACK", "step = step0 + applied", "step counts applied updates only", "NPB_VERSION stays 154"):
        assert words in text, words
    # the two options left the list of what is not here
    not_here = text[text.index("Not here: a shared trunk"):]
    not_here = not_here[:not_here.index("\n *\n")]
    assert "value-loss clipping" not in not_here and "target_kl" not in not_here


def test_library_exports_and_binding_declares_them():
    abi.check_entry_points(ENTRY_POINTS, [("npb_policy_grad_more", None, None, None, None), ("npb_policy_update_more", None, None, None, 1e-3, 0.9, 0.999, 1e-5, None),
                                          ("npb_policy_train_begin", None, None), ("npb_policy_train_end", None, None, None),
                                          ("npb_policy_get_stats_more", None, None, None)])
    group = dict(_lib.ENTRY_POINTS)["npb_policy_grad_more"]
    assert set(group) == set(ENTRY_POINTS)      # one group, detected by name


def test_the_binding_lays_the_options_out_as_the_compiler_does():
    assert _lib.NpbPpoMore is ppo_abi.NpbPpoMore
    structs = {"npb_ppo_more_t": _lib.NpbPpoMore, "npb_ppo_desc_t": _lib.NpbPpoDesc}
    got, values = abi.probe(structs, ["NPB_PPO_STATS_MORE", "NPB_PPO_STATS", "NPB_VERSION"])
    assert got == abi.layout(structs) and values == [4, 8, 154]
    assert [f[0] for f in _lib.NpbPpoMore._fields_] == ["value_old", "clip_vf", "kl_limit"]


def _more(**members):
    m = _lib.NpbPpoMore()
    m.value_old, m.clip_vf, m.kl_limit = A8, 0.2, 0.03
    for name, value in members.items():
        setattr(m, name, value)
    return m


def _why(m, count=300):
    return abi.why(abi.library().npb_ppo_more_check, None if m is None else ctypes.byref(m), count)


def test_the_check_accepts_valid_options():
    assert _why(None) is None and _why(_more()) is None
    for members in (dict(clip_vf=0.0, value_old=None), dict(clip_vf=0.0, kl_limit=0.0, value_old=None), dict(kl_limit=0.0), dict(clip_vf=1e-9), dict(clip_vf=1e9),
                    dict(kl_limit=1e-12), dict(value_old=A8 + 4)):
        assert _why(_more(**members)) is None, members
    assert _why(_more(), count=1) is None


REFUSALS = [
    ("negative clip_vf", dict(clip_vf=-0.1), "clip_vf must be finite and >= 0"),
    ("infinite clip_vf", dict(clip_vf=float("inf")), "clip_vf must be finite and >= 0"),
    ("NaN clip_vf", dict(clip_vf=float("nan")), "clip_vf must be finite and >= 0"),
    ("negative kl_limit", dict(kl_limit=-1e-3), "kl_limit must be finite and >= 0"),
    ("infinite kl_limit", dict(kl_limit=float("inf")), "kl_limit must be finite and >= 0"),
    ("NaN kl_limit", dict(kl_limit=float("nan")), "kl_limit must be finite and >= 0"),
    ("clip_vf without value_old", dict(value_old=None), "clip_vf > 0 and value_old is NULL"),
    ("misaligned value_old", dict(value_old=A8 + 2), "a misaligned value_old"),
    ("misaligned value_old, clipping off", dict(value_old=A8 + 1, clip_vf=0.0), "a misaligned value_old"),
]


@pytest.mark.parametrize("what, members, reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_check_names_every_refusal(what, members, reason):
    why = _why(_more(**members))
    assert why is not None and why.startswith("npb_policy_grad_more: ") and reason in why, (what, why)
    # and the header lists it
    text = " ".join(abi.header_text().split())
    listed = text[text.index("npb_ppo_more_check(more, count): the host-only validator"):]
    listed = listed[:listed.index("npb_policy_grad_more(h, desc, more, stream)")]
    for words in ("a clip_vf or kl_limit that * is negative or not finite", "clip_vf > 0 with value_old NULL", "a misaligned value_old"):
        assert words in listed, words
