"""CPU: training through time (npb_policy_grad_seq and its companions) is declared by include/npb.h, which states the backward pass through
the cell; exported by libnpb.so and bound; the binding lays npb_ppo_seq_t out as a C compiler does; the library's own check, which needs no
handle and reads no device memory, accepts a valid descriptor and names every refusal the header lists.  No compute calls.  NPB_VERSION
stays where it was: the entry points are detected by name."""
import ctypes

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

ENTRY_POINTS = ("npb_ppo_seq_check", "npb_policy_grad_seq", "npb_policy_update_seq", "npb_policy_shard_sums_seq")
A4 = 0x7000       # "device addresses" the check only looks at: never dereferenced
CELLS, AXES = 15, 3


def test_header_declares_the_entry_points_and_states_the_backward_pass():
    text = abi.header_text()
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_VERSION") == 154
    for words in ("dh' = (carry + back(delta_actor_layer0, W_actor0)) + back(delta_critic_layer0, W_critic0)", "dn = dh' * (1.0f - z);  dz = dh' * u;  direct = dh' * z",
                  "T' = 1.0f - n * n", "S' = s * (1.0f - s)", "else d * 0.25f", "dghn = dan * r;  dr = dan * gh_n", "delta_i = [dar | daz | dan];  delta_h = [dar | daz | dghn]",
                  "carry_out = direct + back(delta_h, W_hh)", "within a tile s DESCENDING", "Training through time is not built into the row-wise entry points",
                  "the state the COLLECTING parameters produced", "a sequence is differentiated whole"):
        assert words in text, words
    assert "training the core on the device" not in text      # the core's "Not here" no longer lists it
    assert abi.declared()["npb_policy_update_seq"] == ("int", ["NpbHandle *", "const npb_ppo_desc_t *", "const npb_ppo_more_t *", "const npb_ppo_seq_t *", "double",
                                                               "double", "double", "double", "void *"])


def test_library_exports_and_binding_declares_them():
    abi.check_entry_points(ENTRY_POINTS, [("npb_policy_grad_seq", None, None, None, None, None),
                                          ("npb_policy_update_seq", None, None, None, None, 1e-3, 0.9, 0.999, 1e-5, None),
                                          ("npb_policy_shard_sums_seq", None, None, None, None, 1, None, None)])
    table = dict(_lib.ENTRY_POINTS)["npb_policy_grad_seq"]
    assert set(table) == set(ENTRY_POINTS)
    for name in ENTRY_POINTS:      # the one table's signatures have the header's arity
        assert len(table[name][1]) == len(abi.declared()[name][1]), name


def test_the_binding_lays_the_descriptor_out_as_the_compiler_does():
    structs = {"npb_ppo_seq_t": _lib.NpbPpoSeq, "npb_ppo_desc_t": _lib.NpbPpoDesc}
    got, _ = abi.probe(structs)
    assert got == abi.layout(structs)


class _Seq:
    """a valid pair: 5 slots of 33 sequences out of a rollout of 70 plants, every tensor set"""

    def __init__(self):
        self.d = s = _lib.NpbPpoSeq()
        s.t, s.plants, s.index, s.n_plants, s.episode, s.ended, s.first, s.hidden = 5, 33, A4, 70, A4 + 0x100, A4 + 0x201, A4 + 0x300, A4 + 0x400
        self.desc = d = _lib.NpbPpoDesc()
        d.obs, d.act, d.logp_old, d.adv, d.ret, d.count = A4, A4 + 8, A4 + 16, A4 + 24, A4 + 32, 165
        d.clip, d.vf_coef, d.max_grad_norm, d.rows_per_chain = 0.2, 0.5, 0.5, 32


def _why(D, n=None, cells=CELLS):
    return abi.why(abi.library().npb_ppo_seq_check, ctypes.byref(D.desc), ctypes.byref(D.d), cells, AXES)


def _desc(**members):
    def change(D):
        for name, value in members.items():
            setattr(D.desc, name, value)
    return change


def test_the_check_accepts_valid_descriptors():
    L = abi.library()
    assert _why(_Seq()) is None
    for change in (abi.set_members(index=None), abi.set_members(hidden=None), abi.set_members(ended=A4 + 3), abi.both(abi.set_members(t=1, plants=1), _desc(count=1)),
                   abi.both(abi.set_members(plants=64, n_plants=64), _desc(count=320, rows_per_chain=64))):
        D = _Seq(); change(D)
        assert _why(D) is None
    assert L.npb_ppo_seq_check(ctypes.byref(_Seq().desc), None, CELLS, AXES).startswith(b"npb_policy_grad_seq: a NULL sequence descriptor")


REFUSALS = [
    ("a NULL desc is npb_ppo_check's", None, "npb_policy_grad: a NULL descriptor"),
    ("what npb_ppo_check refuses", _desc(rows_per_chain=48), "npb_policy_grad: rows_per_chain must be a positive multiple of 32"),
    ("t", abi.set_members(t=0), "npb_policy_grad_seq: t must be >= 1"),
    ("plants", abi.set_members(plants=0), "npb_policy_grad_seq: plants must be >= 1"),
    ("count", _desc(count=164), "npb_policy_grad_seq: desc->count must be t * plants"),
    ("n_plants", abi.set_members(n_plants=0), "npb_policy_grad_seq: n_plants must be >= 1"),
    ("beyond int32", abi.set_members(n_plants=2 ** 31 // 5 + 1), "npb_policy_grad_seq: t * n_plants is beyond 2^31 - 1"),
    ("NULL episode", abi.set_members(episode=None), "npb_policy_grad_seq: episode is NULL"),
    ("NULL ended", abi.set_members(ended=None), "npb_policy_grad_seq: ended is NULL"),
    ("NULL first", abi.set_members(first=None), "npb_policy_grad_seq: first is NULL"),
    ("misaligned index", abi.set_members(index=A4 + 2), "npb_policy_grad_seq: a misaligned index, episode, first or hidden"),
    ("misaligned episode", abi.set_members(episode=A4 + 1), "npb_policy_grad_seq: a misaligned index, episode, first or hidden"),
    ("misaligned first", abi.set_members(first=A4 + 3), "npb_policy_grad_seq: a misaligned index, episode, first or hidden"),
    ("misaligned hidden", abi.set_members(hidden=A4 + 2), "npb_policy_grad_seq: a misaligned index, episode, first or hidden"),
]


@pytest.mark.parametrize("what, change, reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_check_names_every_refusal(what, change, reason):
    D = _Seq()
    if change is None:
        got = abi.why(abi.library().npb_ppo_seq_check, None, ctypes.byref(D.d), CELLS, AXES)
    else:
        change(D)
        got = _why(D)
    assert got is not None and got.startswith(reason), (what, got)
