"""CPU: truncated segments (npb_policy_core_segments and its companions) are declared by include/npb.h, which says what a segment is and
what the kernel does differently; exported by libnpb.so and bound through the one table of signatures; the binding lays npb_ppo_segments_t
out as a C compiler does; the library's own checks, which need no handle and read no device memory, accept valid arguments and name every
refusal the header lists.  No compute calls.  NPB_VERSION stays where it was: the entry points are detected by name."""
import ctypes

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib, rollout

ENTRY_POINTS = ("npb_policy_core_segments", "npb_policy_core_segments_check", "npb_rollout_minibatch_segments", "npb_minibatch_segments_check",
                "npb_ppo_segments_check", "npb_policy_grad_segments", "npb_policy_update_segments", "npb_policy_shard_sums_segments", "npb_policy_segment_starts")
A16 = 0x7000      # "device addresses" the checks only look at: never dereferenced
CELLS, AXES, EXTRAS, N, T = 15, 3, 2, 70, 6


def test_header_declares_the_entry_points_and_says_what_a_segment_is():
    """Fails without the feature: the header declares none of them"""
    text = abi.header_text()
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_VERSION") == 154
    for words in ("TRUNCATED SEGMENTS", "g = c * n_plants + p", "starts[0] equals first", "the carry out of local slot 0 is dropped", "no word at row c * every - 1 is read",
                  "out[s][j] = src[c * every +", "row 0 is left alone", "Not here: ragged last segments", "burn-in slots and overlapping segments",
                  "per-slot storage of every state", "a sequence is differentiated whole"):
        assert words in text, words
    assert "Truncated segments are not here" not in text and "Not here: truncated segments" not in text      # the two lines this makes untrue
    assert abi.declared()["npb_policy_update_segments"] == ("int", ["NpbHandle *", "const npb_ppo_desc_t *", "const npb_ppo_more_t *", "const npb_ppo_seq_t *",
                                                                    "const npb_ppo_segments_t *", "double", "double", "double", "double", "void *"])


def test_library_exports_and_binding_declares_them():
    abi.check_entry_points(ENTRY_POINTS, [("npb_policy_core_segments", None, 2, None, 3), ("npb_rollout_minibatch_segments", None, None, 2, None),
                                          ("npb_policy_grad_segments", None, None, None, None, None, None),
                                          ("npb_policy_update_segments", None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-5, None),
                                          ("npb_policy_shard_sums_segments", None, None, None, None, None, 1, None, None),
                                          ("npb_policy_segment_starts", None, 2, None)])
    table = dict(_lib.ENTRY_POINTS)["npb_policy_core_segments"]
    assert set(table) == set(ENTRY_POINTS)      # one group, detected by name
    for name in ENTRY_POINTS:      # the one table's signatures have the header's arity
        assert len(table[name][1]) == len(abi.declared()[name][1]), name


def test_the_binding_lays_the_descriptor_out_as_the_compiler_does():
    structs = {"npb_ppo_segments_t": _lib.NpbPpoSegments, "npb_ppo_seq_t": _lib.NpbPpoSeq}
    got, values = abi.probe(structs, ["NPB_MINIBATCH_SEGMENT"])
    assert got == abi.layout(structs) and values == [_lib.MINIBATCH_UNITS["segment"]] == [rollout.UNITS["segment"]] == [2]


# ---- npb_policy_core_segments_check(every, starts, rows, horizon, core_width)
def _core_why(every=2, starts=A16, rows=3, horizon=T, width=5):
    return abi.why(abi.library().npb_policy_core_segments_check, every, starts, rows, horizon, width)


def test_the_stored_states_check():
    for kw in (dict(), dict(every=1, rows=6), dict(every=6, rows=1), dict(every=4, rows=2), dict(rows=9), dict(every=0, starts=None, rows=0),
               dict(every=0, horizon=0, width=0)):
        assert _core_why(**kw) is None, kw
    for kw, reason in ((dict(width=0), "npb_policy_core_segments: the policy has no core"), (dict(horizon=0), "npb_policy_core_segments: no rollout set"),
                       (dict(every=-1), "npb_policy_core_segments: every must be 0 (off) or 1 .. the rollout's horizon"),
                       (dict(every=7, rows=1), "npb_policy_core_segments: every must be 0 (off) or 1 .. the rollout's horizon"),
                       (dict(rows=2), "npb_policy_core_segments: too few rows"), (dict(every=4, rows=1), "npb_policy_core_segments: too few rows"),
                       (dict(starts=None), "npb_policy_core_segments: a NULL or misaligned starts"),
                       (dict(starts=A16 + 2), "npb_policy_core_segments: a NULL or misaligned starts")):
        got = _core_why(**kw)
        assert got is not None and got.startswith(reason), (kw, got)


# ---- npb_minibatch_segments_check(desc, every, n_plants, t, features_cells, n_axes, n_extras)
class _Mini:
    """a valid descriptor: segments 10 .. 74 of the 3 x 70 that 6 slots make with every = 2, float32 advantages normalised by moments"""

    def __init__(self):
        self.d = d = _lib.NpbMinibatchDesc()
        d.unit, d.type, d.first, d.count, d.eps, d.max_blocks = 2, 0, 10, 64, 1e-8, 0
        d.keys[:] = [1, 2, 3, 4, 5, 6]
        d.adv, d.ret, d.moments = A16 + 4, A16 + 8, A16 + 24
        d.index, d.obs, d.act, d.extra, d.adv_out, d.ret_out = A16 + 4, A16 + 16, A16 + 32, A16 + 48, A16 + 12, A16 + 20


def _mini_why(D, every=2, n=N, t=T):
    return abi.why(abi.library().npb_minibatch_segments_check, None if D is None else ctypes.byref(D.d), every, n, t, CELLS, AXES, EXTRAS)


MINI_REFUSALS = [
    ("a NULL descriptor", None, {}, "npb_rollout_minibatch: a NULL descriptor"),
    ("another unit", abi.set_members(unit=1), {}, "npb_rollout_minibatch_segments: the unit must be NPB_MINIBATCH_SEGMENT"),
    ("every < 1", None, dict(every=0), "npb_rollout_minibatch_segments: every must be >= 1"),
    ("every > t", None, dict(every=7), "npb_rollout_minibatch_segments: every is beyond the recorded slots"),
    ("t % every", None, dict(every=4), "npb_rollout_minibatch_segments: t is not a multiple of every"),
    ("nothing recorded", None, dict(t=0), "npb_rollout_minibatch: nothing recorded yet"),
    ("n_plants", None, dict(n=0), "npb_rollout_minibatch: n_plants must be >= 1"),
    ("the window ends beyond the segments", abi.set_members(first=147), {}, "npb_rollout_minibatch: entries [first, first + count) must lie inside"),
    ("count", abi.set_members(count=0), {}, "npb_rollout_minibatch: count must be >= 1"),
    ("index", abi.set_members(index=None), {}, "npb_rollout_minibatch: index is NULL"),
    ("type", abi.set_members(type=2), {}, "npb_rollout_minibatch: an unknown type"),
    ("moments without adv_out", abi.set_members(adv_out=None), {}, "npb_rollout_minibatch: moments are set"),
    ("misaligned obs", abi.set_members(obs=A16 + 8), {}, "npb_rollout_minibatch: a misaligned obs, act or extra output"),
    ("eps", abi.set_members(eps=-1.0), {}, "npb_rollout_minibatch: eps must be >= 0"),
]


def test_the_minibatch_check_accepts_valid_segment_minibatches():
    assert _mini_why(_Mini()) is None
    for change, kw in ((abi.set_members(first=0, count=3 * N), {}), (abi.set_members(first=146), {}), (abi.set_members(first=0, count=N), dict(every=6)),
                       (abi.set_members(first=6 * N - 64), dict(every=1)), (abi.set_members(moments=None), {}), (abi.set_members(first=0, count=2 * N), dict(every=3))):
        D = _Mini(); change(D)
        assert _mini_why(D, **kw) is None, kw
    # npb_rollout_minibatch itself has no room for every: it refuses the unit
    assert abi.why(abi.library().npb_minibatch_check, ctypes.byref(_Mini().d), N, T, CELLS, AXES, EXTRAS).startswith("npb_rollout_minibatch: an unknown unit")


@pytest.mark.parametrize("what, change, kw, reason", MINI_REFUSALS, ids=[r[0] for r in MINI_REFUSALS])
def test_the_minibatch_check_names_every_refusal(what, change, kw, reason):
    D = None if what == "a NULL descriptor" else _Mini()
    if change is not None:
        change(D)
    got = _mini_why(D, **kw)
    assert got is not None and got.startswith(reason), (what, got)


# ---- npb_ppo_segments_check(desc, seq, seg, features_cells, n_axes)
class _Seg:
    """a valid triple: 33 segments of 2 slots out of the 3 x 70 of a rollout of 70 plants, every tensor set"""

    def __init__(self):
        self.d = s = _lib.NpbPpoSeq()
        s.t, s.plants, s.index, s.n_plants, s.episode, s.ended, s.first, s.hidden = 2, 33, A16, 70, A16 + 0x100, A16 + 0x201, A16 + 0x300, A16 + 0x400
        self.desc = d = _lib.NpbPpoDesc()
        d.obs, d.act, d.logp_old, d.adv, d.ret, d.count = A16, A16 + 8, A16 + 16, A16 + 24, A16 + 32, 66
        d.clip, d.vf_coef, d.max_grad_norm, d.rows_per_chain = 0.2, 0.5, 0.5, 32
        self.seg = g = _lib.NpbPpoSegments()
        g.every, g.chunks = 2, 3


def _seg_why(D, seg=True):
    return abi.why(abi.library().npb_ppo_segments_check, ctypes.byref(D.desc), ctypes.byref(D.d), ctypes.byref(D.seg) if seg else None, CELLS, AXES)


def _of(member, **values):
    def change(D):
        for name, value in values.items():
            setattr(getattr(D, member), name, value)
    return change


SEG_REFUSALS = [
    ("what npb_ppo_seq_check refuses", _of("d", first=None), "npb_policy_grad_seq: first is NULL"),
    ("what npb_ppo_check refuses", _of("desc", rows_per_chain=48), "npb_policy_grad: rows_per_chain must be a positive multiple of 32"),
    ("every", abi.both(_of("seg", every=0)), "npb_policy_grad_segments: every must be >= 1"),
    ("chunks", _of("seg", chunks=0), "npb_policy_grad_segments: chunks must be >= 1"),
    ("seq->t is not every", _of("seg", every=3), "npb_policy_grad_segments: seq->t must be every"),
    ("beyond int32", _of("seg", chunks=2 ** 31 // 140 + 1), "npb_policy_grad_segments: chunks * every * n_plants is beyond 2^31 - 1"),
]


def test_the_segments_check_accepts_valid_descriptors():
    assert _seg_why(_Seg()) is None
    for change in (_of("d", index=None), _of("d", hidden=None), _of("seg", chunks=1), abi.both(_of("d", t=6, plants=11), _of("seg", every=6, chunks=1)),
                   abi.both(_of("d", t=1, plants=66), _of("seg", every=1, chunks=6))):
        D = _Seg(); change(D)
        assert _seg_why(D) is None
    assert _seg_why(_Seg(), seg=False).startswith("npb_policy_grad_segments: a NULL segments descriptor")


@pytest.mark.parametrize("what, change, reason", SEG_REFUSALS, ids=[r[0] for r in SEG_REFUSALS])
def test_the_segments_check_names_every_refusal(what, change, reason):
    D = _Seg(); change(D)
    got = _seg_why(D)
    assert got is not None and got.startswith(reason), (what, got)
