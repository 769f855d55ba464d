"""CPU: the pinned moments, the keyed permutation and the minibatch gather (npb_rollout_moments, npb_rollout_permutation,
npb_rollout_minibatch, npb_minibatch_check) are declared by include/npb.h, exported by libnpb.so and bound; the binding lays both
descriptors out as a C compiler does (a small compiled probe prints sizeof and every offsetof); the library's own check, which needs no
handle and reads no device memory, accepts a valid descriptor and names every refusal the header lists.  No compute calls.

NPB_VERSION stays where the suites of the entry-point groups before this one pin it: the new entry points are detected by name."""
import ctypes

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib

ENTRY_POINTS = ("npb_rollout_moments", "npb_rollout_permutation", "npb_rollout_minibatch", "npb_minibatch_check")
STRUCTS = {"npb_moments_desc_t": _lib.NpbMomentsDesc, "npb_minibatch_desc_t": _lib.NpbMinibatchDesc}
A16 = 0x7000       # "device addresses" the check only looks at: never dereferenced
N, T, CELLS, AXES, EXTRAS = 70, 5, 8, 3, 2


def test_header_declares_the_entry_points_and_the_rules_of_the_road():
    text = abi.header_text()
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_MINIBATCH_ROUNDS") == 6
    assert abi.define("NPB_VERSION") == 154
    for words in ("The order of every addition is pinned", "pad it with +0.0 to a multiple of 256", "the product rounded before the sum",
                  "the sum is not restated as a scan or a different tree", "A NaN or an infinity propagates", "no table, no sort, no memory",
                  "cycle walking", "murmur3's 32-bit finaliser", "one IEEE division in double", "round-to-nearest-even",
                  "the result does not depend on it", "where the reduction order is pinned: npb_rollout_moments, npb_rollout_minibatch", "sampling with replacement",
                  "a checkpoint of a half-drained epoch", "gathering final_obs"):
        assert words in text, words


def test_library_exports_and_binding_declares_them():
    abi.check_entry_points(ENTRY_POINTS, [("npb_rollout_moments", None, None, None), ("npb_rollout_minibatch", None, None, None),
                                          ("npb_rollout_permutation", None, 10, None, 0, 10, None, None)])


def test_the_binding_lays_the_descriptors_out_as_the_compiler_does():
    from nuclear_sim_amd import rollout
    got, values = abi.probe(STRUCTS, ["NPB_MINIBATCH_TRANSITION", "NPB_MINIBATCH_PLANT", "NPB_MINIBATCH_ROUNDS"])
    U = _lib.MINIBATCH_UNITS
    assert got == abi.layout(STRUCTS) and values == [U["transition"], U["plant"], _lib.MINIBATCH_ROUNDS]
    assert U == rollout.UNITS and _lib.MINIBATCH_ROUNDS == rollout.ROUNDS == 6


class _Desc:
    """a valid descriptor: transitions 10 .. 74 of 5 x 70, float32 advantages normalised by moments, every output given"""

    def __init__(self):
        self.d = d = _lib.NpbMinibatchDesc()
        d.unit, d.type, d.first, d.count, d.eps, d.max_blocks = 0, 0, 10, 64, 1e-8, 0
        d.keys[:] = [1, 2, 3, 4, 5, 6]
        d.adv, d.ret, d.moments = A16 + 4, A16 + 8, A16 + 24
        d.index, d.obs, d.act, d.extra, d.adv_out, d.ret_out = A16 + 4, A16 + 16, A16 + 32, A16 + 48, A16 + 12, A16 + 20


def _why(D, n=N, t=T, cells=CELLS, axes=AXES, extras=EXTRAS):
    return abi.why(abi.library().npb_minibatch_check, None if D is None else ctypes.byref(D.d), n, t, cells, axes, extras)


_set = abi.set_members


def test_the_check_accepts_valid_minibatches():
    assert _why(_Desc()) is None
    for change, kw in ((_set(unit=1, first=6, count=64), {}), (_set(first=0, count=N * T), {}), (_set(first=N * T - 1, count=1), {}),
                       (_set(type=1, adv=A16 + 8, adv_out=A16 + 16, ret_out=A16 + 24), {}), (_set(moments=None), {}), (_set(eps=0.0), {}),
                       (_set(obs=None, act=None, extra=None, adv_out=None, ret_out=None, moments=None, adv=None, ret=None), {}),
                       (_set(act=None), {"axes": 0}), (_set(extra=None), {"extras": 0}), (_set(max_blocks=3), {}),
                       (_set(first=2 ** 31 - 2, count=1), {"n": 2 ** 31 - 1, "t": 1})):
        D = _Desc(); change(D)
        assert _why(D, **kw) is None, kw


REFUSALS = [
    ("n_plants", _set(), {"n": 0}, "n_plants must be >= 1"),
    ("no features", _set(), {"cells": 0}, "must have cells"),
    ("nothing recorded", _set(), {"t": 0}, "nothing recorded yet (t == 0)"),
    ("unknown unit", _set(unit=2), {}, "an unknown unit"),
    ("negative unit", _set(unit=-1), {}, "an unknown unit"),
    ("unknown type", _set(type=2), {}, "an unknown type"),
    ("N beyond int32", _set(), {"n": 2 ** 30, "t": 2}, "beyond 2^31 - 1"),
    ("no count", _set(count=0), {}, "count must be >= 1"),
    ("negative first", _set(first=-1), {}, "must lie inside [0, N)"),
    ("past the end", _set(first=N * T - 63), {}, "must lie inside [0, N)"),
    ("past the plants", _set(unit=1, first=7), {}, "must lie inside [0, N)"),
    ("NULL index", _set(index=None), {}, "index is NULL"),
    ("act without axes", _set(), {"axes": 0}, "an act output without axes"),
    ("extra without extras", _set(), {"extras": 0}, "an extra output without extras"),
    ("adv_out without adv", _set(adv=None), {}, "adv_out without adv"),
    ("ret_out without ret", _set(ret=None), {}, "ret_out without ret"),
    ("moments without adv_out", _set(adv_out=None), {}, "moments are set and adv_out"),
    ("negative eps", _set(eps=-1e-9), {}, "eps must be >= 0"),
    ("NaN eps", _set(eps=float("nan")), {}, "eps must be >= 0"),
    ("negative max_blocks", _set(max_blocks=-1), {}, "max_blocks must be >= 0"),
    ("misaligned obs", _set(obs=A16 + 8), {}, "a misaligned obs, act or extra output"),
    ("misaligned act", _set(act=A16 + 4), {}, "a misaligned obs, act or extra output"),
    ("misaligned extra", _set(extra=A16 + 12), {}, "a misaligned obs, act or extra output"),
    ("misaligned moments", _set(moments=A16 + 4), {}, "misaligned moments"),
    ("misaligned adv", _set(adv=A16 + 2), {}, "misaligned adv, ret, adv_out or ret_out"),
    ("misaligned double ret", _set(type=1, adv=A16, ret=A16 + 4, adv_out=A16 + 8, ret_out=A16 + 16), {}, "misaligned adv, ret, adv_out or ret_out"),
    ("misaligned adv_out", _set(adv_out=A16 + 1), {}, "misaligned adv, ret, adv_out or ret_out"),
    ("misaligned index", _set(index=A16 + 2), {}, "a misaligned index"),
]


@pytest.mark.parametrize("what, change, kw, reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_check_names_every_refusal(what, change, kw, reason):
    abi.check_refusal(_Desc, _why, "npb_rollout_minibatch: ", what, change, reason, kw)


def test_a_null_descriptor_is_refused():
    assert "a NULL descriptor" in _why(None)
