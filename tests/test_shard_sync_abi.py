"""CPU: one normaliser and one set of advantage moments across shards (npb_normalizer_shard_delta, npb_normalizer_apply_shards,
npb_rollout_moments_part, npb_rollout_moments_combine and their companions) are declared by include/npb.h, which states their formulas,
exported by libnpb.so and bound in one group; the library's own checks, which need no handle and read no device memory, accept valid
arguments and name every refusal the header lists; what the existing suites pin of the ABI is untouched.  No compute calls."""
import ctypes

import pytest

import abi_support as abi
from nuclear_sim_amd import _lib, normalizer, rollout

ENTRY_POINTS = ("npb_normalizer_shard_count", "npb_normalizer_shards_check", "npb_normalizer_shard_delta", "npb_normalizer_apply_shards",
                "npb_normalizer_get_base", "npb_normalizer_set_base", "npb_moments_shards_check", "npb_rollout_moments_part",
                "npb_rollout_moments_combine")
A8 = 0x7000       # a "device address" the checks only look at: never dereferenced
TITLE = "ONE NORMALISER AND ONE SET OF ADVANTAGE MOMENTS ACROSS SHARDS"


def _section():
    text = abi.header_text()
    text = text[text.index("/* " + TITLE):]
    return " ".join(text[:text.index("*/")].split())


def test_header_declares_the_entry_points_and_states_the_formulas():
    """Fails without the feature: the header declares none of them"""
    assert set(ENTRY_POINTS) <= set(abi.declared())
    assert abi.define("NPB_VERSION") == 154
    assert abi.define("NPB_PPO_SHARDS_MAX") == 64 == _lib.PPO_SHARDS_MAX == normalizer.SHARDS_MAX == rollout.SHARDS_MAX
    text = _section()
    for words in ("NPB_VERSION * stays 154", "no new struct", "na, ma, Ma = base; N, m, M = the state; nb = N - na",
                  "nb > 0: mb = m + (m - ma) * (na / nb); d = mb - ma", "Mb = (M - Ma) - (d * d) * ((na * nb) / N), 0.0 where that is negative",
                  "else: delta = (0.0, 0.0, 0.0)", "With a zero base the delta is the state exactly",
                  "N = n + nb; d = mb - mean; mean = mean + d * (nb / N)", "M2 = (M2 + Mb) + (d * d) * ((n * nb) / N); n = N",
                  "only a shard with nb > 0 is merged", "as the state AND as the base", "stays with its shard",
                  "allowed while frozen", "W = 1 is * the identity only from a zero base",
                  "npb_set_normalizer zeroes the base; npb_normalizer_set_state leaves it alone",
                  "npb_normalizer_shard_count(h) = 3 * S", "part, a DEVICE double [2] = {count, total}", "desc->out is never written",
                  "C = 0.0; T = 0.0; for w ascending C = C + count_w; T = T + total_w", "out[0] = C, out[1] = T / C",
                  "out[2] = T / (C - ddof), out[3] = sqrt(out[2])", "npb_rollout_moments, bit for bit", "no atomics and no scratch", "24 * S bytes"):
        assert words in text, words
    # the refusals the validators make are listed
    for words in ("deltas NULL; deltas * misaligned for a double; n_shards outside 1 .. NPB_PPO_SHARDS_MAX (64)", "no normaliser set",
                  "part NULL, part misaligned for a double", "parts NULL or misaligned; n_shards outside 1 .. NPB_PPO_SHARDS_MAX (64); ddof < 0; out NULL or * misaligned",
                  "whatever npb_rollout_moments refuses a descriptor for"):
        assert words in text, words


def test_the_pinned_sentences_of_the_older_sections_are_still_there():
    whole = abi.header_text()
    flat = " ".join(whole.split())
    for words in ("synchronising shards on the device (normalizer.merge is the host answer)", "Not here: a shared trunk, learning-rate schedules",
                  "Not here: synchronising the running normaliser between shards (normalizer.merge stays the host answer); advantage moments over all * shards"):
        assert words in flat, words
    # the first "*/" behind the shards section's "Not here:" still ends the old paragraph, and the new block stands behind it
    shards = whole[whole.index("TRAINING ONE POLICY ACROSS SHARDS"):]
    not_here = shards[shards.index("Not here:"):]
    not_here = not_here[:not_here.index("*/")]
    for words in ("synchronising the running normaliser between shards", "advantage moments over all", "different numbers of updates",
                  "overlapping the exchange", "more than one device", "have the section below"):
        assert words in not_here, words
    assert TITLE not in not_here and whole.index("/* " + TITLE) > whole.index("TRAINING ONE POLICY ACROSS SHARDS")
    assert whole.index("/* " + TITLE) > whole.index("npb_policy_combine_shards(NpbHandle")
    # the normaliser's section points down to it
    norm = whole[whole.index("synchronising shards on the device (normalizer.merge is the host answer)"):]
    assert TITLE in norm[:norm.index("*/")]


def test_library_exports_and_binding_declares_them_in_one_group():
    """Fails without the feature: the library exports none of them"""
    abi.check_entry_points(ENTRY_POINTS, [("npb_normalizer_shard_delta", None, A8, None), ("npb_normalizer_apply_shards", None, A8, 2, None),
                                          ("npb_normalizer_get_base", None, None, None), ("npb_normalizer_set_base", None, None, None),
                                          ("npb_rollout_moments_part", None, None, 0, A8, None), ("npb_rollout_moments_combine", None, A8, 2, 0, 1, A8, None)])
    group = dict(_lib.ENTRY_POINTS)["npb_normalizer_apply_shards"]
    assert set(group) == set(ENTRY_POINTS)      # one group, detected by name
    assert abi.library().npb_normalizer_shard_count(None) == 0
    # no new structure: the moments calls take the existing descriptor
    assert [f[0] for f in _lib.NpbMomentsDesc._fields_] == ["src", "type", "ddof", "rows", "cols", "out"]


# ---------------------------------------------------------------------------------------------------------------- the validators
def _norm_why(deltas, n_shards):
    return abi.why(abi.library().npb_normalizer_shards_check, deltas, n_shards)


def test_the_normaliser_check_accepts_and_names_every_refusal():
    for W in (1, 2, 64):
        assert _norm_why(A8, W) is None and _norm_why(A8 + 8, W) is None
    for deltas, W, reason in ((None, 2, "deltas is NULL"), (A8 + 4, 2, "a misaligned deltas"), (A8 + 1, 2, "a misaligned deltas"),
                              (A8, 0, "n_shards must be 1 .. NPB_PPO_SHARDS_MAX (64)"), (A8, -1, "n_shards must be 1 .. NPB_PPO_SHARDS_MAX (64)"),
                              (A8, 65, "n_shards must be 1 .. NPB_PPO_SHARDS_MAX (64)")):
        why = _norm_why(deltas, W)
        assert why is not None and why.startswith("npb_normalizer_apply_shards: ") and reason in why, (deltas, W, why)


def _desc(**members):
    d = _lib.NpbMomentsDesc()
    d.src, d.type, d.ddof, d.rows, d.cols, d.out = A8, _lib.ROLLOUT_DTYPES["float32"], 0, 3, 70, A8 + 64
    for name, value in members.items():
        setattr(d, name, value)
    return d


def _part_why(d, part=A8 + 128):
    return abi.why(abi.library().npb_moments_shards_check, ctypes.byref(d), part, None, 0, 0, None)


def _combine_why(parts=A8, n_shards=3, ddof=1, out=A8 + 64):
    return abi.why(abi.library().npb_moments_shards_check, None, None, parts, n_shards, ddof, out)


def test_the_moments_check_accepts_valid_calls():
    assert _part_why(_desc()) is None
    for members in (dict(type=_lib.ROLLOUT_DTYPES["float64"]), dict(rows=1, cols=1), dict(src=A8 + 4), dict(rows=2 ** 20, cols=2 ** 31 - 1)):
        assert _part_why(_desc(**members)) is None, members
    assert _combine_why() is None
    for kw in (dict(n_shards=1), dict(n_shards=64), dict(ddof=0), dict(ddof=7), dict(parts=A8 + 8), dict(out=A8 + 8)):
        assert _combine_why(**kw) is None, kw


PART_REFUSALS = [
    ("NULL src", dict(src=None), "npb_rollout_moments: NULL src or out"),
    ("NULL out", dict(out=None), "npb_rollout_moments: NULL src or out"),
    ("unknown type", dict(type=7), "npb_rollout_moments: an unknown type"),
    ("no rows", dict(rows=0), "npb_rollout_moments: rows and cols must be >= 1"),
    ("no cols", dict(cols=0), "npb_rollout_moments: rows and cols must be >= 1"),
    ("cols beyond int32", dict(cols=2 ** 31), "npb_rollout_moments: cols beyond 2^31 - 1"),
    ("beyond 2^53", dict(rows=2 ** 40, cols=2 ** 20), "npb_rollout_moments: rows * cols beyond 2^53"),
    ("negative ddof", dict(ddof=-1), "npb_rollout_moments: ddof must be >= 0"),
    ("count <= ddof", dict(rows=1, cols=1, ddof=1), "npb_rollout_moments: rows * cols <= ddof"),
    ("misaligned src", dict(src=A8 + 2), "npb_rollout_moments: src is misaligned for its type"),
    ("misaligned double src", dict(src=A8 + 4, type=1), "npb_rollout_moments: src is misaligned for its type"),
    ("misaligned out", dict(out=A8 + 4), "npb_rollout_moments: a misaligned out"),
]


@pytest.mark.parametrize("what, members, reason", PART_REFUSALS, ids=[r[0] for r in PART_REFUSALS])
def test_the_part_is_refused_for_what_the_descriptor_is_refused_today(what, members, reason):
    why = _part_why(_desc(**members))
    assert why is not None and reason in why, (what, why)


def test_the_part_and_the_combine_name_their_own_refusals():
    assert "npb_rollout_moments_part: part is NULL" in _part_why(_desc(), None)
    assert "npb_rollout_moments_part: a misaligned part" in _part_why(_desc(), A8 + 4)
    for kw, reason in ((dict(parts=None), "parts is NULL"), (dict(parts=A8 + 4), "a misaligned parts"), (dict(n_shards=0), "n_shards must be 1 .. NPB_PPO_SHARDS_MAX (64)"),
                       (dict(n_shards=65), "n_shards must be 1 .. NPB_PPO_SHARDS_MAX (64)"), (dict(n_shards=-3), "n_shards must be 1 .. NPB_PPO_SHARDS_MAX (64)"),
                       (dict(ddof=-1), "ddof must be >= 0"), (dict(out=None), "out is NULL"), (dict(out=A8 + 4), "a misaligned out")):
        why = _combine_why(**kw)
        assert why is not None and why.startswith("npb_rollout_moments_combine: ") and reason in why, (kw, why)
