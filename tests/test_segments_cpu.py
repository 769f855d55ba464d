"""CPU: the numpy statement of truncated segments (nuclear_sim_amd.recurrent: starts, segment_words, gradient_segments, shard_sums_segments;
nuclear_sim_amd.rollout.minibatch with unit "segment").  A segment minibatch IS a sequence minibatch of length L whose plants are segments:
with one segment a plant it is ``gradient`` bit for bit; it is the right truncated gradient -- float32 against torch float64 autograd of the
same loss with the state detached at every boundary and the stored states fed as constants -- and not the whole-sequence one; the gather
and the index are brute force's; the stored states are ``replay``'s at the boundaries.  No device.

The shape: t = 6 slots, 40 plants (a ragged second tile), K * C = 6, H = 5, actor (7,), critic (9, 6), A = 3."""
import numpy as np
import pytest

from nuclear_sim_amd import ppo, recurrent, rollout
from recurrent_train_support import bits, distance, statement
from segments_support import autograd_truncated, rollout_problem, segment_batch, statement_segments

T, N, CELLS, H, A, ACTOR, CRITIC = 6, 40, 6, 5, 3, (7,), (9, 6)
# tests/test_recurrent_train_cpu.py's limit for the whole-sequence statement: the linear rounding bound eps_f32 * t * (K * C + H + the widths)
# is about 7e-5 here (a segment's chains are no longer than a sequence's); a wrong term errs by order 1
LIMIT = 1e-3


def _rollout(every, gates="hard", activation="relu", seed=5):
    return rollout_problem(seed, T, N, CELLS, H, A, ACTOR, CRITIC, gates, activation, every)


def test_one_segment_a_plant_is_the_whole_sequence_gradient_by_bits():
    """Fails without the feature: recurrent.gradient_segments does not exist"""
    R = _rollout(T)
    assert R["chunks"] == 1 and np.array_equal(bits(R["starts"][0]), bits(R["first"]))
    kw = dict(ent_coef=0.01, value_old=R["value_old"], clip_vf=0.2)
    whole = statement(R, **kw)
    Q = segment_batch(R)
    seg = statement_segments(R, Q, **dict(kw, value_old=Q["value_old"]))
    assert np.array_equal(bits(seg["grad"]), bits(whole["grad"])) and np.array_equal(bits(seg["hidden"]), bits(whole["hidden"]))
    for name in ppo.STATS:
        assert bits(np.float64(seg["stats"][name])) == bits(np.float64(whole["stats"][name])), name
    for name in ppo.STATS_MORE:
        assert bits(np.float64(seg["more"][name])) == bits(np.float64(whole["more"][name])), name
    # and the shard sums likewise
    a = statement(R, recurrent.shard_sums, count_total=2 * T * N)
    b = statement_segments(R, Q, recurrent.shard_sums_segments, count_total=2 * T * N)
    assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("every", [1, 2, 3])
@pytest.mark.parametrize("gates, activation", [("soft", "tanh"), ("hard", "relu")])
def test_truncation_is_what_it_claims_against_float64_autograd(gates, activation, every):
    R = _rollout(every, gates, activation)
    Q = segment_batch(R)
    out = statement_segments(R, Q, max_grad_norm=0.0, ent_coef=0.01)
    want = autograd_truncated(R, ent_coef=0.01)
    d = distance(out["grad"], want)
    print("pooled |g32 - g64| / |g64| (%s, %s, every %d): %.3e" % (gates, activation, every, d))
    assert out["grad"].dtype == np.float32 and d <= LIMIT, d
    n_core = recurrent.core_size(CELLS, H)
    edges = [0, 3 * H * CELLS, 3 * H * CELLS + 3 * H, n_core - 3 * H, n_core, R["theta"].size - 2 * A, R["theta"].size - A]
    for lo, hi in zip(edges[:-1], edges[1:]):
        assert np.abs(want[lo:hi]).max() > 0 and distance(out["grad"][lo:hi], want[lo:hi]) <= LIMIT, (lo, hi)
    assert out["stats"]["skipped"] == 2.0 and out["stats"]["count"] == T * N
    # the carry really is cut: the whole-sequence gradient of the same problem is another one, by far more than rounding
    whole = statement(R, max_grad_norm=0.0, ent_coef=0.01)
    print("the whole-sequence gradient stands %.3e from the truncated float64 one" % distance(whole["grad"], want))
    assert distance(whole["grad"], want) > 10 * LIMIT
    # under the parameters that made the stored states the forward pass is the whole sequence's, bit for bit: only the backward is cut
    flat = whole["hidden"].reshape(T, N, H)
    got = out["hidden"].reshape(every, R["chunks"], N, H)      # [s, c, p] of segment g = c * n + p
    assert np.array_equal(bits(np.ascontiguousarray(got.transpose(1, 0, 2, 3).reshape(T, N, H))), bits(flat))


@pytest.mark.parametrize("every", [1, 2, 3, 6])
def test_gather_and_index_against_brute_force(every):
    n, t = 33, 6
    rng = np.random.default_rng(every)
    arrays = {"obs": rng.standard_normal((t + 1, n, 2, 3)).astype(np.float32), "act": rng.standard_normal((t + 1, n, 2)),
              "extra": rng.standard_normal((t + 1, n, 1)).astype(np.float32)}
    adv, ret = rng.standard_normal((t + 1, n)).astype(np.float32), rng.standard_normal((t + 1, n)).astype(np.float32)
    keys = rollout.permutation_keys(7, every)
    chunks = t // every
    total, seen, B = chunks * n, [], 40
    moments = rollout.moments(adv[:t])
    for first in range(0, total, B):
        count = min(B, total - first)
        mb = rollout.minibatch(arrays, t, adv, ret, keys, first, count, unit="segment", every=every, moments=moments)
        assert np.array_equal(mb["index"], rollout.permutation(total, keys, first, count))
        assert mb["obs"].shape == (every, count, 2, 3) and mb["act"].shape == (every, count, 2) and mb["adv"].shape == (every, count)
        for j, g in enumerate(mb["index"]):
            c, p = divmod(int(g), n)
            for s in range(every):
                src = c * every + s
                assert np.array_equal(bits(mb["obs"][s, j]), bits(arrays["obs"][src, p])) and np.array_equal(bits(mb["act"][s, j]), bits(arrays["act"][src, p]))
                assert np.array_equal(bits(mb["extra"][s, j]), bits(arrays["extra"][src, p])) and bits(mb["ret"][s, j]) == bits(ret[src, p])
                want = np.float32((np.float64(adv[src, p]) - moments[1]) / (moments[3] + np.float64(1e-8)))
                assert bits(mb["adv"][s, j]) == bits(want)
        seen += [divmod(int(g), n) for g in mb["index"]]
    assert sorted(seen) == [(c, p) for c in range(chunks) for p in range(n)]      # one epoch visits every (c, p) exactly once
    with pytest.raises(ValueError, match="goes with unit='segment'"):
        rollout.minibatch(arrays, t, adv, ret, keys, 0, 4, unit="plant", every=2)
    with pytest.raises(ValueError, match="goes with unit='segment'"):
        rollout.minibatch(arrays, t, adv, ret, keys, 0, 4, unit="segment")
    with pytest.raises(ValueError, match="ragged last segments"):
        rollout.minibatch(arrays, t, adv, ret, keys, 0, 4, unit="segment", every=4)
    with pytest.raises(ValueError, match="every must be"):
        rollout.minibatch(arrays, t, adv, ret, keys, 0, 4, unit="segment", every=7)


@pytest.mark.parametrize("gates", ["soft", "hard"])
def test_starts_are_replay_at_the_boundaries(gates):
    R = _rollout(3, gates, "tanh" if gates == "soft" else "relu")
    core = recurrent.unpack(R["theta"], CELLS, A, ACTOR, CRITIC, H)[0]
    full = recurrent.replay(R["first"], R["obs"], R["episode"], R["ended"], core, gates)
    for every in (1, 2, 3, 6):
        got = recurrent.starts(R["first"], R["obs"], R["episode"], R["ended"], core, gates, every)
        assert got.shape == (T // every, N, H) and np.array_equal(bits(got), bits(np.ascontiguousarray(full[::every])))
        assert np.array_equal(bits(got[0]), bits(R["first"]))
    S = R["starts"]
    assert not bits(S[1, 1]).any()      # plant 1 restarts exactly on the boundary in front of slot 3: a +0.0 row
    assert not bits(S[1, 4]).any()      # plant 4's slot 2, the last of segment 0, is poisoned: a +0.0 row
    assert S[1, 0].any() and S[1, 2].any() and S[0].any()      # (the others carry a state; plant 2's restart lies inside segment 0)
    with pytest.raises(ValueError, match="ragged last segments"):
        recurrent.starts(R["first"], R["obs"], R["episode"], R["ended"], core, gates, 4)


def test_segment_words_and_ids_outside_the_rollout():
    R = _rollout(2)
    index = np.array([0, N + 3, 2 * N + 39, -1, 3 * N], dtype=np.int32)      # chunks * n = 120: the last two lie outside
    ep, en, ok = recurrent.segment_words(R["episode"], R["ended"], index, N, 2)
    assert ep.shape == (2, 5) and en.shape == (2, 5) and list(ok) == [True, True, True, False, False]
    assert np.array_equal(ep[:, 1], R["episode"][2:4, 3]) and np.array_equal(en[:, 2], R["ended"][4:6, 39]) and not ep[:, 3:].any() and not en[:, 3:].any()
    # the restart in front of a segment's first slot is dropped (it is in starts): plant 1 restarts in front of slot 2 = segment (1, 1)'s slot 0
    fresh = recurrent.restarts(*recurrent.segment_words(R["episode"], R["ended"], None, N, 2)[:2])
    assert recurrent.restarts(R["episode"], R["ended"])[2, 1] and not fresh[0].any() and fresh[1, 2]      # plant 2's cut: inside segment (0, 2)
    # a segment id outside poisons and skips its sequence, and the others' bits do not move
    Q = segment_batch(R, index)
    out = statement_segments(R, Q, keep=True)
    assert out["stats"]["skipped"] == 2 * 2 and np.isnan(out["logp_new"][:, 3:]).all() and not out["hidden"][:, 3:].any()
    alone = statement_segments(R, segment_batch(R, index[:3]))
    assert np.array_equal(bits(out["logp_new"][:, :3]), bits(alone["logp_new"])) and np.array_equal(bits(out["hidden"][:, :3]), bits(alone["hidden"]))
