"""CPU: the numpy statement of the rollout (nuclear_sim_amd.rollout) -- the contract the device's bits are compared with.

``rollout.advantages`` is checked against an independent textbook statement: per plant the slots are split into episode segments at the
ended slots, and A_t is the direct sum over the rest of its segment of (gamma * lam)^l * delta_(t+l).  The two differ in the order of
their roundings only: fewer than 4 T roundings of 2^-53 each, so rtol = 1e-12 -- with rewards in [1, 2] and values in [0, 0.25] every
delta is positive, every sum is one of positive terms and nothing cancels, so the bound holds relative to each result.
Exact identities are compared by bits.  No GPU, no library."""
import numpy as np
import pytest

from nuclear_sim_amd import rollout

T, N = 8, 5
SEEDS = (0, 1, 2, 3)
TERMINATED, TRUNCATED, CUT = rollout.TERMINATED, rollout.TRUNCATED, rollout.CUT


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _case(seed, T=T, n=N):
    """random reward [1, 2), float32 values [0, 0.25), outcomes, and the rows the truncated slots took (R = T: one per slot would do)"""
    rng = np.random.default_rng(seed)
    ended = rng.choice(np.array([0, TERMINATED, TRUNCATED, CUT, TERMINATED | CUT, TRUNCATED | CUT], dtype=np.uint8), size=(T, n),
                       p=[0.70, 0.08, 0.10, 0.06, 0.03, 0.03])
    ended[:, seed % n] = 0                                        # a plant without an end
    final_row = np.full((T, n), -1, dtype=np.int32)
    taken = np.zeros(n, dtype=np.int32)
    for t in range(T):
        for p in np.flatnonzero(ended[t] & TRUNCATED):
            final_row[t, p] = p * T + taken[p]
            taken[p] += 1
    return {"reward": 1.0 + rng.random((T, n)), "ended": ended, "final_row": final_row, "values": (0.25 * rng.random((T, n))).astype(np.float32),
            "last_value": (0.25 * rng.random(n)).astype(np.float32), "final_values": (0.25 * rng.random(n * T)).astype(np.float32)}


def _textbook(c, gamma, lam):
    """A_t = sum_l (gamma lam)^l delta_(t+l) over the rest of t's episode segment, by direct summation, plant by plant"""
    Tn, n = c["reward"].shape
    v = c["values"].astype(np.float64)
    adv = np.zeros((Tn, n))
    for p in range(n):
        ends = [t for t in range(Tn) if c["ended"][t, p]]
        start = 0
        for end in ends + ([Tn - 1] if not ends or ends[-1] != Tn - 1 else []):
            e = int(c["ended"][end, p])
            delta = []
            for u in range(start, end + 1):
                if u < end:
                    nv = v[u + 1, p]
                elif e & (TERMINATED | CUT):
                    nv = 0.0
                elif e & TRUNCATED:
                    nv = float(c["final_values"][c["final_row"][u, p]])
                else:
                    nv = float(c["last_value"][p])      # the last slot, not ended
                delta.append(c["reward"][u, p] + gamma * nv - v[u, p])
            for t in range(start, end + 1):
                adv[t, p] = sum((gamma * lam) ** l * d for l, d in enumerate(delta[t - start:]))
            start = end + 1
    return adv, adv + v


def test_the_seeds_cover_every_outcome():
    seen = set()
    for seed in SEEDS:
        e = _case(seed)["ended"]
        for p in range(N):
            col = e[:, p]
            ends = np.flatnonzero(col)
            seen |= {"no end"} if not len(ends) else set()
            seen |= {"terminated"} if (col == TERMINATED).any() else set()
            seen |= {"truncated"} if (col == TRUNCATED).any() else set()
            seen |= {"cut"} if (col == CUT).any() else set()
            seen |= {"an end on the last slot"} if col[-1] else set()
            seen |= {"two ends in one plant"} if len(ends) >= 2 else set()
    assert seen == {"no end", "terminated", "truncated", "cut", "an end on the last slot", "two ends in one plant"}, seen


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("gamma, lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0), (0.5, 1.0)])
def test_advantages_against_the_textbook_sum(seed, gamma, lam):
    c = _case(seed)
    adv, ret = rollout.advantages(gamma=gamma, lam=lam, dtype=np.float64, **c)
    want_adv, want_ret = _textbook(c, gamma, lam)
    assert (want_adv > 0).all()      # nothing cancels: the bound is relative to every result
    np.testing.assert_allclose(adv, want_adv, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(ret, want_ret, rtol=1e-12, atol=0.0)
    a32, r32 = rollout.advantages(gamma=gamma, lam=lam, dtype=np.float32, **c)
    assert a32.dtype == np.float32 and np.array_equal(_bits(a32), _bits(adv.astype(np.float32))) and np.array_equal(_bits(r32), _bits(ret.astype(np.float32)))


@pytest.mark.parametrize("seed", SEEDS)
def test_lambda_zero_gives_delta_by_bits(seed):
    c = _case(seed)
    gamma = 0.97
    adv, ret = rollout.advantages(gamma=gamma, lam=0.0, dtype=np.float64, **c)
    v = c["values"].astype(np.float64)
    for t in range(T):
        for p in range(N):
            e = int(c["ended"][t, p])
            if e & (TERMINATED | CUT):
                nv = 0.0
            elif e & TRUNCATED:
                nv = float(c["final_values"][c["final_row"][t, p]])
            else:
                nv = float(c["last_value"][p]) if t == T - 1 else v[t + 1, p]
            delta = (c["reward"][t, p] + gamma * nv) - v[t, p]
            assert _bits(np.float64(delta + 0.0)) == _bits(adv[t, p]), (t, p)      # (A = delta + 0 * carry)
            assert _bits(np.float64(adv[t, p] + v[t, p])) == _bits(ret[t, p]), (t, p)


@pytest.mark.parametrize("seed", SEEDS)
def test_lambda_one_without_values_is_the_discounted_return_to_go_by_bits(seed):
    c = _case(seed)
    gamma = 0.93
    adv, ret = rollout.advantages(c["reward"], c["ended"], c["final_row"], gamma=gamma, lam=1.0, dtype=np.float64)
    assert np.array_equal(_bits(adv), _bits(ret))
    for p in range(N):
        g = 0.0
        for t in range(T - 1, -1, -1):
            g = c["reward"][t, p] + gamma * (0.0 if c["ended"][t, p] else g)
            assert _bits(np.float64(g)) == _bits(ret[t, p]), (t, p)


def test_a_nan_in_one_episode_leaves_the_one_in_front_of_it_finite():
    for bit in (TERMINATED, TRUNCATED, CUT):
        c = _case(7)
        c["ended"][:] = 0
        c["ended"][3, 1] = bit                   # plant 1: an episode over the slots 0 .. 3, the next one from slot 4
        c["final_row"][:] = -1
        c["final_row"][3, 1] = 1 * T if bit == TRUNCATED else -1
        c["reward"][5, 1] = np.nan
        c["values"][6, 1] = np.nan
        adv, ret = rollout.advantages(gamma=0.99, lam=0.95, dtype=np.float64, **c)
        assert np.isfinite(adv[:4, 1]).all() and np.isfinite(ret[:4, 1]).all(), bit
        assert np.isnan(adv[4:6, 1]).all(), bit
        others = np.arange(N) != 1
        assert np.isfinite(adv[:, others]).all()
    c["ended"][3, 1] = 0                          # without the boundary the NaN does travel
    adv, _ = rollout.advantages(gamma=0.99, lam=0.95, dtype=np.float64, **c)
    assert np.isnan(adv[:6, 1]).all()


def test_refusals_of_the_statement():
    c = _case(0)
    for gamma, lam in ((1.5, 0.9), (0.9, -0.1), (float("nan"), 0.9), (0.9, float("nan"))):
        with pytest.raises(ValueError):
            rollout.advantages(gamma=gamma, lam=lam, **c)
    with pytest.raises(ValueError):
        rollout.advantages(c["reward"][:0], c["ended"][:0], c["final_row"][:0])
    for kw in ({"horizon": 0}, {"horizon": 4097}, {"extras": 9}, {"final_rows": -1}):
        with pytest.raises(ValueError):
            rollout.Recorder(**dict({"horizon": 4, "n": 3, "stack": (2, 3)}, **kw))


def test_the_recorder_assigns_final_rows_and_the_bound_holds_at_equality():
    """max_episode_steps 2 over 5 slots, the first truncation on slot 0 (the carried length is 1 when the rollout begins): slots 0, 2, 4 =
    ceil(5 / 2) = 3 rows of every plant, all taken and none short; a termination moves one plant's later truncations"""
    n, K, C, L, Tn = 3, 2, 3, 2, 5
    assert rollout.final_rows_bound(Tn, L) == 3 and rollout.final_rows_bound(6, L) == 3 and rollout.final_rows_bound(7, L) == 4
    assert rollout.final_rows_bound(Tn, 0) == 0 and rollout.final_rows_bound(Tn, None) == 0 and rollout.final_rows_bound(4, 9) == 1
    with pytest.raises(ValueError, match="below"):
        rollout.Recorder(Tn, n, (K, C), final_rows=2, autoreset=True, max_episode_steps=L)
    rec = rollout.Recorder(Tn, n, (K, C), axes=2, extras=1, final_rows=3, autoreset=True, max_episode_steps=L)
    stacks = np.arange(7 * n * K * C, dtype=np.float32).reshape(7, n, K, C)
    zeros = np.zeros(n)
    rec.pre(stacks[0], np.zeros((n, 2)), np.zeros((n, 1)))
    rec.post(zeros, zeros, stacks[0], episode=np.zeros(n))          # one step before the rollout begins: every carried length is 1
    rec.begin()
    assert rec.t == 0 and (rec.final_row == -1).all() and (rec.n_final == 0).all()
    index = np.zeros(n, dtype=np.int32)
    for t in range(Tn):
        done = np.zeros(n)
        done[1] = t == 2                                             # plant 1 terminates on the step its truncation is due: termination wins
        rec.pre(stacks[t], np.full((n, 2), t), np.full((n, 1), 10.0 + t))
        bits = rec.post(np.full(n, float(t)), done, stacks[t + 1], episode=index)
        index += bits != 0
    assert rec.t == Tn
    assert rec.ended[:, 0].tolist() == [2, 0, 2, 0, 2] and rec.ended[:, 1].tolist() == [2, 0, 1, 0, 2]
    assert rec.final_row[:, 0].tolist() == [0, -1, 1, -1, 2] and rec.final_row[:, 1].tolist() == [3, -1, -1, -1, 4] and rec.final_row[:, 2].tolist() == [6, -1, 7, -1, 8]
    assert rec.n_final.tolist() == [3, 2, 3]                          # at the bound, not beyond it
    assert rec.episode[:, 0].tolist() == [0, 1, 1, 2, 2]
    for t, p in ((0, 0), (2, 0), (4, 0), (0, 1), (4, 1), (2, 2)):
        assert np.array_equal(rec.final_obs[rec.final_row[t, p]], stacks[t + 1][p]), (t, p)
    assert np.array_equal(rec.obs[3], stacks[3]) and (rec.act[3] == 3).all() and (rec.extra[3] == 13.0).all() and (rec.reward[4] == 4.0).all()
    with pytest.raises(ValueError, match="full"):
        rec.pre(stacks[0], np.zeros((n, 2)), np.zeros((n, 1)))
    # a cut between two steps: bit 2 on the masked plants' previous slot, nothing in front of slot 0, their length starts again
    rec.begin()
    rec.cut(np.array([1, 0, 0]))
    assert (rec.ended[0] == [2, 2, 2]).all()                          # (slot 0 of the run before is untouched: t == 0)
    rec.pre(stacks[0], np.zeros((n, 2)), np.zeros((n, 1)))
    rec.post(zeros, zeros, stacks[1])
    rec.cut(np.array([0, 0, 1]))
    assert rec.ended[0].tolist() == [0, 0, 4]
    rec.pre(stacks[1], np.zeros((n, 2)), np.zeros((n, 1)))
    assert rec.post(zeros, zeros, stacks[2]).tolist() == [2, 2, 0]    # the cut plant's truncation is one step later


def test_without_autoreset_only_termination_is_recorded():
    rec = rollout.Recorder(3, 2, (1, 2), autoreset=False, max_episode_steps=1)
    assert rec.act is None and rec.extra.shape == (3, 2, 0) and rec.final_obs.shape == (0, 1, 2)
    for t in range(3):
        rec.pre(np.zeros((2, 1, 2)))
        rec.post(np.zeros(2), np.array([t == 1, 0]), np.zeros((2, 1, 2)), episode=np.array([5, 5]))
    assert rec.ended[:, 0].tolist() == [0, 1, 0] and (rec.ended[:, 1] == 0).all() and (rec.episode == -1).all() and (rec.final_row == -1).all()
