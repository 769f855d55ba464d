"""CPU: one normaliser and one set of advantage moments across shards, the numpy statements (nuclear_sim_amd.normalizer.shard_delta and
combine; nuclear_sim_amd.rollout.moments_part, moments_combine and moments_shards): what the device's npb_normalizer_shard_delta,
npb_normalizer_apply_shards, npb_rollout_moments_part and npb_rollout_moments_combine give by bits (tests/test_shard_sync_gpu.py).

Bits where the statement promises bits (a zero base, an empty shard, one shard's moments), the project's oracle tolerance against an exact
two-pass reference where it promises accuracy, a derived bound for the pinned sums against math.fsum, and the refusals by name.
Every test fails without the feature: the functions do not exist."""
import math

import numpy as np
import pytest

from nuclear_sim_amd import normalizer, rollout
from test_normalizer_cpu import TOL, _spec

KEYS = ("count", "mean", "M2")
U = 2.0 ** -53


def _bits(state):
    return [np.asarray(state[k], dtype=np.float64).tobytes() for k in KEYS]


def _zeros(S):
    return {k: np.zeros(S) for k in KEYS}


def _some_state(seed, S=5, n=40.0):
    rng = np.random.default_rng(seed)
    return {"count": np.full(S, n), "mean": 10.0 ** rng.integers(-3, 6, S) * rng.standard_normal(S), "M2": n * rng.random(S) + 0.1}


# ---------------------------------------------------------------------------------------------------------------- the normaliser
def test_a_delta_from_a_zero_base_is_the_state_by_bits():
    for seed in range(20):
        cur = _some_state(seed)
        cur["M2"][1] = 0.0      # a constant column
        assert _bits(normalizer.shard_delta(cur, _zeros(5))) == _bits(cur), seed
        # and a combine of that one delta from the zero base is the state again: W = 1 from zero is the identity
        assert _bits(normalizer.combine(_zeros(5), [normalizer.shard_delta(cur, _zeros(5))])) == _bits(cur), seed
        cur["mean"][0] = -0.0      # a signed zero survives the delta (the combine's 0.0 + -0.0 is +0.0: the same mean)
        assert _bits(normalizer.shard_delta(cur, _zeros(5))) == _bits(cur), seed
    # an array [3, S] is taken as the dict is
    cur = _some_state(3)
    packed = np.stack([cur[k] for k in KEYS])
    assert _bits(normalizer.shard_delta(packed, np.zeros((3, 5)))) == _bits(cur)


def test_a_shard_with_nothing_new_gives_zeros_and_changes_nothing():
    base, other = _some_state(1), _some_state(2, n=17.0)
    nothing = normalizer.shard_delta(base, base)
    assert all(not nothing[k].any() and not np.signbit(nothing[k]).any() for k in KEYS)
    # a stream that did not move beside streams that did
    cur = {k: v.copy() for k, v in base.items()}
    cur["count"][2:] += 9.0; cur["mean"][2:] += 0.25; cur["M2"][2:] += 3.0
    part = normalizer.shard_delta(cur, base)
    assert part["count"].tolist() == [0.0, 0.0, 9.0, 9.0, 9.0] and not part["mean"][:2].any() and not part["M2"][:2].any()
    want = normalizer.combine(base, [other])
    for deltas in ([nothing, other], [other, nothing], [nothing, other, nothing], [nothing, nothing, other]):
        assert _bits(normalizer.combine(base, deltas)) == _bits(want)
    assert _bits(normalizer.combine(base, [nothing])) == _bits(base)
    # the same from a zero base: the empty shard first, so that the first merged shard is not shard 0
    assert _bits(normalizer.combine(_zeros(5), [_zeros(5), other, _zeros(5)])) == _bits(normalizer.combine(_zeros(5), [other]))


def test_the_order_of_the_shards_is_in_the_bits():
    base = _zeros(5)
    a, b, c = (_some_state(s, n=float(n)) for s, n in ((4, 70), (5, 257), (6, 33)))
    one, two = normalizer.combine(base, [a, b, c]), normalizer.combine(base, [c, b, a])
    assert one["count"].tolist() == two["count"].tolist() == [360.0] * 5
    assert _bits(one) != _bits(two)      # the order is pinned because it matters
    assert np.allclose(one["mean"], two["mean"], rtol=1e-12, atol=0) and np.allclose(one["M2"], two["M2"], rtol=1e-12)


PLANTS, ROUNDS, STREAMS, SILENT = (70, 257, 33), 6, 5, (3, 1)      # (round 3: the middle shard does not step)


@pytest.fixture(scope="module")
def synced():
    """Six synchronisations of three normalisers of 70, 257 and 33 plants, 5 + i folds before synchronisation i, the middle shard silent
    in round 3.  Five streams whose level lies up to 517 standard deviations from zero, the first shift (the spec's ref) within 1.5
    standard deviations of the data, every shard's data offset by 0.7 standard deviations of its own: the shards really differ"""
    rng = np.random.default_rng(20261020)
    stds = np.array([1.0, 12.0, 250.0, 1.0e-6, 3.0e4])
    means = np.array([0.0, 290.5, -517.0, 37.0, 100.0]) * stds
    assert np.max(np.abs(means) / stds) <= 517.0
    refs = means + np.array([0.0, 1.5, -1.5, 0.9, -1.2]) * stds
    offsets = np.array([-0.7, 0.0, 0.7])
    shards = [normalizer.Normalizer(_spec(refs), list(range(STREAMS)), n) for n in PLANTS]
    base = _zeros(STREAMS)
    samples = [[] for _ in range(STREAMS)]
    history = []
    for i in range(ROUNDS):
        for w, Z in enumerate(shards):
            if (i, w) == SILENT:
                continue
            for _ in range(5 + i):
                x = (means + offsets[w] * stds)[:, None] + stds[:, None] * rng.standard_normal((STREAMS, Z.n))
                Z.step(x)
                for c in range(STREAMS):
                    samples[c].append(x[c])
        before = [Z.state() for Z in shards]
        deltas = [normalizer.shard_delta(s, base) for s in before]
        base = normalizer.combine(base, deltas)
        for Z in shards:
            Z.load_state(base)
        history.append({"before": before, "deltas": deltas, "after": {k: v.copy() for k, v in base.items()}})
    return {"history": history, "samples": [np.concatenate(s) for s in samples], "stds": stds, "shards": shards}


def test_six_synchronisations_of_three_shards_against_an_exact_two_pass_reference(synced):
    final = synced["history"][-1]["after"]
    worst = 0.0
    for c in range(STREAMS):
        x = synced["samples"][c].astype(np.longdouble)
        mean = x.sum() / x.size
        M = ((x - mean) ** 2).sum()
        std = np.sqrt(M / x.size)
        assert final["count"][c] == x.size == sum(n * sum(5 + i for i in range(ROUNDS) if (i, w) != SILENT) for w, n in enumerate(PLANTS))
        err_mean, err_M = float(abs(np.longdouble(final["mean"][c]) - mean) / std), float(abs(np.longdouble(final["M2"][c]) - M) / M)
        print("stream %d: mean off by %.3g std, M2 by %.3g relative" % (c, err_mean, err_M))
        worst = max(worst, err_mean, err_M)
        assert err_mean <= TOL and err_M <= TOL, (c, err_mean, err_M)
    print("worst %.3g" % worst)
    # every shard ends every round on the same bits, and the shards' offsets are in the spread: the streams really were merged
    assert all(_bits(Z.state()) == _bits(final) for Z in synced["shards"])
    assert (np.sqrt(final["M2"] / final["count"]) > 1.05 * synced["stds"]).all()


def test_the_silent_shard_exports_zeros_and_the_later_bases_are_not_zero(synced):
    i, w = SILENT
    silent = synced["history"][i]["deltas"][w]
    assert all(not silent[k].any() for k in KEYS)
    assert all(d["count"].all() for j, d in enumerate(synced["history"][i]["deltas"]) if j != w)
    # from round 1 on the delta is taken against a base that is not zero: it is not the state, and it counts only the new samples
    for i, H in enumerate(synced["history"]):
        for w, (cur, d) in enumerate(zip(H["before"], H["deltas"])):
            new = 0 if (i, w) == SILENT else PLANTS[w] * (5 + i)
            assert d["count"].tolist() == [float(new)] * STREAMS, (i, w)
            assert (i == 0) == (_bits(d) == _bits(cur)), (i, w)


def test_one_shard_from_a_base_that_is_not_zero_is_not_asserted_to_be_the_identity(synced):
    """W = 1 is the identity only from a zero base: un-merging and merging again both round.  The count is exact; mean and M2 come back
    within the project's tolerance, and nothing here says they come back by bits"""
    H = synced["history"][2]
    cur, base = H["before"][1], synced["history"][1]["after"]
    back = normalizer.combine(base, [normalizer.shard_delta(cur, base)])
    assert back["count"].tolist() == cur["count"].tolist()
    std = np.sqrt(cur["M2"] / cur["count"])
    assert (np.abs(back["mean"] - cur["mean"]) / std <= TOL).all() and (np.abs(back["M2"] - cur["M2"]) / cur["M2"] <= TOL).all()


# ---------------------------------------------------------------------------------------------------------------- the moments
SHAPES = [(3, 1), (5, 257), (2, 70)]


def _array(seed, shape, dtype):
    rng = np.random.default_rng(seed)
    return (3.0 * rng.standard_normal(shape) + 1.5).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_shards_moments_are_the_moments_by_bits(shape, dtype):
    x = _array(7, shape, dtype)
    for ddof in (0, 1):
        want, got = rollout.moments(x, ddof), rollout.moments_shards([x], ddof)
        assert [np.float64(v).tobytes() for v in got] == [np.float64(v).tobytes() for v in want], (shape, ddof)
    count, total = rollout.moments_part(x)
    assert count == x.size and total / count == rollout.moments(x)[1]


def _levels(cols):
    levels = 0
    while cols > 1:
        cols, levels = -(-cols // rollout.TREE_WIDTH), levels + 1
    return levels


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_three_ragged_shards_against_fsum_within_the_bound_of_the_pinned_sum(dtype):
    """The bound.  A value of the pinned total passes through at most k additions: the rows of its column (the chain starts at 0.0), 8 per
    level of the tree (the halves 128 .. 1) and the W of the combine.  Each addition rounds once, so the total is off by at most
    ((1 + u)^k - 1) <= k u / (1 - k u) of fsum(|summands|), u = 2^-53; the division rounds once more (k + 1).  The squares' summands
    carry three roundings of their own (the difference, the product), so k + 4 for the variance, whose summands are all positive; and
    the computed mean, off by delta, adds count * delta^2 to the sum of squares exactly."""
    xs = [_array(10 + w, shape, dtype) for w, shape in enumerate(SHAPES)]
    count, mean, var, std = rollout.moments_shards(xs, ddof=1)
    flat = np.concatenate([x.astype(np.float64).ravel() for x in xs])
    assert count == flat.size == 3 + 5 * 257 + 2 * 70
    k = max(s[0] for s in SHAPES) + 8 * max(_levels(s[1]) for s in SHAPES) + len(SHAPES)
    assert k == 5 + 16 + 3
    exact_mean = math.fsum(flat) / flat.size
    bound_mean = (k + 1) * U / (1 - (k + 1) * U) * math.fsum(np.abs(flat)) / flat.size
    print("mean off by %.3g, bound %.3g" % (abs(mean - exact_mean), bound_mean))
    assert abs(mean - exact_mean) <= bound_mean
    exact_var = math.fsum((flat - exact_mean) ** 2) / (flat.size - 1)      # (the summands of fsum are themselves rounded: 3 u, inside k + 4 twice over)
    bound_var = 2 * (k + 4) * U / (1 - 2 * (k + 4) * U) * exact_var + flat.size * bound_mean ** 2 / (flat.size - 1)
    print("var off by %.3g, bound %.3g" % (abs(var - exact_var), bound_var))
    assert abs(var - exact_var) <= bound_var and std == np.sqrt(var)
    # the shards' order is in the sum, the result does not depend on it beyond the bound
    other = rollout.moments_shards(xs[::-1], ddof=1)
    assert other[0] == count and abs(other[1] - exact_mean) <= bound_mean and abs(other[2] - exact_var) <= bound_var
    # the second pass is taken around the GLOBAL mean, not around each shard's own
    own = [rollout.moments_part(x, rollout.moments(x, 0)[1])[1] for x in xs]
    around_global = [rollout.moments_part(x, mean)[1] for x in xs]
    assert all(g > o for g, o in zip(around_global, own))


def test_a_nan_propagates():
    xs = [_array(20 + w, shape, np.float32) for w, shape in enumerate(SHAPES)]
    xs[1][3, 200] = np.nan
    count, mean, var, std = rollout.moments_shards(xs)
    assert count == 3 + 5 * 257 + 2 * 70 and np.isnan(mean) and np.isnan(var) and np.isnan(std)
    xs[1][3, 200] = np.inf
    assert np.isinf(rollout.moments_shards(xs)[1]) and np.isnan(rollout.moments_shards(xs)[2])


# ---------------------------------------------------------------------------------------------------------------- the refusals
def test_the_refusals_by_name():
    good, z5, z4 = _some_state(1), _zeros(5), _zeros(4)
    with pytest.raises(ValueError, match="cur has 5 streams and base 4"):
        normalizer.shard_delta(good, z4)
    with pytest.raises(ValueError, match=r"a state is \{count, mean, M2\} or an array \[3, S\]"):
        normalizer.shard_delta(np.zeros((2, 5)), z5)
    with pytest.raises(ValueError, match="vectors of one length"):
        normalizer.shard_delta({"count": np.zeros(5), "mean": np.zeros(4), "M2": np.zeros(5)}, z5)
    with pytest.raises(ValueError, match="1 .. 64 shards, not 0"):
        normalizer.combine(z5, [])
    with pytest.raises(ValueError, match="1 .. 64 shards, not 65"):
        normalizer.combine(z5, [good] * 65)
    normalizer.combine(z5, [good] * 64)
    with pytest.raises(ValueError, match="a delta has 4 streams and the base 5"):
        normalizer.combine(z5, [good, z4])
    x = _array(1, (2, 70), np.float32)
    with pytest.raises(ValueError, match=r"a \[rows, cols\] float32 or float64 array"):
        rollout.moments_part(x[0])
    with pytest.raises(ValueError, match=r"a \[rows, cols\] float32 or float64 array"):
        rollout.moments_part(x.astype(np.float16))
    with pytest.raises(ValueError, match="rows and cols must be >= 1"):
        rollout.moments_part(x[:0])
    part = rollout.moments_part(x)
    with pytest.raises(ValueError, match=r"parts are \[W, 2\]"):
        rollout.moments_combine([part + (0.0,)])
    with pytest.raises(ValueError, match=r"parts are \[W, 2\]"):
        rollout.moments_combine(np.zeros((0, 2)))
    with pytest.raises(ValueError, match=r"parts are \[W, 2\]"):
        rollout.moments_combine([part] * 65)
    rollout.moments_combine([part] * 64)
    with pytest.raises(ValueError, match="ddof must be >= 0"):
        rollout.moments_combine([part], ddof=-1)
    with pytest.raises(ValueError, match="total count .* is below 1"):
        rollout.moments_combine([(0.0, 0.0)])
    with pytest.raises(ValueError, match="must exceed ddof = 140"):
        rollout.moments_combine([part], ddof=140, squares=True)
    with pytest.raises(ValueError, match="must exceed ddof = 1"):
        rollout.moments_shards([x[:1, :1]], ddof=1)
    assert rollout.moments_shards([x[:1, :1], x[:1, 1:2]], ddof=1)[0] == 2.0      # one cell a shard is enough when there are two
