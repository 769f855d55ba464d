"""CPU: the numpy statement of what happens between rollout_advantages and the optimiser (nuclear_sim_amd.rollout: moments,
permutation_keys, permutation, minibatch) -- the contract the device's bits are held to in test_minibatch_gpu.py.

The moments are checked twice: by bits against a recursive restatement of the pinned tree written here, independently of the statement's
loops, and against math.fsum within a bound that is derived, not tuned (see ``_gamma``).  The permutation is checked for being one, for
windows being slices, and the minibatch against plain fancy indexing."""
import math
from fractions import Fraction

import numpy as np
import pytest

from nuclear_sim_amd import rollout

SIZES = [1, 2, 3, 4, 5, 17, 63, 64, 65, 255, 256, 257, 1000, 4097, 65537]


# ---------------------------------------------------------------------------------------------------------------- the permutation
@pytest.mark.parametrize("N", SIZES)
def test_permutation_is_a_permutation_and_windows_are_slices(N):
    keys = rollout.permutation_keys(11, N % 3)
    whole = rollout.permutation(N, keys)
    assert whole.dtype == np.int32 and whole.shape == (N,)
    assert np.array_equal(np.sort(whole), np.arange(N, dtype=np.int32))
    for first, count in ((0, 1), (0, N), (N - 1, 1), (N // 3, N - N // 3), (N // 2, min(7, N - N // 2))):
        assert np.array_equal(rollout.permutation(N, keys, first, count), whole[first:first + count]), (first, count)
    assert rollout.permutation(N, keys, N, 0).size == 0


def test_epochs_and_seeds_give_different_orders():
    orders = {(seed, epoch): rollout.permutation(1000, rollout.permutation_keys(seed, epoch)) for seed in (0, 1) for epoch in (0, 1)}
    names = list(orders)
    for i, a in enumerate(names):
        assert np.array_equal(orders[a], rollout.permutation(1000, rollout.permutation_keys(*a)))      # a function of (seed, epoch) alone
        for b in names[i + 1:]:
            assert not np.array_equal(orders[a], orders[b]), (a, b)
            assert (orders[a] == orders[b]).mean() < 0.05, (a, b)      # unrelated orders agree on about 1 entry in 1000


def test_keys_are_six_high_words_of_a_splitmix64_chain():
    def splitmix(state):      # the generator as published (Steele, Lea, Flood 2014; Vigna's splitmix64.c)
        state = (state + 0x9E3779B97F4A7C15) % 2 ** 64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
        return state, z ^ (z >> 31)
    assert splitmix(0)[1] == 0xE220A8397B1DCDAF      # its first output from state 0, as published
    for seed, epoch in ((0, 0), (12345, 7), (2 ** 64 - 1, 2 ** 40), (-1, 3)):
        _, z = splitmix(seed % 2 ** 64)
        state, want = z ^ (epoch % 2 ** 64), []
        for _ in range(rollout.ROUNDS):
            state, z = splitmix(state)
            want.append(z >> 32)
        keys = rollout.permutation_keys(seed, epoch)
        assert keys.dtype == np.uint32 and keys.tolist() == want
    assert rollout.ROUNDS == 6


def test_permutation_refuses_what_it_cannot_do():
    keys = rollout.permutation_keys(0, 0)
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(ValueError):
            rollout.permutation(bad, keys)
    with pytest.raises(ValueError):
        rollout.permutation(10, keys, 5, 6)
    with pytest.raises(ValueError):
        rollout.permutation(10, keys[:5])
    # the largest N: the network works on 32 bits; a window needs no table
    top = rollout.permutation(2 ** 31 - 1, keys, 2 ** 31 - 1 - 64, 64)
    assert top.min() >= 0 and len(set(top.tolist())) == 64


# ---------------------------------------------------------------------------------------------------------------- the moments
def _tree(c):
    """the pinned tree, restated recursively and element by element: a vector of one value is that value; else every group of 256 (the
    last padded with +0.0) is folded by adding its upper half onto its lower until one value is left, and the groups' values are summed
    by the same tree"""
    c = [np.float64(v) for v in c]
    if len(c) == 1:
        return c[0]

    def fold(group):
        if len(group) == 1:
            return group[0]
        half = len(group) // 2
        return fold([group[i] + group[half + i] for i in range(half)])
    groups = []
    for at in range(0, len(c), 256):
        group = c[at:at + 256]
        groups.append(fold(group + [np.float64(0.0)] * (256 - len(group))))
    return _tree(groups)


def _restated(x, ddof):
    rows, cols = x.shape
    col = [np.float64(0.0)] * cols
    for s in range(rows):
        col = [col[p] + np.float64(x[s, p]) for p in range(cols)]
    count = rows * cols
    mean = _tree(col) / np.float64(count)
    col2 = [np.float64(0.0)] * cols
    for s in range(rows):
        d = [np.float64(x[s, p]) - mean for p in range(cols)]
        col2 = [col2[p] + d[p] * d[p] for p in range(cols)]
    var = _tree(col2) / np.float64(count - ddof)
    return np.float64(count), mean, var, np.sqrt(var)


def _bits(values):
    return [np.float64(v).view(np.int64) for v in values]


SHAPES = [(1, 1, 0), (5, 1, 1), (1, 257, 1), (3, 256, 1), (7, 300, 1), (2, 65536 + 300, 0), (4, 1000, 2)]


@pytest.mark.parametrize("rows, cols, ddof", SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_moments_by_bits_against_the_recursive_restatement(rows, cols, ddof, dtype):
    rng = np.random.default_rng(rows * 1000 + cols)
    x = (rng.standard_normal((rows, cols)) * 3.0 + 0.5).astype(dtype)
    with np.errstate(all="ignore"):
        assert _bits(rollout.moments(x, ddof)) == _bits(_restated(x, ddof))


def _gamma(d):
    """gamma_d = d u / (1 - d u) with u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1): the relative
    perturbation a product of d factors (1 + delta), |delta| <= u, can carry"""
    u = 2.0 ** -53
    return d * u / (1.0 - d * u)


@pytest.mark.parametrize("rows, cols", [(8, 300), (128, 1000), (2, 65536 + 300)])
def test_moments_against_fsum_within_the_derived_bound(rows, cols):
    """Every input passes through at most rows additions down its column and then 8 per tree level, so the computed sum is sum x_i (1 +
    theta_i) with |theta_i| <= gamma_d, d = rows + 8 * levels: |sum - exact| <= gamma_d * sum |x|; the mean adds one division: gamma_{d +
    1}.  The variance is taken against the COMPUTED mean m, an exact double: fl(x_i - m) = (x_i - m)(1 + d1), its square carries d1 twice
    and one rounding more, then the same d additions and a division: every term of sum (x_i - m)^2 carries at most d + 4 factors, so
    |var - exact / (count - ddof)| <= gamma_{d + 4} * exact / (count - ddof).  The exact values are rationals (fractions.Fraction: a
    float is one), so the reference adds no error of its own; math.fsum, which rounds the exact sum once, is held against them too."""
    rng = np.random.default_rng(cols)
    x = (rng.standard_normal((rows, cols)) * 2.0 - 0.25).astype(np.float32)
    count, mean, var, std = rollout.moments(x, ddof=1)
    levels, g = 0, cols
    while g > 1:
        g, levels = -(-g // 256), levels + 1
    assert levels == (3 if cols > 65536 else 2)
    d = rows + 8 * levels
    flat = [float(v) for v in x.ravel()]
    exact = [Fraction(v) for v in flat]
    exact_sum, abs_sum = sum(exact), sum(abs(v) for v in exact)
    assert math.fsum(flat) == float(exact_sum)
    assert count == rows * cols
    assert abs(Fraction(float(mean)) - exact_sum / int(count)) <= Fraction(_gamma(d + 1)) * abs_sum / int(count)
    m = Fraction(float(mean))
    exact_sq = sum((v - m) ** 2 for v in exact)
    assert abs(Fraction(float(var)) - exact_sq / (int(count) - 1)) <= Fraction(_gamma(d + 4)) * exact_sq / (int(count) - 1)
    assert std == np.sqrt(var)


def test_moments_edge_cases():
    one = rollout.moments(np.array([[2.5]], dtype=np.float32), ddof=0)
    assert one == (1.0, 2.5, 0.0, 0.0)
    row = rollout.moments(np.arange(257, dtype=np.float64)[None, :], ddof=0)      # cols = 257: two groups, the second nearly all padding
    assert row[0] == 257.0 and row[1] == 128.0 and row[2] == (257.0 ** 2 - 1.0) / 12.0
    col = rollout.moments(np.arange(5, dtype=np.float32)[:, None], ddof=1)       # cols = 1: no tree
    assert col == (5.0, 2.0, 2.5, np.sqrt(2.5))
    x = np.ones((3, 300), dtype=np.float32)
    x[1, 299] = np.nan
    count, mean, var, std = rollout.moments(x)
    assert count == 900.0 and np.isnan(mean) and np.isnan(var) and np.isnan(std)
    x[1, 299] = np.inf
    assert rollout.moments(x)[1] == np.inf and np.isnan(rollout.moments(x)[2])
    for shape, ddof in (((1, 1), 1), ((2, 3), 6), ((2, 3), 7), ((2, 3), -1)):
        with pytest.raises(ValueError):
            rollout.moments(np.zeros(shape, dtype=np.float32), ddof=ddof)
    with pytest.raises(ValueError):
        rollout.moments(np.zeros(5, dtype=np.float32))
    with pytest.raises(ValueError):
        rollout.moments(np.zeros((2, 2), dtype=np.int32))


# ---------------------------------------------------------------------------------------------------------------- the minibatch
def _arrays(t_all, n, K, C, A, E, seed=0):
    rng = np.random.default_rng(seed)
    return {"obs": rng.standard_normal((t_all, n, K, C)).astype(np.float32),
            "act": rng.standard_normal((t_all, n, A)).astype(np.float32) if A else None,
            "extra": rng.standard_normal((t_all, n, E)).astype(np.float32)}, \
        rng.standard_normal((t_all, n)).astype(np.float32), rng.standard_normal((t_all, n)).astype(np.float32)


@pytest.mark.parametrize("unit", ["transition", "plant"])
@pytest.mark.parametrize("normalise", [False, True])
def test_minibatch_is_plain_fancy_indexing(unit, normalise):
    t_all, t, n, K, C, A, E = 6, 5, 37, 2, 3, 2, 1
    arrays, adv, ret = _arrays(t_all, n, K, C, A, E)
    keys = rollout.permutation_keys(5, 2)
    N = t * n if unit == "transition" else n
    first, count = 7, 20
    m = rollout.moments(adv[:t]) if normalise else None
    got = rollout.minibatch(arrays, t, adv, ret, keys, first, count, unit, moments=m, eps=1e-8)
    index = rollout.permutation(N, keys)[first:first + count]
    assert np.array_equal(got["index"], index)
    want_adv = adv[:t].astype(np.float64)
    if normalise:
        want_adv = (want_adv - m[1]) / (m[3] + 1e-8)
    want_adv = want_adv.astype(np.float32)
    if unit == "transition":
        s, p = index // n, index % n
        assert np.array_equal(got["obs"], arrays["obs"][s, p]) and got["obs"].shape == (count, K, C)
        assert np.array_equal(got["act"], arrays["act"][s, p]) and np.array_equal(got["extra"], arrays["extra"][s, p])
        assert np.array_equal(got["ret"], ret[s, p]) and np.array_equal(got["adv"], want_adv[s, p])
    else:
        assert np.array_equal(got["obs"], arrays["obs"][:t][:, index]) and got["obs"].shape == (t, count, K, C)
        assert np.array_equal(got["act"], arrays["act"][:t][:, index]) and np.array_equal(got["extra"], arrays["extra"][:t][:, index])
        assert np.array_equal(got["ret"], ret[:t][:, index]) and np.array_equal(got["adv"], want_adv[:t][:, index])
    assert got["adv"].dtype == np.float32
    if normalise:
        assert abs(float(want_adv.astype(np.float64).mean())) < 1e-6


def test_minibatch_without_controls_or_extras_and_in_double():
    arrays, adv, ret = _arrays(4, 9, 1, 3, 0, 0)
    arrays["extra"] = np.zeros((4, 9, 0), dtype=np.float32)
    got = rollout.minibatch(arrays, 4, adv.astype(np.float64), ret.astype(np.float64), rollout.permutation_keys(0, 0), 0, 36, moments=(36.0, 0.5, 4.0, 2.0), eps=0.5)
    assert got["act"] is None and got["extra"] is None and got["adv"].dtype == np.float64
    s, p = got["index"] // 9, got["index"] % 9
    assert np.array_equal(got["adv"], (adv.astype(np.float64)[s, p] - 0.5) / 2.5)
    for bad in (dict(unit="episode"), dict(count=0), dict(eps=-1.0), dict(eps=float("nan")), dict(t=0), dict(first=30, count=7)):
        kw = dict(t=4, first=0, count=5, unit="transition", eps=1e-8)
        kw.update(bad)
        with pytest.raises(ValueError):
            rollout.minibatch(arrays, kw["t"], adv, ret, rollout.permutation_keys(0, 0), kw["first"], kw["count"], kw["unit"], eps=kw["eps"])


@pytest.mark.parametrize("unit, t, n, batch", [("transition", 5, 300, 97), ("transition", 5, 300, 64), ("transition", 3, 7, 21), ("plant", 5, 300, 97), ("plant", 2, 65, 64)])
def test_the_minibatches_of_an_epoch_tile_the_range_exactly_once(unit, t, n, batch):
    arrays, adv, ret = _arrays(t, n, 1, 2, 0, 1, seed=3)
    keys = rollout.permutation_keys(1, 4)
    N = t * n if unit == "transition" else n
    seen, sizes = [], []
    for first in range(0, N, batch):
        count = min(batch, N - first)
        seen.append(rollout.minibatch(arrays, t, adv, ret, keys, first, count, unit)["index"])
        sizes.append(count)
    assert sizes[:-1] == [batch] * (len(sizes) - 1) and sizes[-1] == (N % batch or batch)
    if (unit, batch) == ("transition", 97) and N == 1500:
        assert sizes[-1] == 45
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(N, dtype=np.int32))
