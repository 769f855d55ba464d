"""CPU: the numpy statement of the policy (nuclear_sim_amd/policy.py), the contract the device kernel is held to -- its emulated fmaf
against the C library's, its Philox4x32-10 against the published known-answer vectors, the parameter layout, the range of the noise, and
that the whole is a network at all.  No GPU, no library."""
import ctypes
import ctypes.util

import numpy as np
import pytest

from nuclear_sim_amd import policy


def _libm_fmaf():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.fmaf.argtypes = [ctypes.c_float] * 3
    m.fmaf.restype = ctypes.c_float
    return m.fmaf


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _triples():
    """random triples over many binades; cancelling ones (c close to -a * b); near-ties constructed so that a * b + c lies within a hair
    of the midpoint of two floats, on either side: where float32(float64(a) * b + c) rounds twice and goes wrong"""
    rng = np.random.default_rng(7)
    n = 20000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    out = [(a, b, c)]
    p = (a.astype(np.float64) * b.astype(np.float64))
    out.append((a, b, (-p).astype(np.float32)))                                           # cancels to the product's own rounding error
    out.append((a, b, np.nextafter((-p).astype(np.float32), np.float32(np.inf))))
    # near-ties: with x = i * 2^-23, (1 + x) * (h * (1 - x)) = h * (1 - x^2) lies a hair (h * i^2 * 2^-46) below h.  Let h be HALF an ulp of c:
    # the exact sum lies just below the midpoint of c and its neighbour, the double sum rounds ONTO the midpoint (the hair is below its
    # last bit), and the second rounding then ties to even: wrong whenever c's mantissa is odd
    k = 4000
    e = rng.integers(-10, 30, k).astype(np.float64)
    c = ((1.0 + rng.integers(0, 2 ** 23, k) * 2.0 ** -23) * 2.0 ** e).astype(np.float32)
    x = rng.integers(1, 200, k) * 2.0 ** -23
    a, b = (1.0 + x).astype(np.float32), (2.0 ** (e - 24.0) * (1.0 - x)).astype(np.float32)
    assert np.array_equal(a.astype(np.float64), 1.0 + x) and np.array_equal(b.astype(np.float64), 2.0 ** (e - 24.0) * (1.0 - x))
    out += [(a, b, c), (a, -b, c), (-a, b, -c), (a, b, -c)]
    return out


def test_the_emulated_fmaf_is_the_c_librarys():
    fmaf = _libm_fmaf()
    double_rounding_differs = 0
    for a, b, c in _triples():
        got = policy.fmaf(a, b, c)
        want = np.array([fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)
        bad = _bits(got) != _bits(want)
        assert not bad.any(), (a[bad][:3], b[bad][:3], c[bad][:3], got[bad][:3], want[bad][:3])
        naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
        double_rounding_differs += int((_bits(naive) != _bits(want)).sum())
    assert double_rounding_differs > 0      # the triples do reach the cases a plain double sum gets wrong


def test_fmaf_special_values():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    assert policy.fmaf(inf, 1.0, 0.0) == inf and np.isnan(policy.fmaf(inf, 0.0, 1.0)) and np.isnan(policy.fmaf(nan, 1.0, 1.0))
    assert _bits(policy.fmaf(0.0, 0.0, -0.0)) == 0      # the k extension: -0.0 becomes +0.0
    assert _bits(policy.fmaf(0.0, 0.0, np.float32(-1.5))) == _bits(np.float32(-1.5))


# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key -> output
KAT = [((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("counter, key, want", KAT)
def test_philox_known_answers(counter, key, want):
    got = policy.philox4x32(np.array(counter, dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert [int(x) for x in got] == list(want)


def test_noise_words_use_the_counter_the_header_states():
    seed, t, first = 0x299f31d0a4093822, (0x13198a2e << 32) | 0x85a308d3, 0x243f6a88 - 2
    w = policy.noise_words(seed, t, 3, 8, first_plant=first)
    assert w.shape == (3, 4, 4)
    for p in range(3):
        for j in range(4):
            want = policy.philox4x32(np.array([first + p, 0x85a308d3, 0x13198a2e, j], dtype=np.uint32), np.array([0xa4093822, 0x299f31d0], dtype=np.uint32))
            assert np.array_equal(w[p, j], want)
    # a batch split into shards draws what the whole batch draws
    assert np.array_equal(policy.noise(5, 9, 96, 3)[40:], policy.noise(5, 9, 56, 3, first_plant=40))


def test_noise_is_bounded_and_normal():
    z = policy.noise(1234, 0, 200000, 2)
    assert np.isfinite(z).all() and np.abs(z).max() <= policy.Z_MAX
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01 and abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 0.01
    # the extreme words: u1 at its smallest gives the largest radius, still inside the bound; u at its largest stays below 1
    w = np.array([[[0, 0, 0, 0]], [[0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff]]], dtype=np.uint32)
    ze = policy.noise_from_words(w, 2)
    assert np.isfinite(ze).all() and np.abs(ze).max() <= policy.Z_MAX and np.hypot(*ze[0]) > 8.5


def _nets(rng, cells, A, actor, critic, scale=0.3):
    def net(dims):
        return [((scale * rng.standard_normal((o, i))).astype(np.float32), (scale * rng.standard_normal(o)).astype(np.float32)) for i, o in dims]
    a, c = policy.sizes(cells, A, actor, critic)
    return net(a), net(c), (0.2 * rng.standard_normal(A) - 0.5).astype(np.float32)


def test_pack_and_unpack_round_trip():
    rng = np.random.default_rng(3)
    cells, A, actor, critic = 15, 3, (33, 17), (7,)
    a, c, log_std = _nets(rng, cells, A, actor, critic)
    theta = policy.pack(a, c, log_std)
    assert theta.dtype == np.float32 and theta.size == policy.theta_size(cells, A, actor, critic) == (15 * 33 + 33 + 33 * 17 + 17 + 17 * 3 + 3) + (15 * 7 + 7 + 7 + 1) + 6
    a2, c2, ls2, std2 = policy.unpack(theta, cells, A, actor, critic)
    for got, want in zip(a2 + c2, a + c):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(ls2, log_std) and np.array_equal(std2, np.exp(log_std).astype(np.float32))
    assert np.array_equal(theta[:15 * 33].reshape(33, 15), a[0][0])      # W[out][in] row-major first
    with pytest.raises(ValueError):
        policy.unpack(theta[:-1], cells, A, actor, critic)
    with pytest.raises(ValueError):
        policy.check(cells, A, (129,), critic, "relu")
    with pytest.raises(ValueError):
        policy.check(cells, A, actor, (1, 2, 3, 4), "relu")
    with pytest.raises(ValueError):
        policy.check(cells, A, actor, critic, "gelu")


def _a_network(cells, actor, critic, A=3, n=40):
    """against a float64 matmul to 1e-5: the fmaf chain, the padding and the layout compute an MLP"""
    rng = np.random.default_rng(11)
    a, c, log_std = _nets(rng, cells, A, actor, critic, scale=0.15)
    P = policy.Policy(cells, A, actor, critic, "relu", deterministic=True)
    P.load(policy.pack(a, c, log_std))
    x = rng.standard_normal((n, cells)).astype(np.float32)
    act, value, logp = P.step(x)

    def ref(net):
        h = x.astype(np.float64)
        for W, b in net[:-1]:
            h = np.maximum(h @ W.astype(np.float64).T + b, 0.0)
        return h @ net[-1][0].astype(np.float64).T + net[-1][1]
    assert np.abs(act - ref(a)).max() < 1e-5 and np.abs(value - ref(c)[:, 0]).max() < 1e-5
    assert np.allclose(logp, -(A * policy.HALF_LOG_2PI) - log_std.astype(np.float64).sum(), rtol=0, atol=1e-6) and P.t == 0
    assert np.array_equal(P.values(x), value)
    assert np.ptp(act, axis=0).min() > 0 and np.ptp(value) > 0


@pytest.mark.parametrize("cells, actor, critic", [(15, (7,), (33, 17)), (64, (64, 64), (64, 64))])
def test_the_relu_statement_is_a_network(cells, actor, critic):
    _a_network(cells, actor, critic)


@pytest.mark.parametrize("row", ["a", "d", "e", "f"])
def test_the_relu_statement_is_a_network_at_the_shape_tables_rows(row):
    """the rows of tests/test_policy_shapes_gpu.py's table with 65, 100, 255 and 66 cells, widths from 1 to 128 that differ between the
    nets, 2, 5, 7 and 6 axes: the same float64 matmul, the same 1e-5"""
    import test_policy_shapes_gpu as T
    S = T.table_spec(row)
    _a_network(S["cells"], S["actor"], S["critic"], S["n_axes"])


@pytest.mark.parametrize("row", ["a", "b", "c", "d", "e", "f"])
def test_the_explicit_rows_of_the_shape_table_reach_the_critic(row):
    """a condition on the GPU test's inputs: the 70 rows policy_values is given have values that are finite and differ, float32 and
    float64 rows alike (the critic of row e has ONE hidden unit, row f's chain ends in one)"""
    import test_policy_shapes_gpu as T
    S = T.table_spec(row)
    P = policy.Policy(S["cells"], S["n_axes"], S["actor"], S["critic"], "relu", deterministic=True)
    P.load(T.table_theta(row))
    for dtype in (np.float32, np.float64):
        v = P.values(T.table_rows(row, dtype))
        assert np.isfinite(v).all() and np.ptp(v) > 0 and len(np.unique(v)) > 10


def test_sampling_outputs_and_the_nan_rule():
    rng = np.random.default_rng(5)
    cells, A, actor, critic, n = 8, 3, (6,), (5,), 10
    a, c, log_std = _nets(rng, cells, A, actor, critic)
    P = policy.Policy(cells, A, actor, critic, "tanh", seed=77, act_dtype=np.float64)
    P.load(policy.pack(a, c, log_std))
    x = rng.standard_normal((n, cells))
    x[2, 3], x[7, 0] = np.nan, 1e300      # a NaN; a double that narrows to an infinity
    act, value, logp = P.step(x)
    assert P.t == 1 and act.dtype == np.float64 and value.dtype == logp.dtype == np.float32
    bad = np.zeros(n, dtype=bool); bad[[2, 7]] = True
    assert np.isnan(act[bad]).all() and np.isnan(value[bad]).all() and np.isnan(logp[bad]).all()
    assert np.isfinite(act[~bad]).all() and np.isfinite(value[~bad]).all() and np.isfinite(logp[~bad]).all()
    z = policy.noise(77, 0, n, A)
    mean = policy.forward(a, x, "tanh").astype(np.float64)
    std = np.exp(log_std).astype(np.float32).astype(np.float64)
    assert np.array_equal(act[~bad], (mean + std * z)[~bad])
    want = -(A * policy.HALF_LOG_2PI) - 0.5 * (z * z).sum(axis=1) - log_std.astype(np.float64).sum()
    assert np.allclose(logp[~bad], want[~bad], rtol=0, atol=1e-5)
    act2, _, _ = P.step(x)
    assert P.t == 2 and not np.array_equal(act2[~bad], act[~bad])
