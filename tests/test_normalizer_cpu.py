"""CPU: the statement of the running normaliser (nuclear_sim_amd/normalizer.py) -- the fold against an exact two-pass reference, what a
sample that does not count leaves behind, the clamp, freezing, the return's carry, the table through features.Stack, the merge of shards
and the refusals.  No device."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nuclear_sim_amd import features, normalizer
from nuclear_sim_amd.rollout import _tree

N_PLANTS, FOLDS, STREAMS = 300, 40, 5
# The oracle tolerance of the project.  The fold's own bound lies inside it: the sums are taken around a shift that is at most 100 standard
# deviations from the data (the first fold; afterwards around the running mean), so an error of one rounding, u = 2^-53 = 1.1e-16, in a
# sum of d or d * d is at most u * (1 + 100^2) of the variance's scale, and a value passes through the tree's depth of additions: 8 halvings
# and one further level for 300 plants, 9 -- u * (1 + 1e4) * 9 = 1e-11 < 1e-10.
TOL = 1e-10


def _spec(refs, scales=None, dtype="float64", stack=1):
    scales = [1.0] * len(refs) if scales is None else scales
    return {"stack": stack, "dtype": dtype, "columns": [features.column(c, ref=float(r), scale=float(s)) for c, (r, s) in enumerate(zip(refs, scales))]}


@pytest.fixture(scope="module")
def run():
    """40 folds of 300 plants x 5 streams with a few NaN, inf and 1e200 sprinkled in: the samples, who counts, and the normaliser behind
    them.  Column c has mean m_c and standard deviation s_c, and its first shift (the spec's ref) lies within 100 s_c of m_c"""
    rng = np.random.default_rng(20261020)
    means = np.array([0.0, 290.5, -3.0e4, 1.0e-3, 15.5e6])
    stds = np.array([1.0, 12.0, 250.0, 1.0e-6, 3.0e4])
    refs = means + np.array([0.0, 100.0, -100.0, 37.0, -99.0]) * stds
    x = means[None, :, None] + stds[None, :, None] * rng.standard_normal((FOLDS, STREAMS, N_PLANTS))
    bad = rng.random(x.shape) < 0.004
    kinds = rng.integers(0, 4, size=x.shape)
    x = np.where(bad, np.choose(kinds, [np.nan, np.inf, -np.inf, 1e200]), x)
    Z = normalizer.Normalizer(_spec(refs), list(range(STREAMS)), N_PLANTS)
    for t in range(FOLDS):
        Z.step(x[t])
    return {"x": x, "bad": bad, "Z": Z, "refs": refs, "stds": stds}


def test_the_fold_against_a_longdouble_two_pass_reference(run):
    x, bad, Z = run["x"], run["bad"], run["Z"]
    assert bad.sum() > 100 and all(bad[:, c].any() for c in range(STREAMS))
    for c in range(STREAMS):
        good = x[:, c][~bad[:, c]].astype(np.longdouble)
        mean = good.sum() / good.size
        var = ((good - mean) ** 2).sum() / good.size
        std = np.sqrt(var)
        assert Z.count[c] == good.size
        err_mean = abs(np.longdouble(Z.mean[c]) - mean) / std
        err_var = abs(np.longdouble(Z.M2[c]) / np.longdouble(Z.count[c]) - var) / var
        print("stream %d: mean off by %.3g std, variance by %.3g relative" % (c, float(err_mean), float(err_var)))
        assert err_mean <= TOL and err_var <= TOL, (c, float(err_mean), float(err_var))


def test_the_first_fold_from_a_far_ref_is_the_shifted_data_formula(run):
    """count == 0: mean = ref + s1 / cnt and M2 = s2 - s1^2 / cnt, checked against the exact reference for the stream 100 std away"""
    x, bad, refs = run["x"], run["bad"], run["refs"]
    Z = normalizer.Normalizer(_spec(refs), list(range(STREAMS)), N_PLANTS)
    Z.step(x[0])
    for c in range(STREAMS):
        good = x[0, c][~bad[0, c]].astype(np.longdouble)
        mean = good.sum() / good.size
        var = ((good - mean) ** 2).sum() / good.size
        assert Z.count[c] == good.size
        assert abs(np.longdouble(Z.mean[c]) - mean) / np.sqrt(var) <= TOL
        assert abs(np.longdouble(Z.M2[c]) / good.size - var) / var <= TOL


def test_samples_that_do_not_count_leave_what_a_fold_without_them_leaves():
    rng = np.random.default_rng(5)
    spec = _spec([2.0, -1.0])
    x = 3.0 + rng.standard_normal((6, 2, N_PLANTS))
    # at the tail: a fold over fewer plants is the same tree, its padding +0.0 where the bad samples stood
    tail = x.copy()
    tail[:, 0, -3:] = np.nan
    tail[:, 1, -3:] = np.inf
    A, B = normalizer.Normalizer(spec, [0, 1], N_PLANTS), normalizer.Normalizer(spec, [0, 1], N_PLANTS - 3)
    for t in range(6):
        A.step(tail[t])
        B.step(tail[t][:, :-3])
    for name in ("count", "mean", "M2"):
        assert np.array_equal(getattr(A, name), getattr(B, name)), name
    assert A.count[0] == 6 * (N_PLANTS - 3)
    # in the middle: which kind of bad value stood there makes no difference, and nothing becomes a NaN
    states = []
    for value in (np.nan, np.inf, -np.inf, 1e200, -1e160):
        y = x.copy()
        y[2, 0, 17] = y[4, 1, 256] = y[0, 0, 0] = value
        Z = normalizer.Normalizer(spec, [0, 1], N_PLANTS)
        for t in range(6):
            Z.step(y[t])
        states.append(Z.state())
        assert Z.count.tolist() == [6 * N_PLANTS - 2, 6 * N_PLANTS - 1]
        assert np.isfinite(Z.mean).all() and np.isfinite(Z.M2).all()
    for S in states[1:]:
        for name in ("count", "mean", "M2"):
            assert np.array_equal(S[name], states[0][name]), name


def test_the_clamp_is_reachable_and_a_constant_column_stays_at_zero():
    v, n = 0.7, N_PLANTS
    d = np.full(n, v)
    raw = _tree(d * d) - (_tree(d) * _tree(d)) / np.float64(n)
    assert raw < 0.0      # the rounding of s2 against s1^2 / N: what the clamp is for
    Z = normalizer.Normalizer(_spec([0.0]), [0], n)
    for _ in range(5):
        Z.step(np.full((1, n), v))
        assert Z.M2[0] == 0.0 and not np.signbit(Z.M2[0])
    assert Z.count[0] == 5 * n and Z.mean[0] == v
    ref, scale = Z.table()
    assert scale[0] == 1.0 / np.sqrt(np.float64(0.0) + np.float64(1e-8))


def test_frozen_leaves_the_state_bit_for_bit_and_still_normalises_the_reward():
    rng = np.random.default_rng(9)
    Z = normalizer.Normalizer(_spec([0.0]), [0], 64, reward={"gamma": 0.9, "clip": 5.0})
    for t in range(4):
        Z.step(rng.standard_normal((1, 64)), rng.standard_normal(64), np.zeros(64))
    before, ret = Z.state(), Z.ret.copy()
    Z.training = False
    r = rng.standard_normal(64)
    y = Z.step(1e6 * rng.standard_normal((1, 64)), r, np.zeros(64))
    for name in ("count", "mean", "M2"):
        assert np.array_equal(Z.state()[name].view(np.uint64), before[name].view(np.uint64)), name
    assert np.array_equal(Z.ret, ret * np.float64(0.9) + r)      # the return is still carried
    rscale = 1.0 / np.sqrt(before["M2"][1] / before["count"][1] + np.float64(1e-8))
    assert np.array_equal(y, np.clip(r * rscale, -5.0, 5.0))


def test_the_return_is_carried_by_index_primed_and_ended():
    g = np.float64(0.5)
    Z = normalizer.Normalizer(None, [], 4, reward={"gamma": 0.5, "clip": 1.0})
    one = np.ones(4)
    Z.step(None, one, [0, 0, 1, 0], [0, 0, 0, 0])
    assert Z.ret.tolist() == [1, 1, 1, 1]                       # unprimed: no carry
    Z.step(None, 2 * one, [0, 0, 0, 0], [0, 1, 0, 0])
    assert Z.ret.tolist() == [2.5, 2, 2, 2.5]                   # plant 1: the index moved; plant 2: it ended on the step before
    Z.clear([False, False, False, True])
    Z.step(None, 4 * one, [0, 0, 0, 0], [0, 1, 0, 0])
    assert Z.ret.tolist() == [5.25, 5, 5, 4]                    # plant 3: unprimed by clear
    Z.step(None, one, [1, 0, 0, 0], None)                       # index None: the one seen
    assert Z.ret.tolist() == [3.625, 3.5, 3.5, 3]
    y = Z.step(None, np.array([np.nan, 1e9, -1e9, 0.0]), [0, 0, 0, 0], None)
    assert np.isnan(Z.ret[0]) and Z.ret[1] == 3.5 * g + 1e9     # plant 0 ended: its return restarts at r, a NaN
    assert np.isnan(y[0]) and y[1] == 1.0 and y[2] == -1.0 and y[3] == 0.0      # a NaN passes the clip
    assert Z.count[0] == 4 * 4 + 3                              # the NaN return did not count


def test_apply_with_the_stack_reproduces_a_hand_computed_stack():
    spec = _spec([10.0, 0.0, 5.0], [1.0, 2.0, 1.0], dtype="float64", stack=2)
    spec["columns"][1]["lo"], spec["columns"][1]["hi"] = -1.0, 1.0
    Z = normalizer.Normalizer(spec, [0, 1], 2, eps=0.0)
    s0 = np.array([[1.0, 3.0], [2.0, 6.0], [7.0, 9.0]])      # rows = columns, [n_rows, n]
    Z.step(s0)
    # column 0: samples 1, 3: mean 2, M2 2, var 1; column 1: 2, 6: mean 4, var 4, scale 1 / 2; column 2 is not normalised
    assert Z.mean.tolist() == [2.0, 4.0] and Z.M2.tolist() == [2.0, 8.0]
    applied = Z.apply()
    assert [applied["columns"][j]["ref"] for j in range(3)] == [2.0, 4.0, 5.0]
    assert [applied["columns"][j]["scale"] for j in range(3)] == [1.0, 0.5, 1.0]
    assert applied["columns"][1]["lo"] == -1.0 and spec["columns"][0]["ref"] == 10.0      # the clip stays; the spec itself is untouched
    st = features.Stack(applied, 2)
    st.step(s0)
    want = np.array([[-1.0, -1.0, 2.0], [1.0, 1.0, 4.0]])
    assert np.array_equal(st.out, np.stack([want, want], axis=1))
    s1 = np.array([[2.0, 2.0], [4.0, 4.0], [5.0, 5.0]])
    Z.step(s1)      # column 0: 1, 3, 2, 2: mean 2, M2 2, var 1 / 2
    assert Z.mean.tolist() == [2.0, 4.0] and Z.M2.tolist() == [2.0, 8.0] and Z.count.tolist() == [4.0, 4.0]
    st.spec = Z.apply()
    st.step(s1)
    assert np.array_equal(st.out[:, 0], want) and np.array_equal(st.out[:, 1], np.zeros((2, 3)))
    assert st.spec["columns"][0]["scale"] == 1.0 / np.sqrt(0.5)


def test_merge_of_two_halves_agrees_with_one_run(run):
    x, refs = run["x"], run["refs"]
    halves = []
    for part in (slice(0, 150), slice(150, 300)):
        Z = normalizer.Normalizer(_spec(refs), list(range(STREAMS)), 150)
        for t in range(FOLDS):
            Z.step(x[t][:, part])
        halves.append(Z.state())
    M, whole = normalizer.merge(halves), run["Z"]
    for c in range(STREAMS):
        std = np.sqrt(whole.M2[c] / whole.count[c])
        assert M["count"][c] == whole.count[c]
        assert abs(M["mean"][c] - whole.mean[c]) / std <= TOL
        assert abs(M["M2"][c] - whole.M2[c]) / whole.M2[c] <= TOL
    empty = {k: np.zeros(STREAMS) for k in ("count", "mean", "M2")}
    again = normalizer.merge([empty, halves[0], empty])
    assert all(np.array_equal(again[k], halves[0][k]) for k in again)


REFUSALS = [
    ("neither", dict(columns=[], reward=None), "neither columns nor reward"),
    ("no features", dict(spec=None, columns=[0]), "no features are set"),
    ("out of range", dict(columns=[3]), "out of range"),
    ("negative", dict(columns=[-1]), "out of range"),
    ("twice", dict(columns=[0, 0]), "named twice"),
    ("bits", dict(columns=[1]), "'bits' column"),
    ("column ref", dict(columns=[2]), "second column"),
    ("NaN eps", dict(columns=[0], eps=float("nan")), "eps must be >= 0"),
    ("negative eps", dict(columns=[0], eps=-1e-9), "eps must be >= 0"),
    ("gamma above 1", dict(columns=[0], reward={"gamma": 1.5, "clip": 1.0}), "gamma must lie in [0, 1]"),
    ("NaN gamma", dict(columns=[0], reward={"gamma": float("nan"), "clip": 1.0}), "gamma must lie in [0, 1]"),
    ("clip 0", dict(columns=[0], reward={"gamma": 0.9, "clip": 0.0}), "clip must be positive"),
    ("NaN clip", dict(columns=[0], reward={"gamma": 0.9, "clip": float("nan")}), "clip must be positive"),
]


@pytest.mark.parametrize("what, args, reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_check_names_every_refusal(what, args, reason):
    spec = {"stack": 1, "dtype": "float32", "columns": [features.column(0), features.column(1, kind="bits", mask=1), features.column(2, ref=("col", 0))]}
    kw = dict(spec=spec, columns=[0], reward=None, eps=1e-8)
    kw.update(args)
    with pytest.raises(ValueError) as e:
        normalizer.check(kw["spec"], kw["columns"], kw["reward"], kw["eps"])
    assert reason in str(e.value), (what, str(e.value))
    normalizer.check(spec, [0], {"gamma": 0.99, "clip": 5.0}, 0.0)      # and a valid one passes


def test_the_cost_tool_names_its_flags():
    """tools/normalizer_cost.py, written on tools/overhead_harness.py: its command line, without a device"""
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "normalizer_cost.py")
    p = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--n", "--block", "--rounds", "--bank", "--bench-steps", "--parent", "--process-repeats", "--package-root", "--only-off", "--out"):
        assert re.search(r"(?<![\w-])%s(?![\w-])" % re.escape(flag), p.stdout), flag
