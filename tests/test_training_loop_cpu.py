"""CPU: the two things tests/test_training_loop_gpu.py takes for granted of the numpy statements, checked on the statements alone.

1. THE BOUND on |logp_new - logp_old| of an unchanged policy.  The policy draws z, writes ``act = mean + std * z`` narrowed to the controls'
input type and records ``logp_old = (float)lp(z)``; the gradient recovers ``d = (act - mean) / std`` and forms ``logp_new = (float)lp(d)``.
With ``e_a = (0.5 * spacing(|act_a|, controls dtype) + 4 * spacing(|act_a|, float64)) / std_a`` -- the narrowing of the action, and the
roundings of the product, the sum, the difference and the quotient in double -- d stands at most e from z, each term 0.5 * d^2 at most
``|z| * e + e^2 / 2`` from 0.5 * z^2, and the two narrowings to float add one float32 spacing of logp_old:

    bound = sum_a (|z_a| * e_a + e_a^2 / 2) * (1 + 1e-6) + spacing(float32 |logp_old|)

``logp_bound`` states it; the GPU suite imports it.  Here ``policy.outputs`` and then ``ppo.gradient`` run on 2048 rows with 1, 3 and 8
axes, float32 and float64 controls, sampling and deterministic.  Measured: float32 controls, the largest diff / bound 0.985, 0.917 and
0.821 for 1, 3 and 8 axes (600, 478 and 338 of the rows differ in some bit); float64 controls and a deterministic policy, logp_new is
logp_old by bits on every row.

2. THE ORDER the GPU suite assumes of one step: the normaliser's fold, then the table, then the features' pass A, and the policy of the
NEXT step reads that stack.  ``Normalizer``, ``features.Stack`` and ``policy.Policy`` are chained on synthetic samples; a frame written
before a table change keeps its old normalisation in the stack (documented: normalizer.py, THE TABLE)."""
import numpy as np
import pytest

from nuclear_sim_amd import features, normalizer, policy, ppo
from test_ppo_cpu import CLIP, ENT, VF, make_theta

ROWS, CELLS, HIDDEN, CHAIN = 2048, 15, (33, 17), 64
# |log ratio| is read back as log(ratio): the exp that formed the ratio may err by 4 ulp of a number next to 1 (the device's licence; numpy's
# by 1) and the log taken here by one more.  That is the measurement's own error, 5 * 2^-52, a hundred-millionth of the bounds it is added to
LOG_RATIO_SLACK = 5.0 * 2.0 ** -52


def logp_bound(act, z, std, logp_old):
    """``(bound, ulp)`` float64 [rows]: the module docstring's bound from a minibatch's own data -- ``act`` [rows, A] of the controls' input
    type, the ``z`` [rows, A] that made it, ``std`` [A] and the recorded ``logp_old`` float32 [rows]; ``ulp`` is spacing(float32 |logp_old|)"""
    act = np.abs(np.asarray(act))
    assert act.dtype in (np.float32, np.float64) and np.asarray(logp_old).dtype == np.float32
    wide = act.astype(np.float64)
    e = (0.5 * np.spacing(act).astype(np.float64) + 4.0 * np.spacing(wide)) / np.asarray(std, dtype=np.float64)[None, :]
    ulp = np.spacing(np.abs(np.asarray(logp_old))).astype(np.float64)
    return ((np.abs(np.asarray(z, dtype=np.float64)) * e + 0.5 * e * e) * (1.0 + 1e-6)).sum(axis=1) + ulp, ulp


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a.view(np.int64)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("deterministic", [False, True], ids=["sampling", "deterministic"])
@pytest.mark.parametrize("axes", [1, 3, 8])
@pytest.mark.parametrize("act_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_an_unchanged_policy_gives_its_own_logp_back_within_the_bound(act_dtype, axes, deterministic):
    rng = np.random.default_rng(100 + axes)
    theta = make_theta(rng, CELLS, axes, HIDDEN, HIDDEN)
    a_net, c_net, log_std, std = policy.unpack(theta, CELLS, axes, HIDDEN, HIDDEN)
    obs = rng.standard_normal((ROWS, CELLS)).astype(np.float32)
    z = np.zeros((ROWS, axes)) if deterministic else policy.noise(7, 0, ROWS, axes)
    act, value, logp_old = policy.outputs(policy.forward(a_net, obs, "relu"), policy.forward(c_net, obs, "relu")[:, 0], log_std, std, z, obs, act_dtype)
    assert act.dtype == act_dtype
    out = ppo.gradient(theta, CELLS, axes, HIDDEN, HIDDEN, "relu", obs, act, logp_old, rng.standard_normal(ROWS).astype(np.float32),
                       rng.standard_normal(ROWS).astype(np.float32), clip=CLIP, vf_coef=VF, ent_coef=ENT, rows_per_chain=CHAIN)
    assert out["stats"]["skipped"] == 0 and out["stats"]["clip_fraction"] == 0.0 and out["stats"]["approx_kl"] >= 0.0
    assert np.array_equal(_bits(out["value_new"]), _bits(value))
    bound, ulp = logp_bound(act, z, std, logp_old)
    diff = np.abs(out["logp_new"].astype(np.float64) - logp_old.astype(np.float64))
    log_ratio = np.abs(np.log(out["ratio"]))
    print("the largest diff / bound %.3f; rows whose logp differs in some bit: %d of %d" % ((diff / bound).max(), int((diff != 0).sum()), ROWS))
    assert (diff <= bound).all()
    if deterministic or act_dtype == np.float64:
        assert np.array_equal(_bits(out["logp_new"]), _bits(logp_old))
    if deterministic:      # d is exactly 0 and the two sums are the same sequence of doubles: only logp_old's narrowing is left
        assert (log_ratio <= 0.5 * ulp + LOG_RATIO_SLACK).all()
    else:
        assert (diff != 0).any() == (act_dtype == np.float32)      # (float32 controls do move some row: the bound is not idle)
        assert (log_ratio <= bound + 0.5 * ulp + LOG_RATIO_SLACK).all()


# ---------------------------------------------------------------------------------------------------------------- 2
def test_fold_then_table_then_pass_a_and_the_next_policy_reads_that_stack():
    n, K, A, steps = 40, 3, 2, 4
    spec = {"stack": K, "dtype": "float32",
            "columns": [features.column(0, scale=0.1, ref=50.0, lo=-5.0, hi=5.0, live=True), features.column(1, kind="bits", mask=0x3),
                        features.column(2, live=True), features.column(0, ref=("col", 2), live=True, ref_live=True)]}
    Z = normalizer.Normalizer(spec, [0, 2], n, reward={"gamma": 0.99, "clip": 5.0})
    ref = features.Stack(spec, n)
    P = policy.Policy(K * 4, A, (7,), (7,), "relu", seed=3)
    P.load(make_theta(np.random.default_rng(1), K * 4, A, (7,), (7,)))
    rng = np.random.default_rng(2)
    samples = lambda t: np.stack([60.0 + 3.0 * t + 5.0 * rng.standard_normal(n), rng.integers(0, 8, n).astype(np.float64), t + rng.standard_normal(n)])
    frames, tables, read = [], [], []
    for t in range(steps):
        before = ref.out.copy()      # what the policy of this step reads: the stack the step before left
        if t:
            act, value, logp = P.step(before)
            read.append((before, value))
        x = samples(t)
        old = Z.apply()
        Z.step(x, rng.standard_normal(n), np.zeros(n, np.uint8))      # 1. the fold ...
        ref.spec = Z.apply()                                          # 2. ... then the table ...
        ref.step(x)                                                   # 3. ... then pass A
        frames.append((x, ref.out[:, -1].copy()))
        tables.append(Z.table())
        # the newest frame is normalised with statistics that include it, not with the table the step began with
        assert np.array_equal(_bits(ref.out[:, -1]), _bits(features.frame(x, Z.apply())))
        assert not np.array_equal(_bits(ref.out[:, -1, [0, 2]]), _bits(features.frame(x, old)[:, [0, 2]]))
        # the columns the normaliser leaves alone keep the spec's own transform
        assert np.array_equal(_bits(ref.out[:, -1, [1, 3]]), _bits(features.frame(x, spec)[:, [1, 3]]))
        if t:      # the frame of the step before kept ITS table's normalisation: the stack is not rewritten when the table moves
            x_old, f_old = frames[t - 1]
            assert np.array_equal(_bits(ref.out[:, -2]), _bits(f_old))
            assert not np.array_equal(_bits(f_old[:, [0, 2]]), _bits(features.frame(x_old, Z.apply())[:, [0, 2]]))
    assert Z.count.tolist() == [float(steps * n)] * 3
    assert not np.array_equal(tables[0][0], tables[-1][0]) and not np.array_equal(tables[0][1], tables[-1][1])
    # the policy of step t read the stack behind step t - 1, frames of three different tables in it: its value is the critic of exactly
    # those rows, and not of the same samples normalised again with the newest table
    before, value = read[-1]
    assert np.array_equal(_bits(value), _bits(P.values(before)))
    again = np.stack([features.frame(x, Z.apply()) for x, _ in frames[-K - 1:-1]], axis=1)
    assert again.shape == before.shape and not np.array_equal(_bits(P.values(again)), _bits(value))
