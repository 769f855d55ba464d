"""CPU: the host half of tests/test_recurrent_shapes_gpu.py -- its shape table, its types and recurrent_train_support.edges' cells at
time's edges -- built by that module's own functions from seeds alone, and nuclear_sim_amd.recurrent's statement held to its own reference
there, so that a bit mismatch on the device points at the device.  No device.

  * the float32 statement against torch float64 autograd of the same loss at every row, hard gates with relu nets and soft gates with
    tanh nets, with the edge cells in: the pooled distance is at most 1e-3, the limit test_recurrent_train_cpu.py states for it;
  * the CONDITIONS the GPU tests rest on, per row: of each of the r, z and n gate deltas the share of exact zeros lies in [0.1, 0.9] (both
    the clamped and the open branch of the hard gates are taken), the clip fraction strictly between 0 and 1, ``skipped`` is the count
    ``edges`` returns, and the restarts are where it planted them;
  * the narrowing rule: a float64 feature of 1e300 poisons its cell, and the perturbed doubles give the bits of their float32 roundings;
  * t = 1: dW_hh is non-zero exactly through the plants whose ``first`` is non-zero."""
import functools

import numpy as np
import pytest

from nuclear_sim_amd import recurrent
from recurrent_train_support import EDGE_PLANTS, autograd, bits, distance, poisoned_cells, statement
import test_recurrent_shapes_gpu as G

LIMIT = 1e-3      # test_recurrent_train_cpu.py's: the linear rounding bound is far below it at every row, a wrong term errs by order 1
KINDS = [("hard", "relu"), ("soft", "tanh")]


@functools.lru_cache(maxsize=None)
def _reference(row, gates, activation):
    """the row's main run through the statement, once: ``(P, skipped, outputs with the gate deltas)``"""
    t, count, chain = G.MAIN[row]
    P, skipped = G.table_problem(row, t, count, gates, activation)
    return P, skipped, statement(P, plants_per_chain=chain, max_grad_norm=0.0, ent_coef=0.01, keep=True)


@pytest.mark.parametrize("gates, activation", KINDS)
@pytest.mark.parametrize("row", G.ROWS)
def test_the_statement_against_float64_autograd_at_the_table(row, gates, activation):
    P, skipped, out = _reference(row, gates, activation)
    want = autograd(P, ent_coef=0.01)
    d = distance(out["grad"], want)
    print("row %s (%s, %s): pooled |g32 - g64| / |g64| = %.3e" % (row, gates, activation, d))
    assert d <= LIMIT, d
    n_core = recurrent.core_size(P["cells"], P["core"])
    A = P["n_axes"]
    for lo, hi in ((0, n_core), (n_core, P["theta"].size - 2 * A), (P["theta"].size - 2 * A, P["theta"].size - A)):      # the core, the nets, log_std
        assert np.abs(want[lo:hi]).max() > 0 and distance(out["grad"][lo:hi], want[lo:hi]) <= LIMIT, (lo, hi)
    assert out["stats"]["skipped"] == skipped and (out["grad"][-A:] == 0).all()


@pytest.mark.parametrize("row", G.ROWS)
def test_the_conditions_the_gpu_tests_rest_on(row):
    P, skipped, out = _reference(row, "hard", "relu")
    G.conditions(P, skipped, out)
    t, count = P["t"], P["count"]
    bad = poisoned_cells(P)
    assert bad.sum() == skipped and bad[0, 31] and bad[t - 1, 32] and bad[1, count - 1] and bad[2, count - 1]
    assert bad[2, EDGE_PLANTS["restarted"]] and bad[1, EDGE_PLANTS["skipped"]] and np.isnan(P["adv"][1, EDGE_PLANTS["skipped"]])
    assert bad[1, EDGE_PLANTS["wide"]] == (P["obs"].dtype == np.float64)
    assert not bits(out["hidden"][bad]).any() and np.isnan(out["value_new"][bad]).all() and np.isfinite(out["value_new"][~bad]).all()
    for name in ("delta_i", "delta_h"):      # a poisoned cell's own deltas: +0.0
        assert not bits(out[name][bad]).any(), name
    assert P["obs"].dtype == G.TABLE[row][6] and P["act"].dtype == G.TABLE[row][7] and P["adv"].dtype == P["ret"].dtype == G.TABLE[row][8]


def test_the_types_are_mixed_and_half_the_rows_clip_the_value_loss():
    for column in (6, 7, 8):
        kinds = [G.TABLE[row][column] for row in G.ROWS]
        assert kinds.count(np.float64) >= 3 and kinds.count(np.float32) >= 3, column
    assert sum(G.TABLE[row][9] > 0 for row in G.ROWS) == len(G.ROWS) // 2
    for row in G.ROWS:      # the rule of npd_policy_small, and which rows sit on which side of it
        C, K, H, actor, critic = G.TABLE[row][:5]
        small = C * K <= 64 and max(actor + critic) <= 64 and H <= 64
        assert small == (row == "a"), row


@pytest.mark.parametrize("row", ["b", "h"])
def test_the_narrowing_rule(row):
    """the doubles are not floats, their float32 roundings are the draws, and the statement reads the roundings: no bit moves when it is
    handed them instead.  1e300 is finite as a double and poisons its cell"""
    P, skipped, out = _reference(row, "hard", "relu")
    assert P["obs"].dtype == np.float64
    with np.errstate(over="ignore"):
        narrow = P["obs"].astype(np.float32)
    fine = np.isfinite(narrow)
    assert (narrow[fine].astype(np.float64) != P["obs"][fine]).mean() > 0.99 and np.isfinite(P["obs"][1, EDGE_PLANTS["wide"], 0])
    assert np.abs(narrow[fine].astype(np.float64) / P["obs"][fine] - 1.0).max() <= 1e-9 * (1 + 1e-6)
    t, count, chain = G.MAIN[row]
    again = statement(dict(P, obs=narrow), plants_per_chain=chain, max_grad_norm=0.0, ent_coef=0.01)
    for name in ("grad", "logp_new", "value_new", "ratio", "hidden"):
        assert np.array_equal(bits(out[name]), bits(again[name])), name
    cell = (1, EDGE_PLANTS["wide"])
    assert np.isnan(out["value_new"][cell]) and not bits(out["hidden"][cell]).any() and out["hidden"][0, EDGE_PLANTS["wide"]].any()
    # teeth: the other double tensors are read as doubles -- their roundings do move the ratio
    if P["adv"].dtype == np.float64:
        moved = statement(dict(P, adv=P["adv"].astype(np.float32)), plants_per_chain=chain, max_grad_norm=0.0, ent_coef=0.01)
        assert not np.array_equal(bits(out["grad"]), bits(moved["grad"]))


@pytest.mark.parametrize("row", ["b", "g"])
def test_one_slot_has_no_carry(row):
    """t = 1: the only way to W_hh is through ``first`` -- plant 3's is +0.0; with every plant's +0.0, dW_hh is all zeros, by bits, while
    db_hh and the rest still move"""
    P, skipped = G.table_problem(row, 1, 33)
    assert skipped == 0 and not P["first"][3].any()
    cells, H = P["cells"], P["core"]
    lo, hi = 3 * H * cells + 3 * H, 3 * H * cells + 3 * H + 3 * H * H
    out = statement(P, max_grad_norm=0.0, keep=True)
    assert out["grad"][lo:hi].any() and out["delta_h"][0, 3].any()
    alone = statement(dict(P, first=np.zeros_like(P["first"])), max_grad_norm=0.0)
    assert not bits(alone["grad"][lo:hi]).any() and alone["grad"][hi:hi + 3 * H].any() and alone["grad"][:lo].any()
    # plant by plant: with the ``first`` of one plant alone (the first whose gates are not all clamped), W_hh's gradient is that plant's
    # delta_h times its state -- non-zero exactly there
    p = int(np.flatnonzero(out["delta_h"][0].any(axis=1) & P["first"].any(axis=1))[0])
    one = np.zeros_like(P["first"])
    one[p] = P["first"][p]
    single = statement(dict(P, first=one), max_grad_norm=0.0, keep=True)
    want = np.outer(single["delta_h"][0, p] != 0, one[p] != 0)
    assert want.any() and np.array_equal(single["grad"][lo:hi].reshape(3 * H, H) != 0, want)
