"""CPU: nuclear_sim_amd.recurrent's statement of training through time (``gradient``, ``shard_sums``, ``cell_keep``): it is the right
gradient -- float32 against torch float64 autograd of the same loss, soft gates with tanh nets and hard gates with relu nets -- and it
keeps its invariants: the combine of one shard is the gradient, a restart cuts the sequence, a poisoned cell passes no carry and a
skipped one does, and the chains pin only the order of the sums.  No device.

The shape: t = 6 slots, 40 plants (a ragged second tile), K * C = 6, H = 5, actor (7,), critic (9, 6), A = 3."""
import numpy as np
import pytest

from nuclear_sim_amd import ppo, recurrent
from recurrent_train_support import CUT, autograd, bits, distance, problem, statement

T, COUNT, CELLS, H, A, ACTOR, CRITIC = 6, 40, 6, 5, 3, (7,), (9, 6)
# the linear rounding bound eps_f32 * t * (K * C + H + the widths) is about 7e-5 here; a wrong term errs by order 1
LIMIT = 1e-3


def _problem(gates="hard", activation="relu", seed=5, **kw):
    return problem(seed, T, COUNT, CELLS, H, A, ACTOR, CRITIC, gates, activation, **kw)


@pytest.mark.parametrize("gates, activation", [("soft", "tanh"), ("hard", "relu")])
def test_float32_statement_against_float64_autograd(gates, activation):
    P = _problem(gates, activation)
    out = statement(P, max_grad_norm=0.0, ent_coef=0.01)
    want = autograd(P, ent_coef=0.01)
    assert out["grad"].dtype == np.float32 and out["grad"].shape == P["theta"].shape
    d = distance(out["grad"], want)
    print("pooled |g32 - g64| / |g64| (%s, %s): %.3e" % (gates, activation, d))
    assert d <= LIMIT, d
    # every block of theta on its own: the core's four and the rest
    n_core = recurrent.core_size(CELLS, H)
    edges = [0, 3 * H * CELLS, 3 * H * CELLS + 3 * H, n_core - 3 * H, n_core, P["theta"].size - 2 * A, P["theta"].size - A]
    for lo, hi in zip(edges[:-1], edges[1:]):
        assert np.abs(want[lo:hi]).max() > 0 and distance(out["grad"][lo:hi], want[lo:hi]) <= LIMIT, (lo, hi)
    assert out["stats"]["skipped"] == 2.0 and out["stats"]["count"] == T * COUNT
    assert (out["grad"][-A:] == 0).all()


def test_cell_keep_is_cell():
    P = _problem("soft", "tanh")
    core = recurrent.unpack(P["theta"], CELLS, A, ACTOR, CRITIC, H)[0]
    x, h = P["obs"][0], P["first"]
    K = recurrent.cell_keep(core, x, h, "soft")
    assert np.array_equal(bits(K["h2"]), bits(recurrent.cell(core, x, h, "soft")))
    assert set(K) == {"h2", "gi", "gh", "r", "z", "n", "ar", "az", "an"} and K["gi"].shape == (COUNT, 3 * H) and K["an"].shape == (COUNT, H)


@pytest.mark.parametrize("clip_vf", [0.0, 0.2])
def test_combine_of_one_shard_is_the_gradient_by_bits(clip_vf):
    P = _problem()
    kw = dict(value_old=P["value_old"], clip_vf=clip_vf)
    out = statement(P, ent_coef=0.01, **kw)
    vec = statement(P, recurrent.shard_sums, count_total=T * COUNT, **kw)
    g, stats, more = ppo.combine(vec[None], P["theta"], A, T * COUNT, ent_coef=0.01)
    assert np.array_equal(bits(g), bits(out["grad"]))
    for name in ppo.STATS:
        assert bits(np.float64(stats[name])) == bits(np.float64(out["stats"][name])), name
    for name in ppo.STATS_MORE:
        assert bits(np.float64(more[name])) == bits(np.float64(out["more"][name])), name
    # a shard of a larger update divides its seeds by the whole count
    half = statement(P, recurrent.shard_sums, count_total=2 * T * COUNT, **kw)
    n_w = P["theta"].size - 2 * A
    assert np.allclose(half[:n_w], 0.5 * vec[:n_w], rtol=1e-5, atol=1e-12) and not np.array_equal(half[:n_w], vec[:n_w])


def _tail(P, plant, s0):
    """slots s0.. of one plant as a sequence of their own, from first = +0.0"""
    Q = dict(P, t=P["t"] - s0, count=1, first=np.zeros((1, H), np.float32))
    for name in ("obs", "act", "logp_old", "adv", "ret", "episode", "ended", "value_old"):
        Q[name] = P[name][s0:, plant:plant + 1]
    return Q


@pytest.mark.parametrize("kind", ["episode", "cut"])
def test_a_restart_cuts_the_sequence(kind):
    """the plant restarting in front of slot 3 has, for slots 3.., the logp_new / value_new bits of the same slots run as their own
    sequence from first = 0"""
    P = _problem(special=False)
    if kind == "episode":
        P["episode"][3:, 7] += 1
    else:
        P["ended"][2, 7] |= CUT
    out, alone = statement(P), statement(_tail(P, 7, 3))
    for name in ("logp_new", "value_new"):
        assert np.array_equal(bits(out[name][3:, 7]), bits(alone[name][:, 0])), name
    assert np.array_equal(bits(out["hidden"][3:, 7]), bits(alone["hidden"][:, 0]))
    # teeth: without the restart the state flows on
    Q = _problem(special=False)
    assert not np.array_equal(bits(statement(Q)["value_new"][3:, 7]), bits(alone["value_new"][:, 0]))
    # and the gradient sees the cut: later slots' advantages move no gate delta in front of it
    base = statement(P, keep=True)
    Q = dict(P, adv=P["adv"].copy())
    Q["adv"][3:, 7] *= -3.0
    moved = statement(Q, keep=True)
    for name in ("delta_i", "delta_h"):
        assert np.array_equal(bits(base[name][:3, 7]), bits(moved[name][:3, 7])) and not np.array_equal(bits(base[name][3:, 7]), bits(moved[name][3:, 7]))


def test_poisoned_and_skipped_cells():
    P = _problem()
    out = statement(P, keep=True)
    for name in ("logp_new", "value_new", "ratio"):
        assert np.isnan(out[name][2, 4]) and np.isnan(out[name][1, 5]), name
        assert np.isfinite(np.delete(out[name].reshape(-1), [2 * COUNT + 4, 1 * COUNT + 5])).all(), name
    assert (out["hidden"][2, 4] == 0).all() and np.isfinite(out["hidden"]).all()
    assert out["stats"]["skipped"] == 2.0 and np.isfinite(out["grad"]).all()
    assert not bits(out["delta_i"][2, 4]).any() and not bits(out["delta_h"][2, 4]).any()      # the poisoned cell's own deltas: +0.0
    assert np.abs(out["delta_i"][1, 5]).max() > 0                                              # the skipped cell's: the carry's
    # later slots' adv, perturbed: behind the poisoned cell no bit of the plant's earlier gate deltas changes; through the skipped one
    # the carry flows
    Q = dict(P, adv=P["adv"].copy())
    Q["adv"][3:, 4] *= -2.5
    Q["adv"][2:, 5] *= -2.5
    moved = statement(Q, keep=True)
    for name in ("delta_i", "delta_h"):
        assert np.array_equal(bits(out[name][:3, 4]), bits(moved[name][:3, 4])), name
        assert not np.array_equal(bits(out[name][3:, 4]), bits(moved[name][3:, 4])), name
        assert not np.array_equal(bits(out[name][:2, 5]), bits(moved[name][:2, 5])), name
        others = np.delete(np.arange(COUNT), [4, 5])
        assert np.array_equal(bits(out[name][:, others]), bits(moved[name][:, others])), name


def test_poisoned_cell_stops_the_carry_by_bits():
    """the direct form of the same: cell_back on a poisoned cell gives +0.0 for every gate delta and the carry, whatever dh' is"""
    P = _problem()
    core = recurrent.unpack(P["theta"], CELLS, A, ACTOR, CRITIC, H)[0]
    x, h = np.nan_to_num(P["obs"][2]), P["first"]
    K = recurrent.cell_keep(core, x, h, "hard")
    bad = np.zeros(COUNT, dtype=bool)
    bad[4] = True
    rng = np.random.default_rng(0)
    outs = [recurrent.cell_back(core, K, rng.standard_normal((COUNT, H)).astype(np.float32), h, bad, "hard") for _ in range(2)]
    for v in outs[0]:
        assert np.array_equal(bits(v[4]), np.zeros_like(bits(v[4])))      # +0.0, not -0.0
        assert np.abs(np.delete(v, 4, axis=0)).max() > 0
    assert not np.array_equal(bits(outs[0][2][5]), bits(outs[1][2][5]))


def test_chains_pin_the_order_of_the_sums_and_nothing_else():
    P = _problem()
    a, b = statement(P, plants_per_chain=32), statement(P, plants_per_chain=64)
    assert len(recurrent.order(T, COUNT, 32)[0]) == 2 * 32 * T and len(recurrent.order(T, COUNT, 64)[0]) == 64 * T
    for name in ("logp_new", "value_new", "ratio", "hidden"):
        assert np.array_equal(bits(a[name]), bits(b[name])), name
    assert not np.array_equal(bits(a["grad"]), bits(b["grad"])) and distance(a["grad"], b["grad"]) < 1e-5
    rows, rpc = recurrent.order(2, 33, 32)
    assert rpc == 64 and list(rows[:3]) == [33, 34, 35] and list(rows[32:35]) == [0, 1, 2] and list(rows[64:68]) == [65, 32, -1, -1]
    with pytest.raises(ValueError, match="multiple of 32"):
        statement(P, plants_per_chain=48)
