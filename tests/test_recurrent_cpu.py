"""CPU: nuclear_sim_amd.recurrent, the numpy statement of the recurrent policy (a GRU cell in front of actor and critic): its soft
gates against torch.nn.GRUCell in torch's own parameter layout, its hard gates at their knees, the restart rule and ``replay`` over a
hand-made rollout, the poison rule, and ``pack`` / ``unpack``.  No device."""
import numpy as np
import pytest
import torch

from nuclear_sim_amd import policy, recurrent


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _nets(rng, H, A, actor=(7,), critic=(5,)):
    def net(dims):
        return [((0.3 * rng.standard_normal((o, i))).astype(np.float32), (0.1 * rng.standard_normal(o)).astype(np.float32)) for i, o in dims]
    a, c = policy.sizes(H, A, actor, critic)
    return net(a), net(c), (0.3 * rng.standard_normal(A) - 0.7).astype(np.float32)


def _core(rng, cells, H, scale=0.4):
    return tuple((scale * rng.standard_normal(shape)).astype(np.float32) for shape in ((3 * H, cells), (3 * H, H), (3 * H,), (3 * H,)))


@pytest.mark.parametrize("H", [6, 33])
@pytest.mark.parametrize("cells", [5, 64])
def test_soft_gates_are_torchs_gru_cell_in_its_own_layout(H, cells):
    """200 random rows: parameters go through ``pack`` in GRUCell's layout and gate order, come back through ``unpack``, and the cell
    agrees with torch's float32 GRUCell on the CPU to 1e-5 absolute -- a swapped gate, block or bias errs by about 0.1"""
    torch.manual_seed(H * 100 + cells)
    gru = torch.nn.GRUCell(cells, H)
    with torch.no_grad():
        for p in gru.parameters():
            p.mul_(2.0)      # (torch's default init is small: make the gates work)
    rng = np.random.default_rng(H + cells)
    a, c, log_std = _nets(rng, H, 2)
    core = tuple(p.detach().numpy() for p in (gru.weight_ih, gru.weight_hh, gru.bias_ih, gru.bias_hh))
    theta = recurrent.pack(a, c, log_std, core=core)
    back = recurrent.unpack(theta, cells, 2, (7,), (5,), core=H)[0]
    x = rng.standard_normal((200, cells)).astype(np.float32)
    h = rng.uniform(-1, 1, (200, H)).astype(np.float32)
    with torch.no_grad():
        want = gru(torch.from_numpy(x), torch.from_numpy(h)).numpy()
    got = recurrent.cell(back, x, h, "soft")
    assert got.dtype == np.float32 and got.shape == (200, H)
    assert np.abs(got - want).max() <= 1e-5, np.abs(got - want).max()
    assert np.abs(want - h).max() > 0.05      # the cell does move its state


def test_hard_gates_saturate_on_both_sides_and_are_exact_at_the_knees():
    f = np.float32
    a = np.array([-1e30, -3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 1e30], dtype=f)
    assert np.array_equal(_bits(recurrent.sigma(a, "hard")), _bits(np.array([0, 0, 0, 0.25, 0.5, 0.75, 1, 1, 1], dtype=f)))      # +0.0, not -0.0
    just = np.array([np.nextafter(f(-2), f(0)), np.nextafter(f(2), f(0))], dtype=f)
    s = recurrent.sigma(just, "hard")
    assert 0 < s[0] < 1e-6 and 1 - 1e-6 < s[1] <= 1      # (0.25f * a + 0.5f just under the upper knee rounds to 1: the sum's own rounding)
    t = np.array([-1e30, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 1e30], dtype=f)
    assert np.array_equal(_bits(recurrent.tau(t, "hard")), _bits(np.array([-1, -1, -1, -0.5, 0, 0.5, 1, 1, 1], dtype=f)))
    inside = np.array([np.nextafter(f(-1), f(0)), np.nextafter(f(1), f(0))], dtype=f)
    assert np.array_equal(_bits(recurrent.tau(inside, "hard")), _bits(inside))
    assert np.isnan(recurrent.sigma(np.array([np.nan], dtype=f), "hard")).all() and np.isnan(recurrent.tau(np.array([np.nan], dtype=f), "hard")).all()
    # the soft sigmoid is written through tanh: 0.5 * tanh(0.5 * a) + 0.5
    v = np.linspace(-6, 6, 41).astype(f)
    assert np.abs(recurrent.sigma(v, "soft") - 1.0 / (1.0 + np.exp(-v.astype(np.float64)))).max() < 2e-7
    # a cell of hard gates, by hand: one input, one hidden cell, weights that put each gate where the arithmetic is exact
    core = (np.array([[1.0], [2.0], [0.5]], dtype=f), np.array([[1.0], [0.0], [2.0]], dtype=f), np.zeros(3, f), np.array([0.0, 0.0, 0.25], dtype=f))
    x, h = np.array([[1.0]], dtype=f), np.array([[0.5]], dtype=f)
    r = 0.25 * (1.0 + 0.5) + 0.5            # 0.875
    z = 1.0                                  # 0.25 * 2 + 0.5
    n = min(1.0, 0.5 + r * (2 * 0.5 + 0.25))  # 0.5 + 0.875 * 1.25 = 1.59 -> 1
    assert recurrent.cell(core, x, h, "hard")[0, 0] == f(n + z * (0.5 - n))


def _policy(rng, n, cells=5, H=6, A=2, gates="hard", **kw):
    a, c, log_std = _nets(rng, H, A)
    P = recurrent.Policy(cells, A, (7,), (5,), "relu", core=H, gates=gates, n=n, **kw)
    P.load(recurrent.pack(a, c, log_std, core=_core(rng, cells, H)))
    return P


def test_replay_reproduces_the_policys_own_states_over_a_termination_a_truncation_and_a_cut():
    """a hand-made rollout of 7 slots and 4 plants: plant 0 runs through, plant 1 terminates behind slot 2 and plant 2 is truncated
    behind slot 4 (their episode index moves), plant 3 is reset by the caller between slots 3 and 4 on a handle without an index of its
    own for it (the index stands, the slot before carries the cut)"""
    rng = np.random.default_rng(5)
    n, T, cells = 4, 7, 5
    P = _policy(rng, n, seed=9)
    P.step(rng.standard_normal((n, cells)), episode=np.zeros(n, np.int32))      # a step before the rollout: `first` is not zeros
    obs = rng.standard_normal((T, n, cells)).astype(np.float32)
    episode, ended = np.zeros((T, n), np.int32), np.zeros((T, n), np.uint8)
    ended[2, 1], ended[4, 2], ended[3, 3] = 1, 2, 4
    episode[3:, 1], episode[5:, 2] = 1, 1
    states, outs, first = [], [], None
    for t in range(T):
        if t == 4:
            P.unprime(np.arange(n) == 3)
        out = P.step(obs[t], episode=episode[t])
        if t == 0:
            first = P.last_start.copy()
        states.append(P.last_start.copy()); outs.append(out)
    states = np.stack(states)
    assert first.any()
    assert not states[3, 1].any() and not states[5, 2].any() and not states[4, 3].any() and states[4, 0].any() and states[3, 3].any()
    got = recurrent.replay(first, obs, episode, ended, P.gru, "hard")
    assert np.array_equal(_bits(got), _bits(states))
    # and the recorded outputs follow from the replayed states
    for t in range(T):
        h2, _ = recurrent.advance(P.gru, obs[t], got[t], "hard")
        assert np.array_equal(_bits(policy.forward(P.nets[1], h2, "relu")[:, 0]), _bits(outs[t][1])), t


def test_values_apply_the_restart_rule_and_remember_nothing():
    rng = np.random.default_rng(6)
    P = _policy(rng, 3)
    x = rng.standard_normal((3, 5))
    P.step(x, episode=np.array([0, 0, 0]))
    h, seen, primed = P.h.copy(), P.seen.copy(), P.primed.copy()
    v = P.values(x, episode=np.array([0, 1, 0]))
    assert np.array_equal(P.h, h) and np.array_equal(P.seen, seen) and np.array_equal(P.primed, primed)
    own = P.values(x, hidden=np.where(np.arange(3)[:, None] == 1, 0, h).astype(np.float32))
    assert np.array_equal(_bits(v), _bits(own)) and v[1] != P.values(x, hidden=h)[1]


def test_a_poisoned_plant_restarts_at_zero_and_moves_no_neighbour():
    rng = np.random.default_rng(7)
    P, Q = _policy(rng, 3, seed=4), None
    rng = np.random.default_rng(7)
    Q = _policy(rng, 3, seed=4)
    x = rng.standard_normal((3, 5))
    bad = x.copy(); bad[1, 2] = np.inf
    ep = np.zeros(3, np.int32)
    P.step(x, ep); Q.step(x, ep)
    a, v, lp = P.step(bad, ep)
    a2, v2, lp2 = Q.step(x, ep)
    assert np.isnan(a[1]).all() and np.isnan(v[1]) and np.isnan(lp[1])
    assert np.array_equal(_bits(P.h[1]), np.zeros(6, np.int32))      # +0.0 in every cell
    for k in (0, 2):
        assert np.array_equal(_bits(P.h[k]), _bits(Q.h[k])) and np.array_equal(_bits(a[k]), _bits(a2[k])) and _bits(v)[k] == _bits(v2)[k]
    a, v, lp = P.step(x, ep)      # the next step: finite again, from a state of zeros
    assert np.isfinite(a).all() and np.isfinite(v).all() and np.isfinite(P.h).all()
    assert np.array_equal(_bits(P.last_start[1]), np.zeros(6, np.int32))


@pytest.mark.parametrize("cells, H, A, actor, critic", [(5, 6, 2, (7,), (5,)), (64, 33, 3, (33, 17), (7, 9, 3)), (256, 128, 8, (128,), (1,))])
def test_pack_and_unpack_round_trip_and_theta_size_matches(cells, H, A, actor, critic):
    rng = np.random.default_rng(cells)
    a, c, log_std = _nets(rng, H, A, actor, critic)
    core = _core(rng, cells, H)
    theta = recurrent.pack(a, c, log_std, core=core)
    assert theta.dtype == np.float32 and theta.size == recurrent.theta_size(cells, A, actor, critic, H)
    assert theta.size == recurrent.core_size(cells, H) + policy.theta_size(H, A, actor, critic)
    g, a2, c2, ls, std = recurrent.unpack(theta, cells, A, actor, critic, H)
    for got, want in zip(g, core):
        assert np.array_equal(got, want)
    for got, want in zip(a2 + c2, a + c):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(ls, log_std) and np.array_equal(std, np.exp(log_std).astype(np.float32))
    # theta's order: W_ih | b_ih | W_hh | b_hh | the nets
    assert np.array_equal(theta[:3 * H * cells], core[0].reshape(-1)) and np.array_equal(theta[3 * H * cells:3 * H * cells + 3 * H], core[2])
    # without a core everything is policy's
    assert recurrent.theta_size(cells, A, actor, critic) == policy.theta_size(cells, A, actor, critic)
    with pytest.raises(ValueError):
        recurrent.unpack(theta[:-1], cells, A, actor, critic, H)
    with pytest.raises(ValueError):
        recurrent.check(cells, A, actor, critic, "relu", 129)
    with pytest.raises(ValueError):
        recurrent.check(cells, A, actor, critic, "relu", H, "firm")
