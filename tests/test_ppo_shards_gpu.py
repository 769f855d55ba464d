"""GPU: training one policy across shards (npb_policy_shard_sums, npb_policy_apply_shards, npb_policy_combine_shards;
BatchedPlantEnv.policy_shard_sums, policy_apply_shards, policy_combine_shards, policy_train(exchange=, shard_cells=)) against
nuclear_sim_amd.ppo.shard_sums and combine, on the bit contracts of test_ppo_gpu.py: a relu net by bits once the statement is fed the
device's ratio (and Adam the device's std), a tanh net device against device.

The shapes are the smallest at which these kernels can go wrong: the small LDS build (64 cells, hidden (64, 64) twice) and the large one
(65 cells, one net 65 wide); 2 and 5 axes; 32, 70 and 97 rows in chains of 32 and 64 (one to four chains, a ragged last tile); 1, 2 and 3
shards.

1. W = 1: shard_sums then apply_shards leaves grad, stats, more, theta, m, v and the padded weights (one forward step's outputs) with the
   bits of the plain gradient and Adam step (what npb_policy_update_more launches) on a second handle loaded alike.
2. policy_shard_sums against ppo.shard_sums by bits: count_total != count, a poisoned row at a tile seam, float and double tensors,
   max_blocks 1 and 0; the handle's grad, stats and more stay as they were.
3. policy_combine_shards against ppo.combine by bits for W = 2 and 3: the crafted order vectors of the CPU suite, both branches of the
   norm clip decided by the total, ent_coef != 0, count_total in stats[7].
4. The gate on the total, between npb_policy_train_begin and _end, on the crafted kl vectors of the CPU suite.
5. Replicas: two handles of 70 and 97 plants, a rollout of T = 3 through the real chain, three updates in lockstep.
6. Accumulation: one handle, two minibatches' sums in the rows of one buffer, one apply.
7. policy_train(exchange=lambda v: v[None], shard_cells=[t * n]) is plain policy_train, by bits."""
import ctypes

import numpy as np
import pytest
import torch

from nuclear_sim_amd import _lib, ppo
from nuclear_sim_amd._lib import NpbError
from test_policy_gpu import F32, F64, _np, _plain, _same, _weights
from test_ppo_gpu import HYPER, _batch, _policy, _to
from test_ppo_options_gpu import GATE, LR, _rolled, _state
from test_ppo_options_gpu import B as TRAIN_B
from test_ppo_shards_cpu import COUNTS, crafted_gate, crafted_order

pytestmark = pytest.mark.gpu

SMALL = dict(C=16, K=4, actor=(64, 64), critic=(64, 64))      # 64 cells: the small LDS build
LARGE = dict(C=13, K=5, actor=(65,), critic=(7,))             # 65 cells and a net 65 wide: the large one
_NP = {F32: np.float32, F64: np.float64}
CLIP_VF = 0.2
ADAM = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-5)


def _make(shape, A, activation, seed, fdtype=F32, cdtype=F32):
    return _policy(shape["C"], shape["K"], fdtype, shape["actor"], shape["critic"], A, cdtype, activation, seed)


def _rows(env, seed, count, activation, fdtype=F32, cdtype=F32, adtype=F32, poison=False):
    """a host minibatch around the env's theta with its old values; ``poison``: a NaN advantage and an infinite feature at the seam of the
    first two tiles (the last row of a batch of 32)"""
    batch = _batch(seed, _np(env.policy_theta()), count, env.policy_spec(), activation, fdtype, cdtype, adtype)
    old = (batch["ret"] + 0.3 * np.random.default_rng(seed + 1).standard_normal(count)).astype(np.float32)
    if poison:
        batch["adv"][31] = np.nan
        if count > 32:
            batch["obs"][32, 3] = np.inf
    return batch, old


def _handle(env):
    """grad, stats and more as they stand on the handle"""
    n = env.policy_theta().numel()
    with torch.cuda.device(env.device):
        out = [torch.zeros(n, dtype=F32, device=env.device), torch.zeros(8, dtype=F64, device=env.device), torch.zeros(4, dtype=F64, device=env.device)]
    for t, f in zip(out, (env.L.npb_policy_get_grad, env.L.npb_policy_get_stats, env.L.npb_policy_get_stats_more)):
        assert f(env._h, ctypes.c_void_p(t.data_ptr()), env._stream()) == 0
    return [_np(t) for t in out]


def _ratio(env, batch, chain, old):
    """the device's own ratio of these rows (a plain gradient with diagnostics)"""
    return _np(env.policy_grad(_to(env, batch), rows_per_chain=chain, diagnostics=True, clip_vf=CLIP_VF, value_old=torch.as_tensor(old), **HYPER)["ratio"])


def _want_sums(env, batch, old, chain, count_total, ratio, theta=None):
    S = env.policy_spec()
    return ppo.shard_sums(_np(env.policy_theta()) if theta is None else theta, S["cells"], S["n_axes"], S["actor"], S["critic"], S["activation"],
                          count_total=count_total, clip=HYPER["clip"], vf_coef=HYPER["vf_coef"], rows_per_chain=chain, ratio=ratio, value_old=old,
                          clip_vf=CLIP_VF, **batch)


def _got_sums(env, batch, old, chain, count_total, **kw):
    return env.policy_shard_sums(_to(env, batch), count_total, clip=HYPER["clip"], vf_coef=HYPER["vf_coef"], rows_per_chain=chain, clip_vf=CLIP_VF,
                                 value_old=torch.as_tensor(old), **kw)


def _stats(stats, more):
    return np.array([stats[k] for k in ppo.STATS]), np.array([more[k] for k in ppo.STATS_MORE])


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("shape, A, activation, count, chain", [(SMALL, 2, "relu", 70, 32), (SMALL, 5, "tanh", 97, 64), (LARGE, 5, "relu", 97, 32),
                                                             (LARGE, 2, "tanh", 70, 64)])
def test_one_shard_is_the_plain_update_bit_for_bit(shape, A, activation, count, chain):
    one, two = _make(shape, A, activation, 7), _make(shape, A, activation, 7)
    batch, old = _rows(one, 3, count, activation)
    _same(one.policy_theta(), two.policy_theta(), "loaded alike")
    for k in range(2):      # (Adam's first step from zero, and one from a state)
        two.policy_grad(_to(two, batch), rows_per_chain=chain, clip_vf=CLIP_VF, value_old=torch.as_tensor(old), **HYPER)
        two.policy_adam(**ADAM)
        vec = _got_sums(one, batch, old, chain, count)
        assert vec.shape == (one.policy_shard_size(),) == (ppo.shard_size(one.policy_theta().numel(), A),) and vec.dtype == F64
        one.policy_apply_shards(vec[None], count, HYPER["ent_coef"], HYPER["max_grad_norm"], **ADAM)
        for got, want, name in zip(_handle(one), _handle(two), ("grad", "stats", "more")):
            _same(got, want, (k, name))
        for got, want, name in zip(_state(one), _state(two), ("theta", "m", "v", "step")):
            _same(np.asarray(got), np.asarray(want), (k, name))
    assert _state(one)[3] == 2 and _state(one)[1].any()
    a, b = one.step(), two.step()      # the repack ran: the next step reads the new weights
    _same(a[0], b[0], "obs"); _same(one.controls_input(), two.controls_input(), "act")
    _same(one.policy_outputs()["value"], two.policy_outputs()["value"], "value"); _same(one.policy_outputs()["logp"], two.policy_outputs()["logp"], "logp")
    one.close(); two.close()


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("shape, A, count, chain, fdtype, cdtype, adtype", [
    (SMALL, 2, 32, 32, F32, F32, F32), (LARGE, 5, 32, 64, F64, F64, F64), (SMALL, 5, 70, 32, F64, F32, F64), (LARGE, 2, 70, 64, F32, F64, F32),
    (LARGE, 5, 97, 32, F32, F32, F64), (SMALL, 2, 97, 64, F64, F64, F32)])
def test_shard_sums_against_the_statement_bit_for_bit(shape, A, count, chain, fdtype, cdtype, adtype):
    """Fails without the feature: policy_shard_sums does not exist"""
    env = _make(shape, A, "relu", count + A, fdtype, cdtype)
    batch, old = _rows(env, count, count, "relu", fdtype, cdtype, adtype, poison=True)
    total = count + 102
    ratio = _ratio(env, batch, chain, old)
    before = _handle(env)
    want = _want_sums(env, batch, old, chain, total, ratio)
    P = want.size - 18
    assert np.isfinite(want).all() and want[:P].any() and want[P + 11] == (1 if count == 32 else 2) and not want[P + A:P + 8].any()
    own = _want_sums(env, batch, old, chain, count, ratio)
    assert not np.array_equal(want[:P], own[:P])      # (the divisor is in the bits)
    for blocks in (1, 0):
        _same(_got_sums(env, batch, old, chain, total, max_blocks=blocks), want, ("sums", blocks))
    with torch.cuda.device(env.device):      # into a row of a larger buffer: the rows beside it stay
        buf = torch.full((3, want.size), 7.0, dtype=F64, device=env.device)
    assert _got_sums(env, batch, old, chain, total, out=buf[1]) is not None
    _same(buf[1], want, "a row of a buffer"); assert (_np(buf[0]) == 7.0).all() and (_np(buf[2]) == 7.0).all()
    for got, was, name in zip(_handle(env), before, ("grad", "stats", "more")):
        _same(got, was, name + " left as it was")
    # refusals, by name
    with pytest.raises(NpbError, match="npb_policy_shard_sums: count_total < desc->count"):
        _got_sums(env, batch, old, chain, count - 1, out=buf[1])
    with pytest.raises(ValueError, match="contiguous float64"):
        _got_sums(env, batch, old, chain, total, out=buf[:, 0])
    d, held = env._ppo_desc(_to(env, batch), rows_per_chain=chain, max_blocks=0, **HYPER)
    m = _lib.NpbPpoMore()
    m.kl_limit = 0.03
    assert env.L.npb_policy_shard_sums(env._h, ctypes.byref(d), ctypes.byref(m), total, ctypes.c_void_p(buf.data_ptr()), env._stream()) != 0
    assert b"npb_policy_shard_sums: kl_limit > 0: the gate belongs to the combine" in env.L.npb_last_error(env._h)
    assert env.L.npb_policy_shard_sums(env._h, ctypes.byref(d), None, total, None, env._stream()) != 0
    assert b"npb_policy_shard_sums: a NULL or misaligned out" in env.L.npb_last_error(env._h)
    assert env.L.npb_policy_shard_sums(env._h, ctypes.byref(d), None, total, ctypes.c_void_p(buf.data_ptr() + 4), env._stream()) != 0
    assert b"npb_policy_shard_sums: a NULL or misaligned out" in env.L.npb_last_error(env._h)
    _same(buf[1], want, "a refused call writes nothing")
    env.set_policy(None)
    assert env.L.npb_policy_shard_sums(env._h, ctypes.byref(d), None, total, ctypes.c_void_p(buf.data_ptr()), env._stream()) != 0
    assert b"npb_policy_shard_sums: no policy set" in env.L.npb_last_error(env._h)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def _combine_both(env, vectors, count_total, ent_coef, max_grad_norm, what):
    A = env.policy_spec()["n_axes"]
    got = env.policy_combine_shards(torch.as_tensor(vectors).to(env.device), count_total, ent_coef, max_grad_norm)
    grad, stats, more = ppo.combine(vectors, _np(env.policy_theta()), A, count_total, ent_coef=ent_coef, max_grad_norm=max_grad_norm)
    s, m = _stats(stats, more)
    _same(got["grad"], grad, (what, "grad")); _same(got["stats"], s, (what, "stats")); _same(got["more"], m, (what, "more"))
    assert s[7] == count_total and not grad[-A:].any()
    return grad, stats


@pytest.mark.parametrize("shape, A", [(SMALL, 2), (LARGE, 5)])
def test_combine_shards_against_the_statement_bit_for_bit(shape, A):
    env = _make(shape, A, "relu", 5)
    n = sum(COUNTS)
    vectors = []
    for w, count in enumerate(COUNTS):      # 70, 97 and 32 rows: the device's own vectors
        batch, old = _rows(env, 20 + w, count, "relu")
        vectors.append(_np(_got_sums(env, batch, old, 32, n)))
    vectors = np.stack(vectors)
    theta = _np(env.policy_theta())
    for W in (2, 3):
        v, total = vectors[:W], sum(COUNTS[:W])
        norm = ppo.combine(v, theta, A, total, ent_coef=0.01, max_grad_norm=0.0)[1]["grad_norm"]
        largest = max(ppo.combine(v[w:w + 1], theta, A, total, ent_coef=0.01, max_grad_norm=0.0)[1]["grad_norm"] for w in range(W))
        print("W = %d: the total's norm %.4f, the largest shard's own %.4f" % (W, norm, largest))
        assert norm > largest
        between = 0.5 * (norm + largest)
        clipped, stats = _combine_both(env, v, total, 0.01, between, (W, "clipped by the total alone"))
        assert stats["grad_norm"] == norm
        free, _ = _combine_both(env, v, total, 0.01, 2.0 * norm, (W, "not clipped"))
        off, _ = _combine_both(env, v, total, 0.3, 0.0, (W, "the clip off, another ent_coef"))
        assert not np.array_equal(clipped, free) and np.array_equal(free[:-2 * A], off[:-2 * A]) and not np.array_equal(free[-2 * A:-A], off[-2 * A:-A])
    # the order: the crafted vectors of the CPU suite, and the same shards in another order give other bits
    crafted = crafted_order(theta.size, A)
    grad, _ = _combine_both(env, crafted, n, 0.25, 0.0, "crafted")
    assert grad[0] == 0.0
    other, _ = _combine_both(env, crafted[[0, 2, 1]], n, 0.25, 0.0, "crafted, permuted")
    assert other[0] == 1.0
    with pytest.raises(NpbError, match="npb_policy_combine_shards: kl_limit > 0"):
        s = env._ppo_shards(torch.as_tensor(crafted).to(env.device), n, 0.0, 0.5, 0.03)
        _lib.check(env.L.npb_policy_combine_shards(env._h, ctypes.byref(s), env._stream()), env._h)
    with pytest.raises(ValueError, match="contiguous float64"):
        env.policy_combine_shards(torch.as_tensor(crafted[:, :-1]).to(env.device), n)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_the_gate_follows_the_total_between_begin_and_end():
    A = 3
    env = _policy(5, 3, F32, (7,), (7,), A, F32, "relu", 2)
    n = sum(COUNTS)
    C = crafted_gate(env.policy_theta().numel(), A)
    limit = C["limit"]
    dev = {k: torch.as_tensor(C[k][0]).to(env.device) for k in ("total", "shard", "nan")}
    # a first ungated update, so that the pair starts from a state: step0 = 1
    env.policy_apply_shards(dev["shard"], n, 0.01, 0.5, **ADAM)
    theta, m, v, step0 = _state(env)
    assert step0 == 1
    with pytest.raises(NpbError, match="npb_policy_apply_shards: kl_limit > 0 outside npb_policy_train_begin"):
        env.policy_apply_shards(dev["shard"], n, 0.01, 0.5, kl_limit=limit, **ADAM)
    assert env.L.npb_policy_train_begin(env._h, env._stream()) == 0
    with pytest.raises(NpbError, match="npb_policy_apply_shards: kl_limit == 0 between npb_policy_train_begin and npb_policy_train_end"):
        env.policy_apply_shards(dev["shard"], n, 0.01, 0.5, **ADAM)
    stopped, step = False, step0
    for i, name in enumerate(("shard", "nan", "total", "shard")):      # applied, applied (a NaN does not stop), stopped, stopped for good
        before = _np(env.policy_theta())
        env.policy_apply_shards(dev[name], n, 0.01, 0.5, kl_limit=limit, **ADAM)
        grad, stats, more = ppo.combine(C[name][0], before, A, n, ent_coef=0.01, max_grad_norm=0.5, stopped=stopped, kl_limit=limit)
        stopped = bool(more["stopped"])
        assert stopped == (i >= 2)
        got = _handle(env)
        s, mo = _stats(stats, more)
        _same(got[0], grad, (name, "grad")); _same(got[1], s, (name, "stats")); _same(got[2], mo, (name, "more"))
        now = _np(env.policy_theta())
        if stopped:
            _same(now, before, (name, "an update that is not applied leaves theta and std"))
        else:
            theta, m, v, step = ppo.adam(theta, m, v, step, grad, A, std=now[-A:], **ADAM)
            _same(now, theta, (name, "theta"))
    applied = ctypes.c_uint32(99)
    assert env.L.npb_policy_train_end(env._h, ctypes.byref(applied), env._stream()) == 0      # the one read-back
    assert applied.value == 2
    end = _state(env)
    assert end[3] == step0 + 2 == step
    _same(end[0], theta, "theta"); _same(end[1], m, "m"); _same(end[2], v, "v")
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def _replica(n, seed, T=3):
    env = _plain(n)
    env.set_rollout(T, extras=2)
    a, c, log_std = _weights(8, 15, 3, (33, 17), (7,))
    env.set_policy(a, c, log_std, activation="relu", seed=seed, extras=("value", "logp"))
    env.collect(T)
    env.rollout_advantages(0.99, 0.95, values=("extra", 0), last_value=env.policy_values())
    return env


def test_two_replicas_stay_bit_equal_through_three_updates():
    A, T, chain = 3, 3, 64
    envs = [_replica(70, 21), _replica(97, 5)]
    _same(envs[0].policy_theta(), envs[1].policy_theta(), "one policy")
    S = envs[0].policy_spec()
    theta = _np(envs[0].policy_theta())
    m, v, step = np.zeros_like(theta), np.zeros_like(theta), 0
    streams = [iter(e.rollout_minibatches(e.n, 1, seed=3 + i)) for i, e in enumerate(envs)]      # T * n cells in batches of n: three updates
    L = envs[0].policy_shard_size()
    for update in range(3):
        batches = [next(s) for s in streams]
        total = sum(b["adv"].numel() for b in batches)
        assert total == 167
        with torch.cuda.device(envs[0].device):
            every = torch.zeros((2, L), dtype=F64, device=envs[0].device)
        want = []
        for w, (env, batch) in enumerate(zip(envs, batches)):
            count = batch["adv"].numel()
            host = {k: _np(batch[k]) for k in ("act", "adv", "ret")}
            host["obs"], host["logp_old"] = _np(batch["obs"]).reshape(count, -1), _np(batch["extra"])[:, 1]
            ratio = _np(env.policy_grad(batch, rows_per_chain=chain, diagnostics=True, **HYPER)["ratio"])
            env.policy_shard_sums(batch, total, HYPER["clip"], HYPER["vf_coef"], chain, out=every[w])
            want.append(ppo.shard_sums(theta, S["cells"], A, S["actor"], S["critic"], "relu", count_total=total, clip=HYPER["clip"], vf_coef=HYPER["vf_coef"],
                                       rows_per_chain=chain, ratio=ratio, **host))
        _same(every, np.stack(want), (update, "the two vectors"))
        for env in envs:
            env.policy_apply_shards(every, total, HYPER["ent_coef"], HYPER["max_grad_norm"], **ADAM)
        states = [_state(e) for e in envs]
        for a, b, name in zip(states[0], states[1], ("theta", "m", "v", "step")):
            _same(np.asarray(a), np.asarray(b), (update, name, "replica against replica"))
        grad, _, _ = ppo.combine(np.stack(want), theta, A, total, ent_coef=HYPER["ent_coef"], max_grad_norm=HYPER["max_grad_norm"])
        theta, m, v, step = ppo.adam(theta, m, v, step, grad, A, std=states[0][0][-A:], **ADAM)
        _same(states[0][0], theta, (update, "theta")); _same(states[0][1], m, (update, "m")); _same(states[0][2], v, (update, "v"))
        assert states[0][3] == step == update + 1
    for e in envs:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_one_handle_accumulates_two_minibatches_into_one_step():
    A, chain = 5, 32
    env = _make(LARGE, A, "relu", 9)
    S, theta = env.policy_spec(), _np(env.policy_theta())
    n = 70 + 97
    with torch.cuda.device(env.device):
        buf = torch.zeros((2, env.policy_shard_size()), dtype=F64, device=env.device)
    want = []
    for w, count in enumerate((70, 97)):
        batch, old = _rows(env, 40 + w, count, "relu")
        ratio = _ratio(env, batch, chain, old)
        _got_sums(env, batch, old, chain, n, out=buf[w])
        want.append(_want_sums(env, batch, old, chain, n, ratio))
    _same(buf, np.stack(want), "the two rows")
    env.policy_apply_shards(buf, n, HYPER["ent_coef"], HYPER["max_grad_norm"], **ADAM)
    grad, stats, more = ppo.combine(np.stack(want), theta, A, n, ent_coef=HYPER["ent_coef"], max_grad_norm=HYPER["max_grad_norm"])
    got = _handle(env)
    s, mo = _stats(stats, more)
    _same(got[0], grad, "grad"); _same(got[1], s, "stats"); _same(got[2], mo, "more")
    assert s[7] == n and stats["skipped"] == 0
    now, m, v, step = _state(env)
    t2, m2, v2, step2 = ppo.adam(theta, np.zeros_like(theta), np.zeros_like(theta), 0, grad, A, std=now[-A:], **ADAM)
    assert step == step2 == 1
    _same(now, t2, "theta"); _same(m, m2, "m"); _same(v, v2, "v")
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "target_kl"])
def test_policy_train_through_an_exchange_of_one_is_policy_train(gated):
    kw = dict(dict(HYPER, lr=LR, **GATE), more=True)
    plain = _rolled()
    cells = 8 * plain.n
    if gated:      # a limit the third of the four updates crosses
        kl = _np(plain.policy_train(TRAIN_B, 2, seed=3, **kw)[0])[:, ppo.STATS.index("approx_kl")]
        plain.close()
        plain = _rolled()
        kw["target_kl"] = (0.5 * (kl[1] + kl[2])) / 1.5
    want = plain.policy_train(TRAIN_B, 2, seed=3, **kw)
    sharded = _rolled()
    seen = []

    def exchange(vec):
        seen.append(vec.shape)
        return vec[None]
    with pytest.raises(ValueError, match="different numbers of updates"):      # before any device work: the handle is untouched
        sharded.policy_train(TRAIN_B, 2, seed=3, exchange=exchange, shard_cells=[cells, TRAIN_B], **kw)
    with pytest.raises(ValueError, match="both, or neither"):
        sharded.policy_train(TRAIN_B, 2, seed=3, exchange=exchange, **kw)
    assert not seen and _state(sharded)[3] == 0
    got = sharded.policy_train(TRAIN_B, 2, seed=3, exchange=exchange, shard_cells=[cells], **kw)
    assert seen == [(sharded.policy_shard_size(),)] * 4
    _same(got[0], want[0], "stats"); _same(got[1], want[1], "more")
    if gated:
        assert _np(got[1])[:, 2].tolist() == [1, 1, 0, 0]
    for a, b, name in zip(_state(sharded), _state(plain), ("theta", "m", "v", "step")):
        _same(np.asarray(a), np.asarray(b), name)
    assert _state(sharded)[3] == (2 if gated else 4)
    plain.close(); sharded.close()
