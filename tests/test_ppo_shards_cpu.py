"""CPU: one policy across shards, the statement (nuclear_sim_amd.ppo.shard_sums, combine; nuclear_sim_amd.sharding.gather_shard_sums).

1. ``combine(shard_sums(count_total=count)[None])`` has the bits of ``gradient``: grad, every stat and every ``more``.
2. The divisor: 199 rows cut into shards of 70, 97 and 32 with ``count_total = 199``; the combined, unclipped gradient may stand at most
   2 times as far from the float64 autograd of the loss over the whole batch as ``ppo.gradient`` over the whole batch does.  Why 2: the
   only new roundings are W - 1 double additions per entry, replacing chain additions already there, so the ratio should sit near 1.
   Measured: relu 1.00 (6.686e-07 / 6.686e-07), tanh 1.07 (3.870e-07 / 3.615e-07).
3. Order: crafted vectors with entries ``1e16, 1.0, -1e16`` over three shards: a permutation of the shards changes the bits, and
   ``combine`` returns those of the ascending order.
4. The gate follows the total.  A shard's own decision would be ``kl_w / count_w > kl_limit``; the total's is ``(kl_0 + kl_1 + kl_2) /
   count_total > kl_limit``.  In exact arithmetic the total cannot cross when no shard does (the sum of the bounds is the bound of the
   sum), so that direction exists at the level of the roundings only: every ``kl_w`` is the largest double whose own mean does not
   cross, and the total's mean then does.  The other way round is ordinary: one shard far across, the total not.
5. World size 2 over gloo: both ranks end with bit-equal theta, m and v, those of one process that combines the two vectors."""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from nuclear_sim_amd import ppo
from test_ppo_cpu import CLIP, ENT, VF, autograd, make_batch, make_theta, pooled, split

SMALL = (64, (64, 64), (64, 64))      # cells, actor, critic: the small LDS build of the device (K * C = 64, widths <= 64)
LARGE = (65, (65,), (7,))             # the large build: 65 cells and one net 65 wide
HYPER = dict(clip=CLIP, vf_coef=VF)
COUNTS = (70, 97, 32)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what


def _problem(seed, n, cells, actor, critic, A, activation):
    rng = np.random.default_rng(seed)
    theta = make_theta(rng, cells, A, actor, critic)
    return theta, make_batch(rng, theta, n, cells, A, actor, critic, activation)


def _cut(batch, lo, hi, **more):
    out = {k: v[lo:hi] for k, v in batch.items()}
    out.update({k: v[lo:hi] for k, v in more.items() if v is not None})
    return out


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("shape, A, n, chain, activation, clip_vf, poison", [
    (SMALL, 2, 70, 32, "relu", 0.0, False), (SMALL, 5, 97, 64, "tanh", 0.2, False), (LARGE, 5, 70, 32, "relu", 0.2, True),
    (LARGE, 2, 97, 64, "tanh", 0.0, True), (LARGE, 2, 32, 32, "relu", 0.2, False)])
def test_one_shard_of_the_whole_update_combines_to_the_gradients_bits(shape, A, n, chain, activation, clip_vf, poison):
    """Fails without the feature: the statement has no shard_sums"""
    cells, actor, critic = shape
    theta, batch = _problem(n + A, n, cells, actor, critic, A, activation)
    value_old = (batch["ret"] + 0.3 * np.random.default_rng(1).standard_normal(n)).astype(np.float32) if clip_vf else None
    if poison:
        batch["adv"][31], batch["obs"][32, 3] = np.nan, np.inf      # (a tile seam)
    kw = dict(HYPER, rows_per_chain=chain, value_old=value_old, clip_vf=clip_vf)
    want = ppo.gradient(theta, cells, A, actor, critic, activation, ent_coef=ENT, max_grad_norm=0.5, **batch, **kw)
    vec = ppo.shard_sums(theta, cells, A, actor, critic, activation, count_total=n, **batch, **kw)
    assert vec.dtype == np.float64 and vec.shape == (ppo.shard_size(theta.size, A),) == (theta.size - 2 * A + 18,)
    assert not vec[theta.size - 2 * A + A:theta.size - 2 * A + 8].any()      # dls beyond A: +0.0
    grad, stats, more = ppo.combine(vec[None], theta, A, n, ent_coef=ENT, max_grad_norm=0.5)
    _same(grad, want["grad"], "grad")
    for k in ppo.STATS:
        _same(np.float64(stats[k]), np.float64(want["stats"][k]), k)
    for k in ppo.STATS_MORE:
        _same(np.float64(more[k]), np.float64(want["more"][k]), k)
    assert stats["skipped"] == (2 if poison else 0) and stats["count"] == n and stats["grad_norm"] > 0
    if clip_vf:
        assert 0 < more["vf_clip_fraction"] < 1
    # the gate's two words too, from a stopped start and across a limit
    for stopped, limit in ((True, 10.0), (False, 1e-9), (False, 10.0)):
        w = ppo.gradient(theta, cells, A, actor, critic, activation, ent_coef=ENT, stopped=stopped, kl_limit=limit, **batch, **kw)["more"]
        g = ppo.combine(vec[None], theta, A, n, ent_coef=ENT, stopped=stopped, kl_limit=limit)[2]
        assert (g["applied"], g["stopped"]) == (w["applied"], w["stopped"])


def test_the_vectors_rows_are_the_devices_order():
    assert ppo.SHARD_ROWS[8:] == ("policy_loss", "kl", "clipped", "skipped", "value_loss", "vf_clipped", "ret", "ret2", "diff", "diff2")
    assert len(ppo.SHARD_ROWS) == 18 and ppo.shard_size(100, 3) == 112 and ppo.SHARDS_MAX == 64
    theta, batch = _problem(3, 40, 15, (7,), (7,), 3, "relu")
    with pytest.raises(ValueError, match="count_total"):
        ppo.shard_sums(theta, 15, 3, (7,), (7,), "relu", count_total=39, **batch)
    vec = ppo.shard_sums(theta, 15, 3, (7,), (7,), "relu", count_total=40, **batch)
    with pytest.raises(ValueError, match="shards must be"):
        ppo.combine(vec[None, :-1], theta, 3, 40)
    with pytest.raises(ValueError, match="shards must be"):
        ppo.combine(np.stack([vec] * 65), theta, 3, 40)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("activation", ["relu", "tanh"])
def test_shards_of_70_97_and_32_rows_stand_as_close_to_float64_as_the_whole_batch(activation):
    cells, actor, critic = SMALL
    A, n = 2, sum(COUNTS)
    theta, batch = _problem(5, n, cells, actor, critic, A, activation)
    g64, r = autograd(theta, cells, A, actor, critic, activation, batch, torch.float64)
    assert min(np.abs(r - (1 + CLIP)).min(), np.abs(r - (1 - CLIP)).min()) > 1e-4      # (no row may flip between the evaluations)
    whole = ppo.gradient(theta, cells, A, actor, critic, activation, ent_coef=ENT, max_grad_norm=0.0, rows_per_chain=32, **batch, **HYPER)
    vecs, lo = [], 0
    for c in COUNTS:
        vecs.append(ppo.shard_sums(theta, cells, A, actor, critic, activation, count_total=n, rows_per_chain=32, **_cut(batch, lo, lo + c), **HYPER))
        lo += c
    grad, stats, _ = ppo.combine(np.stack(vecs), theta, A, n, ent_coef=ENT, max_grad_norm=0.0)
    cut = lambda g: split(g, cells, A, actor, critic)
    mine, yard = pooled(cut(grad), g64), pooled(cut(whole["grad"]), g64)
    print("pooled distance from float64: three shards %.3e, the whole batch %.3e, ratio %.2f" % (mine, yard, mine / yard))
    assert mine <= 2 * yard
    assert stats["count"] == n and stats["skipped"] == 0
    for k in ("policy_loss", "value_loss", "approx_kl", "clip_fraction"):
        assert abs(stats[k] - whole["stats"][k]) <= 1e-14 * max(1.0, abs(whole["stats"][k])), k
    # a shard that divided by its own count is far off: the divisor is what this test pins
    own = [ppo.shard_sums(theta, cells, A, actor, critic, activation, count_total=c, rows_per_chain=32, **_cut(batch, sum(COUNTS[:i]), sum(COUNTS[:i + 1])), **HYPER)
           for i, c in enumerate(COUNTS)]
    assert pooled(cut(ppo.combine(np.stack(own), theta, A, n, ent_coef=ENT, max_grad_norm=0.0)[0]), g64) > 0.5


# ---------------------------------------------------------------------------------------------------------------- 3
def crafted_order(theta_size, A, seed=0):
    """three vectors [3, L] for which the order of the sum matters: small random doubles, and at a first, a middle and a last weight, at
    dls[0] and at the policy loss's slot the entries ``1e16, 1.0, -1e16``"""
    L = ppo.shard_size(theta_size, A)
    P = L - 18
    v = 1e-3 * np.random.default_rng(seed).standard_normal((3, L))
    v[:, P + A:P + 8] = 0.0
    v[:, P + 8:] = np.abs(v[:, P + 8:]) * 40
    v[:, P + 11] = 0.0      # (no skipped rows)
    for e in (0, P // 2, P - 1, P, P + 8):
        v[:, e] = (1e16, 1.0, -1e16)
    return v


def test_the_order_of_the_shards_is_the_ascending_one():
    theta, _ = _problem(2, 1, 15, (7,), (7,), 3, "relu")
    A, n = 3, 199
    v = crafted_order(theta.size, A)
    P = v.shape[1] - 18
    got = {perm: ppo.combine(v[list(perm)], theta, A, n, ent_coef=0.25, max_grad_norm=0.0) for perm in itertools.permutations(range(3))}
    grad, stats, _ = got[(0, 1, 2)]
    # ascending: ((0.0 + 1e16) + 1.0) + -1e16 = 0.0, the 1.0 lost; with the two large ones first the 1.0 survives
    assert grad[0] == 0.0 and grad[P // 2] == 0.0 and grad[P - 1] == 0.0 and grad[P] == np.float32(0.0 - 0.25) and stats["policy_loss"] == 0.0
    other = got[(0, 2, 1)]
    assert other[0][0] == 1.0 and other[0][P] == np.float32(1.0 - 0.25) and other[1]["policy_loss"] == 1.0 / n
    assert not np.array_equal(_bits(grad), _bits(other[0]))
    want = np.zeros(v.shape[1])
    for w in range(3):
        want = want + v[w]
    _same(grad[:P], want[:P].astype(np.float32), "the ascending sum, narrowed once")
    assert len({_bits(g[0]).tobytes() for g in got.values()}) > 1


# ---------------------------------------------------------------------------------------------------------------- 4
KL_LIMIT = 0.03


def _largest_not_crossing(count, limit):
    """the largest double x whose own mean ``x / count`` is not > limit"""
    x = np.float64(limit) * np.float64(count)
    while x / np.float64(count) > limit:
        x = np.nextafter(x, -np.inf)
    while np.nextafter(x, np.inf) / np.float64(count) <= limit:
        x = np.nextafter(x, np.inf)
    return x


def crafted_gate(theta_size, A):
    """``{name: (vectors [3, L], the total's decision)}``: the kl slots of three shards of COUNTS rows such that no shard alone crosses
    KL_LIMIT and the total does (``total``), one shard crosses and the total does not (``shard``), and a NaN (``nan``).  The limit of
    ``total`` is searched upwards from KL_LIMIT in steps of 1e-4 (the case lives in the roundings): returned as the dict's ``limit``"""
    L = ppo.shard_size(theta_size, A)
    kl, n = L - 18 + 9, np.float64(sum(COUNTS))
    base = np.zeros((3, L))
    base[:, :L - 18] = 1e-3 * np.random.default_rng(4).standard_normal((3, L - 18))
    for k in range(200):
        limit = KL_LIMIT + 1e-4 * k
        x = [_largest_not_crossing(c, limit) for c in COUNTS]
        if ((0.0 + x[0]) + x[1] + x[2]) / n > limit:
            break
    else:
        raise AssertionError("no limit found")
    total, shard, nan = base.copy(), base.copy(), base.copy()
    total[:, kl] = x
    shard[:, kl] = (0.05 * COUNTS[0], 0.0, 0.0)
    nan[:, kl] = (0.05 * COUNTS[0], np.nan, 0.0)
    return {"limit": limit, "total": (total, True), "shard": (shard, False), "nan": (nan, False)}


def test_the_gate_follows_the_total():
    theta, _ = _problem(2, 1, 15, (7,), (7,), 3, "relu")
    A, n = 3, sum(COUNTS)
    C = crafted_gate(theta.size, A)
    kl = ppo.shard_size(theta.size, A) - 18 + 9
    for name in ("total", "shard", "nan"):
        v, stop = C[name]
        limit = C["limit"]
        own = [bool(v[w, kl] / np.float64(c) > limit) for w, c in enumerate(COUNTS)]
        assert any(own) != stop or name == "nan", (name, own)      # the shards' own decisions say the opposite
        _, stats, more = ppo.combine(v, theta, A, n, kl_limit=limit)
        assert (more["stopped"], more["applied"]) == (float(stop), float(not stop)), name
        assert bool(stats["approx_kl"] > limit) == stop
        # sticky: once stopped, stopped
        assert ppo.combine(v, theta, A, n, stopped=True, kl_limit=limit)[2]["applied"] == 0.0
        # and no gate: applied, not stopped
        assert ppo.combine(v, theta, A, n)[2]["applied"] == 1.0 and ppo.combine(v, theta, A, n)[2]["stopped"] == 0.0
    assert np.isnan(ppo.combine(C["nan"][0], theta, A, n, kl_limit=C["limit"])[1]["approx_kl"])


# ---------------------------------------------------------------------------------------------------------------- 5
_NET = (15, (33, 17), (7,), 3)
_HALVES = ((0, 38), (38, 70))


def _half(rank):
    cells, actor, critic, A = _NET
    theta, batch = _problem(11, 70, cells, actor, critic, A, "relu")
    lo, hi = _HALVES[rank]
    return theta, ppo.shard_sums(theta, cells, A, actor, critic, "relu", count_total=70, rows_per_chain=32, **_cut(batch, lo, hi), **HYPER)


def _finish(theta, vectors):
    A = _NET[3]
    grad, _, _ = ppo.combine(vectors, theta, A, 70, ent_coef=ENT, max_grad_norm=0.5)
    return ppo.adam(theta, np.zeros_like(theta), np.zeros_like(theta), 0, grad, A, lr=1e-2)[:3]


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nuclear_sim_amd.sharding import gather_cells, gather_shard_sums, ppo_exchange
    theta, vec = _half(rank)
    every = gather_shard_sums(torch.from_numpy(vec))
    again = ppo_exchange(None)(torch.from_numpy(vec))
    cells = gather_cells(_HALVES[rank][1] - _HALVES[rank][0])
    q.put((rank, every.numpy(), torch.equal(every, again), cells) + tuple(_finish(theta, every.numpy())))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_over_gloo_end_with_the_same_bits():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=240) for _ in range(2)), key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    vectors = np.stack([_half(0)[1], _half(1)[1]])
    want = _finish(_half(0)[0], vectors)
    for rank, every, twice, cells, theta, m, v in got:
        assert every.dtype == np.float64 and twice and cells == [38, 32]
        _same(every, vectors, "the gathered vectors, in rank order")
        _same(theta, want[0], "theta"); _same(m, want[1], "m"); _same(v, want[2], "v")
    assert want[1].any() and not np.array_equal(want[0], _half(0)[0])
