"""Multi-GPU host logic: plants are independent, so the path shards as contiguous blocks of
plants per rank with NO collective while stepping.  The only exchange is the end-of-episode
concat of the observation block (all-gather, RCCL over xGMI on GPUs / gloo in CPU tests) and a
sum of a few int64 event counters."""
from __future__ import annotations

from typing import Tuple

import torch
import torch.distributed as dist


def shard_range(n_global: int, rank: int, world: int) -> Tuple[int, int]:
    """[lo, hi) of the contiguous shard of rank `rank`; shards differ by at most one plant and are
    indexed by GLOBAL plant id so per-plant seeds / ICs do not depend on the world size."""
    base, rem = divmod(n_global, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def gather_observations(obs_local: torch.Tensor, n_global: int, group=None) -> torch.Tensor:
    """All-gather the [n_local, 22] observation blocks into [n_global, 22] on every rank."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    sizes = [shard_range(n_global, r, world) for r in range(world)]
    maxn = max(hi - lo for lo, hi in sizes)
    pad = torch.zeros((maxn, obs_local.shape[1]), dtype=obs_local.dtype, device=obs_local.device)
    pad[: obs_local.shape[0]] = obs_local
    out = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(out, pad, group=group)
    return torch.cat([o[: hi - lo] for o, (lo, hi) in zip(out, sizes)], dim=0)


def reduce_counters(counters: torch.Tensor, group=None) -> torch.Tensor:
    """Sum int64 event counters (scram count, pump trips, turbine trips, maintenance events)."""
    c = counters.clone()
    dist.all_reduce(c, op=dist.ReduceOp.SUM, group=group)
    return c


def gather_shard_sums(vec: torch.Tensor, group=None) -> torch.Tensor:
    """One all-gather of a shard's L pinned double sums (``env.policy_shard_sums``) into [W, L] on every rank, in rank order: what
    ``policy_apply_shards`` and ``ppo.combine`` add in ascending order.  A gather and not an all-reduce: the order of a reduce is not ours
    to pin, while the gather plus the pinned combine gives every rank the same bits.  8 * L bytes a shard.  It serves every pinned vector:
    the normaliser's delta (``env.normalizer_sync``, L = 3 S) and the moments' parts (``env.rollout_moments_shards``, L = 2) too."""
    world = dist.get_world_size(group)
    vec = vec.contiguous()
    out = torch.empty((world, vec.numel()), dtype=vec.dtype, device=vec.device)
    dist.all_gather(list(out.unbind(0)), vec.reshape(-1), group=group)
    return out


def ppo_exchange(group=None):
    """the ``exchange`` callable of ``env.policy_train``: ``gather_shard_sums`` over ``group``"""
    return lambda vec: gather_shard_sums(vec, group)


def normalizer_exchange(group=None):
    """the ``exchange`` callable of ``env.normalizer_sync`` and ``env.rollout_moments_shards``: ``gather_shard_sums`` over ``group``"""
    return ppo_exchange(group)


def gather_cells(n_cells: int, group=None) -> list:
    """The one host all-gather of the shards' sizes: every rank's number of recorded cells, in rank order (``shard_cells`` of
    ``env.policy_train``)"""
    out = [None] * dist.get_world_size(group)
    dist.all_gather_object(out, int(n_cells), group=group)
    return [int(c) for c in out]


def event_histogram(events: torch.Tensor, bins: int = 16, group=None) -> torch.Tensor:
    """Histogram of a per-plant event count over the WHOLE job (BASELINE config 4's report: how many plants topped off 0, 1, 2 ...
    times): the local bincount, counts beyond the last bin clamped into it, summed over the ranks when there are several."""
    hist = torch.bincount(events.to(torch.int64).clamp(min=0, max=bins - 1), minlength=bins)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(hist, op=dist.ReduceOp.SUM, group=group)
    return hist
