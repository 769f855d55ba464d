"""What one update of the policy on the device (npb_policy_update: the PPO loss of a minibatch, its gradient through both nets, the
clipping and one Adam step) costs, against the same update by hand in eager torch.

The nets are tools/policy_cost.py's: 64 cells (16 columns x 4 frames), 4 axes, actor and critic with hidden (64, 64), relu and tanh.  The
minibatch is 65 536 rows of explicit tensors on the device: obs standard normal, the actions the policy's own means plus std * z with a
scatter of 0.15 std on top, logp_old the density of the unscattered draw (so the ratios scatter around 1 and both branches of the clip
are taken), adv and ret standard normal, all float32.  Setups, event-timed us per update, a block being `--updates` updates in a row:
  device_relu, device_tanh    one npb_policy_update per minibatch through a descriptor built once (clip 0.2, vf_coef 0.5, ent_coef 0.01,
                              max_grad_norm 0.5, chains of 256 rows, lr 3e-4)
  torch_relu, torch_tanh      the same update by hand on the same tensors: torch.nn modules, autograd of the same loss,
                              clip_grad_norm_, torch.optim.Adam(eps=1e-5)
One handle; the order of the setups rotates from round to round.  The claim under test: the device's update is below the by-hand one by
more than the by-hand blocks' own spread (max - min) -- reported as measured, whichever way it falls.
And the step with the feature unused: `off` is the step with the policy set and no training, event-timed; with --parent DIR (a built
checkout of the parent commit) it is measured in fresh processes alternately on this build and on the parent's and held against each
other by overhead_harness.compare_off.  --resources FILE: the remarks of a -Rpass-analysis=kernel-resource-usage build of npb_ppo.hip.
One JSON line, also written to --out (profiles/ppo_cost.json).

--options: what the training step's options cost instead (profiles/ppo_options_cost.json).  The same minibatch and nets, relu; setups,
event-timed us per update in blocks of `--updates`, the order rotating:
  off            npb_policy_update, as above
  clip_vf        npb_policy_update_more with clip_vf 0.2 around old values that stand 0.3 * N(0, 1) from the returns
  gate_open      npb_policy_update_more with a kl_limit no approx_kl reaches, between npb_policy_train_begin and npb_policy_train_end
                 (both outside the timed region: the pair's one read-back is per iteration, and reported as train_end_us)
  gate_stopped   the same with a kl_limit the first update exceeds: every update forms its gradient and statistics and applies nothing
With --parent DIR the `off` update is also timed in fresh processes alternately on this build and on the parent's (--only-off: that
setup alone, which the parent's library has too) and held against each other by overhead_harness.compare_off: the always-on row sums of
explained_variance are what could make `off` dearer.

--shards: what the update cut across shards costs (profiles/ppo_shards_cost.json).  The same minibatch and nets, relu; setups, event-timed
us per call in blocks of `--updates`, the order rotating:
  off            npb_policy_update, as above
  shards_w1      npb_policy_shard_sums then npb_policy_apply_shards over that one vector: the same update in two calls
  sums_alone     npb_policy_shard_sums
  apply_w2 / 8 / 64   npb_policy_apply_shards alone over W synthetic vectors (the handle's own sums in every row)
exchange_bytes_per_shard = 8 * L is stated, not measured, and no all-gather across devices is timed.  With --parent DIR the `off` update
is held against the parent's in fresh processes as under --options: the finish kernel's second instance must leave the plain one alone.

Built on tools/overhead_harness.py like the *_overhead.py scripts; it is not named as they are because tests/test_overhead_harness_cpu.py
pins their list.
"""
import argparse
import ctypes
import os
import sys

from overhead_harness import add_parent_arguments, compare_off, head, off_across_builds, paired, rotated_blocks, stats, time_steps, write_line
from policy_cost import AXES, DT, HIDDEN, C, E, K, L, T, columns, nets, resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5)
LR, BETAS, EPS = 3e-4, (0.9, 0.999), 1e-5
HALF_LOG_2PI = 0.9189385332046727


def by_hand(torch, actor, critic, log_std, batch):
    """one update in eager torch: modules, autograd, clip_grad_norm_, Adam"""
    log_std = torch.nn.Parameter(log_std.clone())
    params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS)
    obs, act, old, adv, ret = (batch[k] for k in ("obs", "act", "logp_old", "adv", "ret"))
    clip, A = HYPER["clip"], act.shape[1]

    def update():
        mean, v = actor(obs), critic(obs).squeeze(1)
        d = (act - mean) / torch.exp(log_std)
        lp = -(A * HALF_LOG_2PI) - (0.5 * d * d + log_std).sum(dim=1)
        r = torch.exp(lp - old)
        loss = (-torch.minimum(r * adv, torch.clamp(r, 1 - clip, 1 + clip) * adv)).mean() + HYPER["vf_coef"] * (0.5 * (v - ret) ** 2).mean() \
            - HYPER["ent_coef"] * (log_std + 0.5 + HALF_LOG_2PI).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, HYPER["max_grad_norm"])
        opt.step()
    return update


def measure(n, rows, updates, rounds, only_off):
    import torch
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, noise_generator="device", autoreset=True, max_episode_steps=L, episode_streams=True,
                                      power_profile_steps=L)
    env.set_features(columns(), stack=K, final=True)
    env.set_controls(AXES)
    env.set_rollout(T, extras=E)
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    env.features()
    made = {a: nets(torch, dev, a) for a in ("relu", "tanh")}
    env.set_policy(*made["tanh"], activation="tanh", seed=1, extras=("value", "logp"))

    def off_block():
        env.rollout_begin()
        for _ in range(8):
            env.step()
        env.rollout_begin()
        us = time_steps(stream, env.step, T)
        env.rollout_begin()
        return us
    off = [off_block() for _ in range(1 + rounds)][1:]
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "rounds": rounds, "features": [K, C],
           "axes": len(AXES), "hidden": list(HIDDEN), "off_block_steps": T, "off": stats(off)}
    if only_off or not hasattr(env, "policy_grad"):
        env.close()
        return out
    # the minibatch
    g = torch.Generator(device="cpu").manual_seed(0)
    A = len(AXES)
    obs = torch.randn((rows, K * C), generator=g).to(dev)
    z = torch.randn((rows, A), generator=g).to(dev)
    scatter = 0.15 * torch.randn((rows, A), generator=g).to(dev)
    batches = {}
    for a, (actor, critic, log_std) in made.items():
        with torch.no_grad():
            std = torch.exp(log_std)
            act = (actor(obs) + std * (z + scatter)).contiguous()
            old = (-(A * HALF_LOG_2PI) - (0.5 * z * z + log_std).sum(dim=1)).contiguous()
        batches[a] = {"obs": obs, "act": act, "logp_old": old, "adv": torch.randn(rows, generator=g).to(dev), "ret": torch.randn(rows, generator=g).to(dev)}
    hand = {a: by_hand(torch, *nets(torch, dev, a), batches[a]) for a in made}
    descs = {a: env._ppo_desc(batches[a], rows_per_chain=256, **HYPER) for a in made}
    state = {"activation": "tanh"}
    stats_out = {}

    def run_block(setup):
        kind, a = setup.split("_")
        if kind == "torch":
            step = hand[a]
        else:
            if state["activation"] != a:      # (set again: theta and the optimiser start over; the shapes and so the work are the same)
                env.set_policy(None)
                env.set_policy(*made[a], activation=a, seed=1, extras=("value", "logp"))
                state["activation"] = a
            d = descs[a][0]

            def step():
                _lib.check(env.L.npb_policy_update(env._h, ctypes.byref(d), LR, BETAS[0], BETAS[1], EPS, env._stream()), env._h)
        for _ in range(3):
            step()
        us = time_steps(stream, step, updates)
        if kind == "device":
            stats_out[a] = env.policy_grad(batches[a], rows_per_chain=256, **HYPER)["stats"].cpu().tolist()
        return us
    setups = ["device_relu", "torch_relu", "device_tanh", "torch_tanh"]
    blocks = rotated_blocks(setups, rounds, run_block)
    out.update({"rows": rows, "updates_per_block": updates, "rows_per_chain": 256, "hyper": HYPER, "lr": LR, "setups": {s: stats(v) for s, v in blocks.items()},
                "last_stats": stats_out})
    for a in ("relu", "tanh"):
        diff = paired(blocks, "torch_" + a, "device_" + a)
        spread = out["setups"]["torch_" + a]["max_us"] - out["setups"]["torch_" + a]["min_us"]
        out[a] = {"by_hand_minus_device_us": diff, "by_hand_spread_us": spread, "device_is_below_by_hand_by_more_than_its_spread": bool(diff["median"] > spread)}
    env.close()
    return out


def measure_options(n, rows, updates, rounds, only_off):
    import time

    import torch
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT)
    env.set_features(columns(), stack=K, final=True)
    env.set_controls(AXES)
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    env.features()
    actor, critic, log_std = nets(torch, dev, "relu")
    env.set_policy(actor, critic, log_std, activation="relu", seed=1)
    g = torch.Generator(device="cpu").manual_seed(0)
    A = len(AXES)
    obs = torch.randn((rows, K * C), generator=g).to(dev)
    z = torch.randn((rows, A), generator=g).to(dev)
    scatter = 0.15 * torch.randn((rows, A), generator=g).to(dev)
    with torch.no_grad():
        act = (actor(obs) + torch.exp(log_std) * (z + scatter)).contiguous()
        old = (-(A * HALF_LOG_2PI) - (0.5 * z * z + log_std).sum(dim=1)).contiguous()
    batch = {"obs": obs, "act": act, "logp_old": old, "adv": torch.randn(rows, generator=g).to(dev), "ret": torch.randn(rows, generator=g).to(dev)}
    value_old = (batch["ret"] + 0.3 * torch.randn(rows, generator=g).to(dev)).contiguous()
    d, held = env._ppo_desc(batch, rows_per_chain=256, **HYPER)
    L, h = env.L, env._h

    def plain():
        _lib.check(L.npb_policy_update(h, ctypes.byref(d), LR, BETAS[0], BETAS[1], EPS, env._stream()), h)
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "rounds": rounds, "features": [K, C], "axes": A, "hidden": list(HIDDEN), "rows": rows,
           "updates_per_block": updates, "rows_per_chain": 256, "hyper": HYPER, "lr": LR, "activation": "relu"}
    if only_off or not hasattr(L, "npb_policy_update_more"):
        for _ in range(3):
            plain()
        out["update_off"] = stats([time_steps(stream, plain, updates) for _ in range(1 + rounds)][1:])
        env.close()
        return out
    more = {}
    for name, clip_vf, kl_limit in (("clip_vf", 0.2, 0.0), ("gate_open", 0.0, 1e300), ("gate_stopped", 0.0, 1e-300)):
        m = _lib.NpbPpoMore()
        m.value_old, m.clip_vf, m.kl_limit = value_old.data_ptr(), clip_vf, kl_limit
        more[name] = m
    ends, last = [], {}

    def run_block(setup):
        if setup == "off":
            step = plain
        else:
            m = more[setup]

            def step():
                _lib.check(L.npb_policy_update_more(h, ctypes.byref(d), ctypes.byref(m), LR, BETAS[0], BETAS[1], EPS, env._stream()), h)
        gated = setup.startswith("gate")
        if gated:
            _lib.check(L.npb_policy_train_begin(h, env._stream()), h)
        for _ in range(3):
            step()
        us = time_steps(stream, step, updates)
        if gated:
            applied = ctypes.c_uint32()
            t0 = time.perf_counter()
            _lib.check(L.npb_policy_train_end(h, ctypes.byref(applied), env._stream()), h)
            ends.append(1e6 * (time.perf_counter() - t0))
            last[setup + "_applied"] = applied.value
        row = torch.zeros(_lib.PPO_STATS_MORE, dtype=torch.float64, device=dev)
        _lib.check(L.npb_policy_get_stats_more(h, ctypes.c_void_p(row.data_ptr()), env._stream()), h)
        last[setup] = row.cpu().tolist()
        return us
    setups = ["off", "clip_vf", "gate_open", "gate_stopped"]
    blocks = rotated_blocks(setups, rounds, run_block)
    out.update({"setups": {s: stats(v) for s, v in blocks.items()}, "update_off": stats(blocks["off"]), "last_more": last,
                "train_end_us": stats(ends), "updates_between_begin_and_end": updates + 3})
    for s in setups[1:]:
        out[s + "_minus_off_us"] = paired(blocks, s, "off")
    out["off_spread_us"] = out["setups"]["off"]["max_us"] - out["setups"]["off"]["min_us"]
    del held
    env.close()
    return out


def main_options(a):
    res = measure_options(a.n, a.rows, a.updates, a.rounds, a.only_off)
    if a.parent and not a.only_off:
        argv = ["--options", "--n", a.n, "--rows", a.rows, "--updates", a.updates, "--rounds", a.rounds]
        this, parent = off_across_builds(__file__, argv, a.parent, a.process_repeats, lambda run: run["result"]["update_off"]["median_us"], 900)
        res["parent_comparison"] = {"update_off": compare_off(this, parent, res["update_off"])}
    out = {"what": "one update of the policy on a minibatch of 65 536 rows (64 cells, 4 axes, hidden (64, 64) actor and critic, relu) with the training "
                   "step's options off (npb_policy_update), with clip_vf, and with the target_kl gate armed, not stopping and stopped, event-timed us "
                   "per update; and the options-off update of this build against the parent's in fresh processes",
           "result": res, "head": head(ROOT)}
    if a.resources:
        out["kernel_resources"] = resources(a.resources)
    write_line(out, a.out)


def measure_shards(n, rows, updates, rounds, only_off):
    import torch
    from nuclear_sim_amd import _lib
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT)
    env.set_features(columns(), stack=K, final=True)
    env.set_controls(AXES)
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    env.features()
    actor, critic, log_std = nets(torch, dev, "relu")
    env.set_policy(actor, critic, log_std, activation="relu", seed=1)
    g = torch.Generator(device="cpu").manual_seed(0)
    A = len(AXES)
    obs = torch.randn((rows, K * C), generator=g).to(dev)
    z = torch.randn((rows, A), generator=g).to(dev)
    scatter = 0.15 * torch.randn((rows, A), generator=g).to(dev)
    with torch.no_grad():
        act = (actor(obs) + torch.exp(log_std) * (z + scatter)).contiguous()
        old = (-(A * HALF_LOG_2PI) - (0.5 * z * z + log_std).sum(dim=1)).contiguous()
    batch = {"obs": obs, "act": act, "logp_old": old, "adv": torch.randn(rows, generator=g).to(dev), "ret": torch.randn(rows, generator=g).to(dev)}
    d, held = env._ppo_desc(batch, rows_per_chain=256, **HYPER)
    L, h = env.L, env._h

    def plain():
        _lib.check(L.npb_policy_update(h, ctypes.byref(d), LR, BETAS[0], BETAS[1], EPS, env._stream()), h)
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "rounds": rounds, "features": [K, C], "axes": A, "hidden": list(HIDDEN), "rows": rows,
           "updates_per_block": updates, "rows_per_chain": 256, "hyper": HYPER, "lr": LR, "activation": "relu"}
    if only_off or not hasattr(L, "npb_policy_shard_sums"):
        for _ in range(3):
            plain()
        out["update_off"] = stats([time_steps(stream, plain, updates) for _ in range(1 + rounds)][1:])
        env.close()
        return out
    length = env.policy_shard_size()
    widths = (1, 2, 8, 64)
    own = torch.zeros((1, length), dtype=torch.float64, device=dev)
    own_desc = env._ppo_shards(own, rows, HYPER["ent_coef"], HYPER["max_grad_norm"])
    # synthetic vectors: the handle's own sums of this minibatch, divided for W * rows rows, in every row
    synthetic, descs = {}, {}
    for W in widths[1:]:
        row = env.policy_shard_sums(batch, W * rows, HYPER["clip"], HYPER["vf_coef"], 256)
        synthetic[W] = row[None].repeat(W, 1).contiguous()
        descs[W] = env._ppo_shards(synthetic[W], W * rows, HYPER["ent_coef"], HYPER["max_grad_norm"])

    def sums():
        _lib.check(L.npb_policy_shard_sums(h, ctypes.byref(d), None, rows, ctypes.c_void_p(own.data_ptr()), env._stream()), h)

    def apply(s):
        _lib.check(L.npb_policy_apply_shards(h, ctypes.byref(s), LR, BETAS[0], BETAS[1], EPS, env._stream()), h)

    def two_calls():
        sums()
        apply(own_desc)
    steps = {"off": plain, "shards_w1": two_calls, "sums_alone": sums}
    for W in widths[1:]:
        steps["apply_w%d" % W] = lambda s=descs[W]: apply(s)

    def run_block(setup):
        for _ in range(3):
            steps[setup]()
        return time_steps(stream, steps[setup], updates)
    blocks = rotated_blocks(list(steps), rounds, run_block)
    out.update({"setups": {s: stats(v) for s, v in blocks.items()}, "update_off": stats(blocks["off"]), "shard_doubles": length, "exchange_bytes_per_shard": 8 * length,
                "shards_w1_minus_off_us": paired(blocks, "shards_w1", "off"), "off_spread_us": max(blocks["off"]) - min(blocks["off"])})
    del held
    env.close()
    return out


def main_shards(a):
    res = measure_shards(a.n, a.rows, a.updates, a.rounds, a.only_off)
    if a.parent and not a.only_off:
        argv = ["--shards", "--n", a.n, "--rows", a.rows, "--updates", a.updates, "--rounds", a.rounds]
        this, parent = off_across_builds(__file__, argv, a.parent, a.process_repeats, lambda run: run["result"]["update_off"]["median_us"], 900)
        res["parent_comparison"] = {"update_off": compare_off(this, parent, res["update_off"])}
    out = {"what": "one policy across shards, on a minibatch of 65 536 rows (64 cells, 4 axes, hidden (64, 64) actor and critic, relu), event-timed us per "
                   "call: the plain npb_policy_update (off); npb_policy_shard_sums + npb_policy_apply_shards at W = 1 (shards_w1); the sums alone; "
                   "npb_policy_apply_shards alone at W = 2, 8 and 64 over synthetic vectors; and the plain update of this build against the parent's in "
                   "fresh processes.  exchange_bytes_per_shard = 8 * L is stated, not measured; no all-gather across devices is timed",
           "result": res, "head": head(ROOT)}
    if a.resources:
        out["kernel_resources"] = resources(a.resources)
    write_line(out, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--options", action="store_true", help="the cost of value-loss clipping and of the target_kl gate (profiles/ppo_options_cost.json)")
    ap.add_argument("--shards", action="store_true", help="the cost of the update cut across shards (profiles/ppo_shards_cost.json)")
    ap.add_argument("--n", type=int, default=65536, help="plants of the env whose step is `off`")
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--resources", default=None, help="the output of a -Rpass-analysis=kernel-resource-usage build of npb_ppo.hip")
    add_parent_arguments(ap, "ppo_cost.json")
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    if a.shards:
        if a.out == os.path.join(ROOT, "profiles", "ppo_cost.json"):
            a.out = os.path.join(ROOT, "profiles", "ppo_shards_cost.json")
        return main_shards(a)
    if a.options:
        if a.out == os.path.join(ROOT, "profiles", "ppo_cost.json"):
            a.out = os.path.join(ROOT, "profiles", "ppo_options_cost.json")
        return main_options(a)
    res = measure(a.n, a.rows, a.updates, a.rounds, a.only_off)
    if a.parent and not a.only_off:
        this, parent = off_across_builds(__file__, ["--n", a.n, "--rounds", a.rounds], a.parent, a.process_repeats, lambda run: run["result"]["off"]["median_us"], 900)
        res["parent_comparison"] = {"off": compare_off(this, parent, res["off"])}
    out = {"what": "one npb_policy_update per minibatch of 65 536 rows (64 cells, 4 axes, hidden (64, 64) actor and critic) against the same update by "
                   "hand in eager torch, relu and tanh, event-timed us per update; and the step with the policy set and no training (`off`), this "
                   "build against the parent's",
           "kernel": "v_mfma_f32_32x32x2_f32 (npb_ppo.hip)", "result": res, "head": head(ROOT)}
    if a.resources:
        out["kernel_resources"] = resources(a.resources)
    write_line(out, a.out)


if __name__ == "__main__":
    main()
