"""What one update of a recurrent policy costs when it is trained through time on the device (npb_policy_update_seq: PPO over whole
sequences, the gradient through both nets, the GRU cell and time, and the Adam step), at the README's shape: features of 16 columns x 4
frames float32 (64 cells), a cell 64 wide with soft gates, actor and critic with hidden (64, 64), tanh, 4 axes, sequences of t = 128 slots,
at 4 096 and 8 192 plants in one minibatch (chains of 32 plants: plants / 32 workgroups, each serial in t).

The minibatches are explicit tensors (random features, actions, advantages and returns; no restarts), so the env behind the handle is
small.  Setups, event-timed us per update:
  rowwise        a policy WITHOUT a core and row-wise policy_grad of 65 536 rows in chains of 256: the feature off, what the parent commit's
                 build runs too.  Its kernel shares the per-row epilogue and the dW / back routines with the sequence kernel (npb_ppo.h)
  seq_<plants>   policy_grad_sequences and policy_adam of t x plants cells
  torch_<plants> the same update by hand in eager torch: torch.nn.GRUCell stepped t times, the nets, the loss, autograd back through time,
                 clip_grad_norm_ and Adam
Reported: each setup's blocks and seq against torch as measured, whichever way it falls.  The sequence kernel is serial in t and parallel
over plants / 32 workgroups, so it fills few of the device's compute units below about 8 192 plants: expect that in the figures.

--parent DIR: a checkout of the parent commit, built.  `rowwise` is then also measured in fresh processes, alternately on this build and on
the parent's (this script with --package-root and --only-off), `--process-repeats` times each, and held against each other by
overhead_harness.compare_off; off_within_the_parents_own_spread judges by the parent's two runs alone.  --resources FILE: the remarks of a
-Rpass-analysis=kernel-resource-usage build of npb_ppo_seq.hip.  One JSON line, also written to --out
(profiles/recurrent_train_cost.json).

--segments: TRUNCATED SEGMENTS (npb_policy_update_segments, npb_policy_segment_starts, npb_policy_core_segments) beside whole sequences, in
the same run, into profiles/segment_train_cost.json.  Setups, event-timed us:
  seq_<plants>              the whole-sequence update above
  seg_<plants>_<every>      policy_grad_sequences on a segment minibatch of ALL (t / every) * plants segments and policy_adam: the cells of the
                            whole-sequence update, in (t / every) times as many workgroups, each (t / every) times less deep
and on a handle of <plants> plants with config 4's autoreset, the features, the controls and a rollout of T = 128 slots:
  step_core / step_core_rec a step with the recurrent policy, without and with policy_segments(16): the difference of the same round's
                            blocks is what recording the stored states costs a step
  refresh_<every>           policy_refresh_segments() alone, over the 128 recorded slots
With --parent the whole-sequence update and step_core (no policy_segments: what the parent runs too) are measured in fresh processes,
alternately on this build and on the parent's, and judged by overhead_harness.compare_off.

Built on tools/overhead_harness.py like the *_overhead.py scripts; it is not named as they are because tests/test_overhead_harness_cpu.py
pins their list.
"""
import argparse
import os
import sys

from overhead_harness import add_parent_arguments, compare_off, head, off_across_builds, paired, rotated_blocks, stats, time_steps, write_line
from policy_cost import AXES, DT, HIDDEN, C, E, K, L, W, columns, nets, resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, T, ROWS = 64, 128, 65536
HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5)
LR, BETAS, EPS = 3e-4, (0.9, 0.999), 1e-5
HALF_LOG_2PI = 0.9189385332046727


def batch_of(torch, dev, shape, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    A = len(AXES)

    def normal(*more):
        return torch.randn(shape + more, generator=g, device=dev, dtype=torch.float32)
    return {"obs": normal(K * C), "act": 0.5 * normal(A), "logp_old": -(A * HALF_LOG_2PI) - 0.5 * normal().abs(), "adv": normal(), "ret": normal()}


def by_hand(torch, gru, actor, critic, log_std, batch, first):
    """one update over whole sequences in eager torch: the cell stepped t times, autograd back through time, clip_grad_norm_, Adam"""
    log_std = torch.nn.Parameter(log_std.clone())
    params = list(gru.parameters()) + list(actor.parameters()) + list(critic.parameters()) + [log_std]
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS)
    obs, act, old, adv, ret = (batch[k] for k in ("obs", "act", "logp_old", "adv", "ret"))
    clip, A = HYPER["clip"], act.shape[-1]

    def update():
        h, states = first, []
        for s in range(obs.shape[0]):
            h = gru(obs[s], h)
            states.append(h)
        hs = torch.stack(states)
        mean, v = actor(hs), critic(hs).squeeze(-1)
        d = (act - mean) / torch.exp(log_std)
        lp = -(A * HALF_LOG_2PI) - (0.5 * d * d + log_std).sum(dim=-1)
        r = torch.exp(lp - old)
        loss = (-torch.minimum(r * adv, torch.clamp(r, 1 - clip, 1 + clip) * adv)).mean() + HYPER["vf_coef"] * (0.5 * (v - ret) ** 2).mean() \
            - HYPER["ent_coef"] * (log_std + 0.5 + HALF_LOG_2PI).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, HYPER["max_grad_norm"])
        opt.step()
    return update


def measure(plants, updates, rounds, only_off):
    import copy

    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(64), dt=DT)
    env.set_features(columns(), stack=K)
    env.set_controls(AXES)
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    actor, critic, _ = nets(torch, dev, "tanh")      # (K * C == H: the same nets with and without the cell)
    log_std = torch.full((len(AXES),), -0.5, device=dev)      # (a std of the actions' own size: the ratios stay finite and some are clipped)
    torch.manual_seed(1)
    gru = torch.nn.GRUCell(K * C, H).to(dev)
    rows = batch_of(torch, dev, (ROWS,), 1)
    setups = ["rowwise"]
    seqs, hands = {}, {}
    if not only_off:
        for n in plants:
            b = batch_of(torch, dev, (T, n), 2 + n)
            b.update(episode=torch.zeros((T, n), dtype=torch.int32, device=dev), ended=torch.zeros((T, n), dtype=torch.uint8, device=dev),
                     first=torch.zeros((n, H), dtype=torch.float32, device=dev))
            seqs[n] = b
            hands[n] = by_hand(torch, copy.deepcopy(gru), copy.deepcopy(actor), copy.deepcopy(critic), log_std, b, b["first"])
            setups += ["seq_%d" % n, "torch_%d" % n]
    state = {"policy": None}

    def switch(want):
        if state["policy"] == want:
            return
        if state["policy"] is not None:
            env.set_policy(None)
        more = dict(core=gru, gates="soft") if want == "core" else {}
        env.set_policy(actor, critic, log_std, activation="tanh", seed=1, **more)
        state["policy"] = want

    def run_block(setup):
        kind, _, n = setup.partition("_")
        if kind == "rowwise":
            switch("mlp")
            return time_steps(stream, lambda: env.policy_grad(rows, rows_per_chain=256, **HYPER), updates)
        if kind == "torch":
            return time_steps(stream, hands[int(n)], updates)
        switch("core")

        def update():
            env.policy_grad_sequences(seqs[int(n)], plants_per_chain=32, **HYPER)
            env.policy_adam(lr=LR, betas=BETAS, eps=EPS)
        return time_steps(stream, update, updates)

    blocks = rotated_blocks(setups, rounds, run_block)
    out = {"device": torch.cuda.get_device_name(dev), "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "updates_per_block": updates,
           "rounds": rounds, "features": [K, C], "axes": len(AXES), "hidden": list(HIDDEN), "core": H, "gates": "soft", "activation": "tanh", "t": T,
           "rowwise_rows": ROWS, "setups": {s: stats(v) for s, v in blocks.items()}}
    for n in seqs:
        seq, hand = out["setups"]["seq_%d" % n]["median_us"], out["setups"]["torch_%d" % n]["median_us"]
        out["plants_%d" % n] = {"workgroups": -(-n // 32), "cells": T * n, "seq_us_per_update": seq, "torch_us_per_update": hand, "seq_ns_per_cell": 1e3 * seq / (T * n),
                                "seq_is_below_by_hand": bool(seq < hand)}
    env.close()
    return out


def measure_segments(plants, everys, updates, rounds, only_off):
    """--segments: the updates on a small handle with explicit tensors, then per size a handle that steps and refreshes.  only_off: what
    the parent's build runs too -- the whole-sequence updates and the step without stored states"""
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(64), dt=DT)
    env.set_features(columns(), stack=K)
    env.set_controls(AXES)
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    actor, critic, _ = nets(torch, dev, "tanh")
    log_std = torch.full((len(AXES),), -0.5, device=dev)
    torch.manual_seed(1)
    gru = torch.nn.GRUCell(K * C, H).to(dev)
    env.set_policy(actor, critic, log_std, activation="tanh", seed=1, core=gru, gates="soft")
    batches, setups = {}, []
    for n in plants:
        b = batch_of(torch, dev, (T, n), 2 + n)
        words = dict(episode=torch.zeros((T, n), dtype=torch.int32, device=dev), ended=torch.zeros((T, n), dtype=torch.uint8, device=dev))
        batches["seq_%d" % n] = dict(b, first=torch.zeros((n, H), dtype=torch.float32, device=dev), **words)
        setups.append("seq_%d" % n)
        for every in ([] if only_off else everys):
            chunks = T // every
            # segment g = c * n + p of the identity index: [every][chunks * n] is the [T][n] tensor's rows c * every + s, chunk by chunk
            cut = {k: v.reshape((chunks, every, n) + tuple(v.shape[2:])).transpose(0, 1).reshape((every, chunks * n) + tuple(v.shape[2:])).contiguous() for k, v in b.items()}
            batches["seg_%d_%d" % (n, every)] = dict(cut, first=torch.zeros((chunks, n, H), dtype=torch.float32, device=dev), every=every, **words)
            setups.append("seg_%d_%d" % (n, every))

    def run_block(setup):
        def update():
            env.policy_grad_sequences(batches[setup], plants_per_chain=32, **HYPER)
            env.policy_adam(lr=LR, betas=BETAS, eps=EPS)
        return time_steps(stream, update, updates)
    blocks = rotated_blocks(setups, rounds, run_block)
    out = {"device": torch.cuda.get_device_name(dev), "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "updates_per_block": updates,
           "rounds": rounds, "features": [K, C], "axes": len(AXES), "hidden": list(HIDDEN), "core": H, "gates": "soft", "activation": "tanh", "t": T,
           "setups": {s: stats(v) for s, v in blocks.items()}}
    env.close()
    for n in plants:
        whole = out["setups"]["seq_%d" % n]["median_us"]
        row = {"cells": T * n, "seq_workgroups": -(-n // 32), "seq_us_per_update": whole}
        for every in ([] if only_off else everys):
            seg = out["setups"]["seg_%d_%d" % (n, every)]["median_us"]
            row["every_%d" % every] = {"workgroups": -(-(T // every) * n // 32), "seg_us_per_update": seg, "seg_over_seq": seg / whole, "seg_is_below_seq": bool(seg < whole)}
        # the handle that steps: config 4's autoreset, the rollout of T slots, the recurrent policy
        big = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, noise_generator="device", autoreset=True, max_episode_steps=L, episode_streams=True,
                                          power_profile_steps=L)
        big.set_features(columns(), stack=K, final=True)
        big.set_controls(AXES)
        big.set_rollout(T, extras=E)
        stream_n = torch.cuda.current_stream(big.device)
        big.features()
        big.set_policy(actor, critic, log_std, activation="tanh", seed=1, extras=("value", "logp"), core=gru, gates="soft")

        def step_block(setup):
            if not only_off:
                big.policy_segments(16 if setup == "step_core_rec" else None)
            big.rollout_begin()
            for _ in range(W):
                big.step()
            big.rollout_begin()
            us = time_steps(stream_n, big.step, T)
            big.rollout_begin()
            return us
        steps = rotated_blocks(["step_core"] if only_off else ["step_core", "step_core_rec"], rounds, step_block)
        row["steps"] = {s: stats(v) for s, v in steps.items()}
        if not only_off:
            row["recording_added_us_per_step"] = paired(steps, "step_core_rec", "step_core")
            for every in everys:
                big.policy_segments(every)
                big.rollout_begin()
                for _ in range(T):
                    big.step()
                time_steps(stream_n, big.policy_refresh_segments, 2)
                row["refresh_%d_us" % every] = stats([time_steps(stream_n, big.policy_refresh_segments, 5) for _ in range(rounds)])
        big.close()
        out["plants_%d" % n] = row
        print("%d plants: measured" % n, file=sys.stderr, flush=True)
    return out


def main_segments(a):
    out = measure_segments(a.plants, a.every, a.updates, a.rounds, a.only_off)
    if a.parent and not a.only_off:
        argv = ["--segments", "--updates", a.updates, "--rounds", a.rounds, "--plants"] + list(a.plants)
        picked = []
        this, parent = off_across_builds(__file__, argv, a.parent, a.process_repeats, lambda run: picked.append(run) or 0.0, 1500)
        runs = {"this": picked[0::2], "parent": picked[1::2]}
        out["parent_comparison"] = {}
        for n in a.plants:
            for name, pick, mine in (("seq_%d" % n, lambda r: r["setups"]["seq_%d" % n]["median_us"], out["setups"]["seq_%d" % n]),
                                     ("step_core_%d" % n, lambda r: r["plants_%d" % n]["steps"]["step_core"]["median_us"], out["plants_%d" % n]["steps"]["step_core"])):
                out["parent_comparison"][name] = compare_off([pick(r) for r in runs["this"]], [pick(r) for r in runs["parent"]], mine)
    out["what"] = ("us per update of t = 128 slots x plants cells through a GRU cell 64 wide (soft gates) and nets (64, 64), tanh: policy_grad_sequences + "
                   "policy_adam over whole sequences (seq) and over all the truncated segments of `every` slots (seg); us per step of the recurrent policy "
                   "without and with the stored segment states recorded every 16 slots; us per policy_refresh_segments() over the 128 recorded slots; and, "
                   "with --parent, the whole-sequence update and the step without stored states of this build against the parent's in fresh processes")
    out["kernel"] = "v_mfma_f32_32x32x2_f32 (npb_ppo_seq.hip)"
    out["head"] = head(ROOT)
    if a.resources:
        out["kernel_resources"] = resources(a.resources)
    write_line(out, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", action="store_true", help="truncated segments beside whole sequences (profiles/segment_train_cost.json)")
    ap.add_argument("--every", type=int, nargs="+", default=[16, 32, 128])
    ap.add_argument("--plants", type=int, nargs="+", default=None)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--resources", default=None, help="the output of a -Rpass-analysis=kernel-resource-usage build of npb_ppo_seq.hip")
    add_parent_arguments(ap, "recurrent_train_cost.json")
    ap.set_defaults(out=None)      # (each mode has its own file)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "segment_train_cost.json" if a.segments else "recurrent_train_cost.json")
    sys.path.insert(0, a.package_root)
    if a.plants is None:
        a.plants = [2048, 4096, 8192] if a.segments else [4096, 8192]
    if a.segments:
        return main_segments(a)
    out = measure(a.plants, a.updates, a.rounds, a.only_off)
    if a.parent and not a.only_off:
        this, parent = off_across_builds(__file__, ["--updates", a.updates, "--rounds", a.rounds], a.parent, a.process_repeats,
                                         lambda run: run["setups"]["rowwise"]["median_us"], 900)
        out["parent_comparison"] = {"rowwise": compare_off(this, parent, out["setups"]["rowwise"])}
    out["what"] = ("us per update: row-wise policy_grad of 65 536 rows without a core (this build and, in fresh processes, the parent's); "
                   "policy_grad_sequences + policy_adam of t = 128 slots x plants through a GRU cell 64 wide (soft gates) and nets (64, 64), tanh; "
                   "and the same update by hand in eager torch")
    out["kernel"] = "v_mfma_f32_32x32x2_f32 (npb_ppo_seq.hip)"
    out["head"] = head(ROOT)
    if a.resources:
        out["kernel_resources"] = resources(a.resources)
    write_line(out, a.out)


if __name__ == "__main__":
    main()
