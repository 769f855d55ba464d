"""What the policy on the device (npb_set_policy: an MLP actor-critic, the Gaussian draw, log-probability and value in one launch in front
of every step) costs on BASELINE config 4 at 65 536 and 32 768 plants.

action_test("oil_top_off", range(n), dt = 5) with autoreset (max_episode_steps 64) and episode streams, which drive the heat-source noise
and the power profile on the device: no per-step host input, so collect() applies.  Features of 16 columns x 4 frames, float32; controls of
4 axes (rod RATE, valve RATE, flow RATE, a VALUE axis), float32 input; the rollout with T = 128 and E = 2 extras (value, logp); actor and
critic with hidden (64, 64).  A block is one horizon: T steps, then the rewind.  One handle per size throughout; the policy is set and
dropped on it between blocks, in an order that rotates from round to round.  Setups, event-timed us per step:
  off            features, controls, autoreset and rollout on, no policy: a fixed [n, 4] controls tensor whose sign is flipped in place
                 before every step (what stands in for a policy in the neighbouring tools)
  relu_det, relu_sample, tanh_det, tanh_sample
                 the policy on, deterministic or sampling, writing the controls' input and the two extras slots
  torch          no policy; the same forward passes, the draw (torch.randn) and the log-probability by hand in eager torch, tanh, writing
                 the same tensors (controls_input(), rollout_extras_input())
and, wall time per step with a synchronise at both ends, policy on (tanh_sample):
  collect        one collect(T) call against T step() calls
Reported per setup: the per-step time of each block (median, quartiles, min..max over the blocks), each setup minus off of the same round,
and whether the device path is below the by-hand one -- as measured, whichever way it falls.

--parent DIR: a checkout of the parent commit, built.  `off` is then also measured in fresh processes, alternately on this build and on
the parent's (this script run with --package-root and --only-off), `--process-repeats` times each, and held against each other by
overhead_harness.compare_off.  --resources FILE: the lines of a -Rpass-analysis=kernel-resource-usage build of npb_policy.hip, whose
register and LDS figures are recorded beside the times.  One JSON line per run, all sizes in one object, also written to --out
(profiles/policy_overhead.json).

Built on tools/overhead_harness.py like the *_overhead.py scripts; it is not named as they are because tests/test_overhead_harness_cpu.py
pins their list.
"""
import argparse
import os
import re
import sys
import time

import numpy as np

from overhead_harness import add_parent_arguments, compare_off, head, off_across_builds, paired, rotated_blocks, stats, time_steps, write_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 8
DT = 5.0
T, E, K, C, L = 128, 2, 4, 16, 64
AXES = [("rod", "rate"), ("valve", "rate"), ("flow", "rate"), (None, "value")]
HIDDEN = (64, 64)
POLICIES = {"relu_det": ("relu", True), "relu_sample": ("relu", False), "tanh_det": ("tanh", True), "tanh_sample": ("tanh", False)}


def columns():
    from nuclear_sim_amd.env import INFO_COLUMNS
    return ([("obs", i) for i in range(8)] + [("info", name) for name in INFO_COLUMNS[:4]] +
            ["reward", ("pump.oil_level", 0), ("pump.oil_level", 1), "prim.fuel_temperature"])[:C]


def nets(torch, dev, activation):
    """actor, critic (torch modules on the device, seeded) and log_std"""
    torch.manual_seed(0)
    act = torch.nn.Tanh if activation == "tanh" else torch.nn.ReLU

    def mlp(out):
        dims, layers = [K * C] + list(HIDDEN), []
        for i, o in zip(dims[:-1], dims[1:]):
            layers += [torch.nn.Linear(i, o), act()]
        return torch.nn.Sequential(*layers, torch.nn.Linear(dims[-1], out)).to(dev)
    actor, critic = mlp(len(AXES)), mlp(1)
    with torch.no_grad():
        for m in list(actor.modules()) + list(critic.modules()):
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(0.1)      # (small actions: the run stays the neighbouring tools' run)
    return actor, critic, torch.full((len(AXES),), -4.0, device=dev)


def by_hand(torch, env, actor, critic, log_std):
    """one step's policy in eager torch, writing the tensors the device's launch writes"""
    half_log_2pi = 0.9189385332046727
    x_in, extras = env.controls_input(), env.rollout_extras_input()
    std = torch.exp(log_std)

    def step():
        with torch.no_grad():
            x = env.features().reshape(env.n, -1)
            mean, value = actor(x), critic(x).squeeze(1)
            z = torch.randn_like(mean)
            x_in.copy_(mean + std * z)
            extras[:, 0].copy_(value)
            extras[:, 1].copy_(-(len(AXES) * half_log_2pi) - (0.5 * z * z + log_std).sum(dim=1))
        return env.step()
    return step


def resources(path):
    """{kernel: {VGPRs, SGPRs, scratch, LDS, occupancy}} from the remarks of -Rpass-analysis=kernel-resource-usage"""
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "LDS Size [bytes/block]": "lds_bytes_per_block",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd"}
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and name and m.group(1) in keys:
            out[name][keys[m.group(1)]] = int(m.group(2))
    return out


def measure(n, rounds, only_off):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, noise_generator="device", autoreset=True, max_episode_steps=L, episode_streams=True,
                                      power_profile_steps=L)
    env.set_features(columns(), stack=K, final=True)
    env.set_controls(AXES)
    env.set_rollout(T, extras=E)
    has = hasattr(env, "set_policy") and not only_off
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    env.controls_input().copy_(((torch.rand((n, len(AXES)), generator=g) * 2.0 - 1.0) * 0.02).to(torch.float32))
    x = env.controls_input()
    env.features()
    setups = ["off"] + (list(POLICIES) + ["torch"] if has else [])
    made = {a: nets(torch, dev, a) for a in ("relu", "tanh")} if has else {}
    hand = by_hand(torch, env, *made["tanh"]) if has else None
    state = {"policy": None}

    def switch(setup):
        want = setup if setup in POLICIES else None
        if state["policy"] == want:
            return
        if state["policy"] is not None:
            env.set_policy(None)
        if want is not None:
            activation, deterministic = POLICIES[want]
            env.set_policy(*made[activation], activation=activation, deterministic=deterministic, seed=1, extras=("value", "logp"))
        state["policy"] = want

    def step(setup):
        if setup == "torch":
            return hand()
        if setup == "off":
            x.neg_()
        return env.step()

    def run_block(setup):
        if has:
            switch(setup)
        env.rollout_begin()
        for _ in range(W):
            step(setup)
        env.rollout_begin()
        us = time_steps(stream, lambda: step(setup), T)
        env.rollout_begin()
        return us

    blocks = rotated_blocks(setups, rounds, run_block)
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": T, "rounds": rounds,
           "features": [K, C], "axes": len(AXES), "extras": E, "hidden": list(HIDDEN), "max_episode_steps": L,
           "setups": {s: stats(v) for s, v in blocks.items()}}
    if has:
        for s in list(POLICIES) + ["torch"]:
            out[s + "_cost_us_per_step"] = paired(blocks, s, "off")
        out["tanh_sample_is_below_by_hand"] = bool(out["tanh_sample_cost_us_per_step"]["median"] < out["torch_cost_us_per_step"]["median"])
        # collect(T) against T step() calls: wall time, the policy sampling with tanh
        switch("tanh_sample")
        wall = {"collect": [], "steps": []}
        for r in range(2 + rounds):
            for which in (("collect", "steps") if r % 2 == 0 else ("steps", "collect")):
                env.rollout_begin()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                if which == "collect":
                    env.collect(T)
                else:
                    for _ in range(T):
                        env.step()
                torch.cuda.synchronize(dev)
                if r >= 2:
                    wall[which].append((time.perf_counter() - t0) * 1e6 / T)
        out["collect_wall_us_per_step"] = {k: stats(v) for k, v in wall.items()}
        out["collect_is_below_the_steps"] = bool(np.median(wall["collect"]) < np.median(wall["steps"]))
        switch("off")
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--resources", default=None, help="the output of a -Rpass-analysis=kernel-resource-usage build of npb_policy.hip")
    add_parent_arguments(ap, "policy_overhead.json")
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    sizes = {}
    for n in a.n:
        res = measure(n, a.rounds, a.only_off)
        print("%d plants: measured" % n, file=sys.stderr, flush=True)
        if a.parent and not a.only_off:
            this, parent = off_across_builds(__file__, ["--n", n, "--rounds", a.rounds], a.parent, a.process_repeats,
                                             lambda run: run["sizes"][str(n)]["setups"]["off"]["median_us"], 900)
            res["parent_comparison"] = {"off": compare_off(this, parent, res["setups"]["off"])}
        sizes[str(n)] = res
    out = {"what": "per-step time of config 4 with autoreset (max_episode_steps 64), episode streams, features of 16 columns x 4 frames float32, "
                   "controls of 4 axes and the rollout (T = 128, E = 2): the policy (hidden (64, 64) actor and critic) off and on, deterministic "
                   "and sampling, relu and tanh; the same policy by hand in eager torch beside it; collect(T) against T step() calls, wall time",
           "kernel": "v_mfma_f32_32x32x2_f32 (npb_policy.hip)", "sizes": sizes, "head": head(ROOT)}
    if a.resources:
        out["kernel_resources"] = resources(a.resources)
    write_line(out, a.out)


if __name__ == "__main__":
    main()
