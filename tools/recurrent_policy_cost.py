"""What a recurrent core in front of the policy on the device (npb_set_policy_core: a GRU cell of width 64 whose hidden state is carried per
plant, in the policy's ONE launch) adds to a step, on tools/policy_cost.py's configuration at 65 536 and 32 768 plants.

action_test("oil_top_off", range(n), dt = 5) with autoreset (max_episode_steps 64) and episode streams; features of 16 columns x 4 frames,
float32 (64 cells); controls of 4 axes; the rollout with T = 128 and E = 2 extras (value, logp); actor and critic with hidden (64, 64),
tanh, sampling.  The cell is 64 wide, so both nets keep their shapes: with and without the core they read 64 cells.  One handle per size;
the policy is set and dropped on it between blocks, in an order that rotates from round to round.  Setups, event-timed us per step:
  mlp            the policy without a core: the feature off, and what the parent commit's build runs too
  core_soft      the same nets behind a GRU cell with sigmoid / tanh gates (two tanhf per hidden cell and one per candidate)
  core_hard      the same with the piecewise-linear gates
  torch          no policy; the same cell (torch.nn.GRUCell), the restart of the hidden state where the episode index moved, the nets, the
                 draw and the log-probability by hand in eager torch, writing the tensors the device's launch writes
Reported: each setup's blocks, core_* minus mlp and torch minus mlp of the same round (the ADDED time per step), and whether the device's
cell is below the by-hand one -- as measured, whichever way it falls.

--parent DIR: a checkout of the parent commit, built.  `mlp` is then also measured in fresh processes, alternately on this build and on
the parent's (this script with --package-root and --only-off), `--process-repeats` times each, and held against each other by
overhead_harness.compare_off; off_within_the_parents_own_spread judges by the parent's two runs alone.  --resources FILE: the remarks of a
-Rpass-analysis=kernel-resource-usage build of npb_policy_core.hip.  One JSON line, also written to --out
(profiles/recurrent_policy_cost.json).

Built on tools/overhead_harness.py like the *_overhead.py scripts; it is not named as they are because tests/test_overhead_harness_cpu.py
pins their list.
"""
import argparse
import os
import sys

from overhead_harness import add_parent_arguments, compare_off, head, off_across_builds, paired, rotated_blocks, stats, time_steps, write_line
from policy_cost import AXES, DT, HIDDEN, C, E, K, L, T, W, columns, nets, resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 64
SETUPS = {"mlp": None, "core_soft": "soft", "core_hard": "hard"}


def cell(torch, dev):
    torch.manual_seed(1)
    return torch.nn.GRUCell(K * C, H).to(dev)


def by_hand(torch, env, gru, actor, critic, log_std):
    """one step's recurrent policy in eager torch, writing the tensors the device's launch writes"""
    half_log_2pi = 0.9189385332046727
    x_in, extras = env.controls_input(), env.rollout_extras_input()
    std = torch.exp(log_std)
    hidden = torch.zeros((env.n, H), device=env.device)
    seen = torch.zeros(env.n, dtype=torch.int32, device=env.device)
    index = env._episode["episode_index"]

    def step():
        with torch.no_grad():
            x = env.features().reshape(env.n, -1)
            h = gru(x, hidden * (index == seen).unsqueeze(1))
            hidden.copy_(h)
            seen.copy_(index)
            mean, value = actor(h), critic(h).squeeze(1)
            z = torch.randn_like(mean)
            x_in.copy_(mean + std * z)
            extras[:, 0].copy_(value)
            extras[:, 1].copy_(-(len(AXES) * half_log_2pi) - (0.5 * z * z + log_std).sum(dim=1))
        return env.step()
    return step


def measure(n, rounds, only_off):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, noise_generator="device", autoreset=True, max_episode_steps=L, episode_streams=True,
                                      power_profile_steps=L)
    env.set_features(columns(), stack=K, final=True)
    env.set_controls(AXES)
    env.set_rollout(T, extras=E)
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    env.features()
    actor, critic, log_std = nets(torch, dev, "tanh")      # (K * C == H: the same nets with and without the cell)
    gru = cell(torch, dev)
    setups = ["mlp"] if only_off else list(SETUPS) + ["torch"]
    hand = None if only_off else by_hand(torch, env, gru, actor, critic, log_std)
    state = {"policy": "none"}

    def switch(setup):
        want = setup if setup in SETUPS else "none"
        if state["policy"] == want:
            return
        if state["policy"] != "none":
            env.set_policy(None)
        if want != "none":
            more = {} if SETUPS[want] is None else dict(core=gru, gates=SETUPS[want])
            env.set_policy(actor, critic, log_std, activation="tanh", seed=1, extras=("value", "logp"), **more)
        state["policy"] = want

    def step(setup):
        return hand() if setup == "torch" else env.step()

    def run_block(setup):
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
           "features": [K, C], "axes": len(AXES), "extras": E, "hidden": list(HIDDEN), "core": H, "max_episode_steps": L,
           "setups": {s: stats(v) for s, v in blocks.items()}}
    if not only_off:
        for s in ("core_soft", "core_hard", "torch"):
            out[s + "_added_us_per_step"] = paired(blocks, s, "mlp")
        out["core_soft_is_below_by_hand"] = bool(out["core_soft_added_us_per_step"]["median"] < out["torch_added_us_per_step"]["median"])
    switch("torch")
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--resources", default=None, help="the output of a -Rpass-analysis=kernel-resource-usage build of npb_policy_core.hip")
    add_parent_arguments(ap, "recurrent_policy_cost.json")
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    sizes = {}
    for n in a.n:
        res = measure(n, a.rounds, a.only_off)
        print("%d plants: measured" % n, file=sys.stderr, flush=True)
        if a.parent and not a.only_off:
            this, parent = off_across_builds(__file__, ["--n", n, "--rounds", a.rounds], a.parent, a.process_repeats,
                                             lambda run: run["sizes"][str(n)]["setups"]["mlp"]["median_us"], 900)
            res["parent_comparison"] = {"mlp": compare_off(this, parent, res["setups"]["mlp"])}
        sizes[str(n)] = res
    out = {"what": "per-step time of config 4 with autoreset (max_episode_steps 64), episode streams, features of 16 columns x 4 frames float32, controls "
                   "of 4 axes and the rollout (T = 128, E = 2), the policy (hidden (64, 64) actor and critic, tanh, sampling) without a core (mlp) and "
                   "behind a GRU cell of width 64 with soft and with hard gates; the same cell and nets by hand in eager torch; and the policy without "
                   "a core of this build against the parent's in fresh processes",
           "kernel": "v_mfma_f32_32x32x2_f32 (npb_policy_core.hip)", "sizes": sizes, "head": head(ROOT)}
    if a.resources:
        out["kernel_resources"] = resources(a.resources)
    write_line(out, a.out)


if __name__ == "__main__":
    main()
