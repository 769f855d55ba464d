"""What episode streams (npb_set_episode_streams) cost on BASELINE config 4 at 65 536 and 32 768 plants.

action_test("oil_top_off", range(n), dt = 5) with autoreset from a bank of `--bank` scenarios, the runner's power profile of `--profile`
steps and device noise: no per-step host input.  One handle per size throughout; the mode is switched on and off on it between
blocks.  Three states, each with the mode off and on, in an order that rotates from round to round:
  quiet   no episode limit and no scram: nothing restarts.  On minus off is what the mode costs a step on which nothing happens -- the
          restart kernel's one vote per wave, the rows taken into the output columns, and the handle's refills against PowerProfile's.
  busy    episodes of 100 steps, the plants' episode clocks staggered beforehand (100 untimed steps, one group of n / 100 plants restored
          from the bank after each), so that about 1 % of the plants truncate on every timed step; the achieved rate is counted from the
          episode indices and reported.
  worst   episodes of `--worst-steps` steps begun together: every step of such an episode is timed on its own, and the one step on
          which every plant truncates at once is reported by itself, beside the median of the others.  With the mode on its restart
          kernel seeds both generators of the whole batch anew and makes the rows pending in the handle's blocks again.
Reported per setup: the per-step time of each block (mean, median, quartiles, min, max over the blocks) and on minus off of the same
state and round.

--parent DIR: a checkout of the parent commit, built.  The mode-off setups are then also measured in fresh processes, alternately on
this build and on the parent's (this script run with --package-root), `--process-repeats` times each, and held against each other setup by
setup by overhead_harness.compare_off.  One JSON line per run, all sizes in one object, also written to --out.
"""
import argparse
import os
import sys

import numpy as np

from overhead_harness import add_parent_arguments, compare_off, head, off_across_builds, paired, rotated_blocks, stats, time_steps, write_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 8
BUSY_EPISODE = 100


def measure(n, block, rounds, profile, bank, worst_steps, stream_block, only_off):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    bank_seeds = list(range(1000, 1000 + bank))
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=5.0, autoreset=True, bank_seeds=bank_seeds, power_profile_steps=profile,
                                      noise_generator="device")
    has_mode = hasattr(env, "enable_episode_streams") and not only_off
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    groups = (torch.arange(n, device=dev) % BUSY_EPISODE).view(1, n) == torch.arange(BUSY_EPISODE, device=dev).view(-1, 1)
    groups = groups.to(torch.uint8)
    limit = {"quiet": None, "busy": BUSY_EPISODE, "worst": worst_steps}
    setups = [(s, on) for s in ("quiet", "busy", "worst") for on in ((False, True) if has_mode else (False,))]
    rates, worst = {}, {s: [] for s in setups}

    def timed(steps):
        return time_steps(stream, env.step, steps)

    def run_block(setup):
        state, on = setup
        if has_mode:
            if env.stream_rows is not None:
                env.disable_episode_streams()
        env._enable_autoreset(limit[state])                # the episode limit of the state; the counters begin at zero
        env.restore_from_bank()
        if has_mode and on:
            env.enable_episode_streams(block=stream_block, bank_noise_seeds=[42] * bank, bank_profile_seeds=bank_seeds)
        if state == "busy":                                # stagger the episode clocks: group k truncates at steps k + 100 j
            for k in range(BUSY_EPISODE):
                env.step()
                env.restore_from_bank(groups[k])
        for _ in range(W):
            env.step()
        if state == "worst":                               # whole episodes begun together, every step timed on its own
            env.restore_from_bank()
            per_step = np.array([[timed(1) for _ in range(worst_steps)] for _ in range(max(1, block // worst_steps))])
            worst[(state, on)].append({"truncating_step_us": float(np.median(per_step[:, -1])), "other_steps_us": float(np.median(per_step[:, :-1]))})
            return float(per_step.mean())
        before = env.step()[3]["episode_index"].sum().item()
        us = timed(block)
        after = env.step()[3]["episode_index"].sum().item()
        rates[(state, on)] = 100.0 * (after - before) / (block + 1) / n
        return us

    blocks = rotated_blocks(setups, rounds, run_block)

    def name(s, on):
        return "%s_%s" % (s, "on" if on else "off")
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": block, "rounds": rounds,
           "profile_steps": profile, "bank_entries": bank, "stream_block": stream_block, "worst_episode_steps": worst_steps,
           "setups": {name(*s): dict(stats(v), mean_us=float(np.mean(v))) for s, v in blocks.items()},
           "restarted_percent_of_plants_per_step": {name(*s): v for s, v in rates.items()},
           "worst": {name(*s): {"truncating_step_us": float(np.median([w["truncating_step_us"] for w in v[1:]])),
                                "other_steps_us": float(np.median([w["other_steps_us"] for w in v[1:]]))} for s, v in worst.items() if len(v) > 1}}
    for s in ("quiet", "busy", "worst"):
        if (s, True) in blocks:      # this script reports the mean beside the harness's median, min and max
            out["mode_cost_us_per_step_" + s] = dict(paired(blocks, (s, True), (s, False)), mean=float(np.mean(blocks[(s, True)]) - np.mean(blocks[(s, False)])))
    if "worst_on" in out["worst"]:
        out["mode_cost_us_truncating_step"] = out["worst"]["worst_on"]["truncating_step_us"] - out["worst"]["worst_off"]["truncating_step_us"]
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--block", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--profile", type=int, default=288, help="rows of the power profile")
    ap.add_argument("--bank", type=int, default=64, help="entries of the start bank")
    ap.add_argument("--worst-steps", type=int, default=16, help="episode length of the worst state")
    ap.add_argument("--stream-block", type=int, default=64, help="rows the handle draws at a time with the mode on")
    add_parent_arguments(ap, "episode_streams_overhead.json")
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    sizes = {}
    for n in a.n:
        res = measure(n, a.block, a.rounds, a.profile, a.bank, a.worst_steps, a.stream_block, a.only_off)
        if a.parent and not a.only_off:
            argv = ["--n", n, "--block", a.block, "--rounds", a.rounds, "--profile", a.profile, "--bank", a.bank, "--worst-steps", a.worst_steps]
            this, parent = off_across_builds(__file__, argv, a.parent, a.process_repeats, lambda run: run["sizes"][str(n)]["setups"], 900)
            res["parent_comparison"] = {s: compare_off([r[s]["median_us"] for r in this], [r[s]["median_us"] for r in parent], res["setups"][s])
                                        for s in ("quiet_off", "busy_off", "worst_off")}
        sizes[str(n)] = res
    out = {"what": "per-step time of config 4 with autoreset from a bank, a power profile and device noise, episode streams off and on: nothing "
                   "restarting, about 1 % of the plants truncating per step, and the one step on which every plant truncates at once",
           "sizes": sizes, "head": head(ROOT)}
    write_line(out, a.out)


if __name__ == "__main__":
    main()
