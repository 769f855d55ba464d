"""What the episode records (npb_set_episode_records) cost on BASELINE config 4 at 65 536 and 32 768 plants.

action_test("oil_top_off", range(n), dt = 5) with autoreset from a bank of `--bank` scenarios, device noise, a constant setpoint and a
two-key work-order summary: no per-step host input.  One handle per size throughout; the records are switched on and off on it between
blocks, in an order that rotates from round to round.  Setups:
  a  quiet_off     no episode limit and no scram: nothing ends; records off
  b  quiet_on      the same with records on (summary copied and cleared, no final_obs): the extra launch, whose waves all leave at the vote
  c  busy_off/on   episodes of 100 steps, the plants' episode clocks staggered beforehand by group p % 100 (100 untimed steps, one group
                   restored from the bank after each), so about 1 % of the plants truncate on every timed step, in a wave one lane at the most
  d  worst_off/on  episodes of `--worst-steps` steps begun together, every step timed on its own: the one step on which every plant
                   truncates at once is reported by itself, beside the median of the others
  e  busy_composed the host path the records replace, at 1 %: records off; after every step the host reads done | truncated (one
                   synchronisation), gathers the ended plants' episode columns and summary rows on the device, copies them to the host and
                   clears those summary rows (clear_maintenance_summary(mask))
busy_off - quiet_off and the truncating step of worst_off against its other steps are the episode kernel's own cost on the same steps.
Reported per setup: the per-step time of each block (mean, median, quartiles, min, max over the blocks), and on minus off of the same
state and round.

--parent DIR: a checkout of the parent commit, built.  quiet_off is then also measured in fresh processes, alternately on this build
and on the parent's (this script run with --package-root and --only-off), `--process-repeats` times each, and held against each other by
overhead_harness.compare_off; bench.py is run alternately from the two trees.  One JSON line per run, all sizes in one object, also
written to --out.
"""
import argparse
import os
import sys

import numpy as np

from overhead_harness import (add_parent_arguments, bench_alternated, compare_off, head, off_across_builds, paired, rotated_blocks, stats,
                              time_steps, write_line)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 8
BUSY_EPISODE = 100
KEYS = ["oil_top_off", ("feedwater", None, None)]


def measure(n, block, rounds, bank, worst_steps, only_off):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=5.0, autoreset=True, bank_seeds=list(range(1000, 1000 + bank)), noise_generator="device")
    env.enable_maintenance_summary(KEYS)
    has_records = hasattr(env, "enable_episode_records") and not only_off
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    sp = torch.full((n,), 90.0, dtype=torch.float64, device=dev)
    groups = ((torch.arange(n, device=dev) % BUSY_EPISODE).view(1, n) == torch.arange(BUSY_EPISODE, device=dev).view(-1, 1)).to(torch.uint8)
    limit = {"quiet": None, "busy": BUSY_EPISODE, "worst": worst_steps}
    setups = [("quiet", "off")] + ([("quiet", "on"), ("busy", "off"), ("busy", "on"), ("busy", "composed"), ("worst", "off"), ("worst", "on")] if has_records else [])
    rates, worst, composed_rows = {}, {s: [] for s in setups}, []

    def step(how):
        _obs, _rew, done, info = env.step(power_setpoint=sp)
        if how != "composed":
            return info
        ended = (done != 0) | (info["truncated"] != 0)
        idx = torch.nonzero(ended).flatten()              # the host learns who ended: one synchronisation per step
        if idx.numel():
            S = env.maintenance_summary()
            cols = [info[k][idx] for k in ("episode_length", "episode_return", "episode_index", "episode_start", "trip_flags", "time")]
            cols += [S[k][:, idx] for k in ("first_created", "first_completed", "n_created", "n_completed")]
            host = [c.cpu() for c in cols]
            composed_rows.append(int(host[0].numel()))
            env.clear_maintenance_summary(ended)
        return info

    def timed(steps, how):
        return time_steps(stream, lambda: step(how), steps)

    def run_block(setup):
        state, how = setup
        if has_records:
            env.disable_episode_records()
        env._enable_autoreset(limit[state])                # the episode limit of the state; the counters begin at zero
        env.restore_from_bank()
        env.clear_maintenance_summary()
        if how == "on":
            # (room for every episode of the block: the worst state ends n of them every worst_steps steps)
            env.enable_episode_records(n * (block // worst_steps + 2) if state == "worst" else None, summary=True, clear_summary=True)
        if state == "busy":                                # stagger the episode clocks: group k truncates at steps k + 100 j
            for k in range(BUSY_EPISODE):
                env.step(power_setpoint=sp)
                env.restore_from_bank(groups[k])
        for _ in range(W):
            step(how)
        if state == "worst":                               # whole episodes begun together, every step timed on its own
            env.restore_from_bank()
            per_step = np.array([[timed(1, how) for _ in range(worst_steps)] for _ in range(max(1, block // worst_steps))])
            worst[(state, how)].append({"truncating_step_us": float(np.median(per_step[:, -1])), "other_steps_us": float(np.median(per_step[:, :-1]))})
            us = float(per_step.mean())
        else:
            before = step(how)["episode_index"].sum().item()
            us = timed(block, how)
            after = step(how)["episode_index"].sum().item()
            rates[(state, how)] = 100.0 * (after - before) / (block + 1) / n
        if how == "on":                                    # the drain is the caller's, outside the timed steps; nothing may have been dropped
            env.episode_records()
        return us

    blocks = rotated_blocks(setups, rounds, run_block)

    def name(s, how):
        return "%s_%s" % (s, how)

    def cost(a, b):      # this script reports the mean beside the harness's median, min and max
        return dict(paired(blocks, a, b), mean=float(np.mean(blocks[a]) - np.mean(blocks[b])))
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": block, "rounds": rounds,
           "bank_entries": bank, "summary_keys": len(KEYS), "worst_episode_steps": worst_steps,
           "setups": {name(*s): dict(stats(v), mean_us=float(np.mean(v))) for s, v in blocks.items()},
           "ended_percent_of_plants_per_step": {name(*s): v for s, v in rates.items()},
           "worst": {name(*s): {"truncating_step_us": float(np.median([w["truncating_step_us"] for w in v[1:]])),
                                "other_steps_us": float(np.median([w["other_steps_us"] for w in v[1:]]))} for s, v in worst.items() if len(v) > 1}}
    if has_records:
        out["records_cost_us_per_step_quiet"] = cost(("quiet", "on"), ("quiet", "off"))
        out["records_cost_us_per_step_busy"] = cost(("busy", "on"), ("busy", "off"))
        out["composed_cost_us_per_step_busy"] = cost(("busy", "composed"), ("busy", "off"))
        out["records_cost_us_per_step_worst_episode"] = cost(("worst", "on"), ("worst", "off"))
        out["episode_kernel_cost_us_per_step_busy"] = cost(("busy", "off"), ("quiet", "off"))
        out["composed_rows_per_step_median"] = float(np.median(composed_rows)) if composed_rows else 0.0
        if "worst_on" in out["worst"]:
            w = out["worst"]
            out["records_cost_us_truncating_step"] = w["worst_on"]["truncating_step_us"] - w["worst_off"]["truncating_step_us"]
            out["episode_kernel_cost_us_truncating_step"] = w["worst_off"]["truncating_step_us"] - w["worst_off"]["other_steps_us"]
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--block", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bank", type=int, default=64, help="entries of the start bank")
    ap.add_argument("--worst-steps", type=int, default=16, help="episode length of the worst state")
    ap.add_argument("--bench-steps", type=int, default=200)
    add_parent_arguments(ap, "episode_records_overhead.json")
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    sizes = {}
    for n in a.n:
        res = measure(n, a.block, a.rounds, a.bank, a.worst_steps, a.only_off)
        print("%d plants: measured" % n, file=sys.stderr, flush=True)
        if a.parent and not a.only_off:
            this, parent = off_across_builds(__file__, ["--n", n, "--block", a.block, "--rounds", a.rounds, "--bank", a.bank], a.parent, a.process_repeats,
                                             lambda run: run["sizes"][str(n)]["setups"]["quiet_off"]["median_us"], 900)
            res["parent_comparison"] = {"quiet_off": compare_off(this, parent, res["setups"]["quiet_off"])}
        sizes[str(n)] = res
    out = {"what": "per-step time of config 4 with autoreset from a bank, device noise and a two-key work-order summary, episode records off and on: "
                   "nothing ending, about 1 % of the plants truncating per step (one lane of a wave at the most), the one step on which every plant "
                   "truncates at once, and the composed host path at 1 %",
           "sizes": sizes, "head": head(ROOT)}
    if a.parent and not a.only_off:
        out["bench"] = bench_alternated(a.parent, a.process_repeats, a.bench_steps, 20)
    write_line(out, a.out)


if __name__ == "__main__":
    main()
