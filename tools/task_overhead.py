"""What a task (npb_set_task: caller-defined reward terms and termination rules) costs on BASELINE config 4 at 65 536 and 32 768 plants.

action_test("oil_top_off", range(n), dt = 5) with autoreset from a bank of `--bank` scenarios, device noise and a constant setpoint: no
per-step host input.  The task has 8 terms -- the step's reward, an info column against a constant, an obs column against another, a
limit and an excess on carried members, the trip flags' pump bits, and the deltas of the event count and of an oil level -- and 3 rules:
the scram pulse, a limit on the plant clock, and NONFINITE on the reward.  One handle per size throughout; the task is set and dropped on it
between blocks, in an order that rotates from round to round.  Setups, event-timed us per step:
  off        no task, no episode ending
  quiet      task on, nothing firing (the clock limit is never reached): the one launch behind every step
  terms      the same with keep_terms: 8 more stores per plant
  busy       task on; the clock rule ends every episode at its step 100, the plants' episode clocks staggered beforehand by group
             p % 100: about 1 % of the plants are ended BY THE TASK and restart from the bank on every timed step
  busy_off   the same episodes without a task, ended by max_episode_steps = 100: what busy is to be held against
  stats      no task, column statistics of 8 columns on        } kernels of the same shape behind the same step,
  windows    no task, event windows of 8 columns on, quiet     } from the same run, to set the task's figure beside
Reported per setup: the per-step time of each block (median, quartiles, min..max over the blocks), and on minus off of the same round.
What the bytes say: the quiet launch reads about 11 values and the bookkeeping and stores a reward, a flag, a cause word and two
previous samples per plant, some 150 B: 10 MB at 65 536 plants against the step's 451 MB.

--parent DIR: a checkout of the parent commit, built.  `off` is then also measured in fresh processes, alternately on this build and on
the parent's (this script run with --package-root and --only-off), `--process-repeats` times each, and held against each other by
overhead_harness.compare_off.  bench.py is run alternately from the two trees and its ms per step printed beside it.  One JSON line per
run, all sizes in one object, also written to --out.
"""
import argparse
import os
import sys

from overhead_harness import (add_parent_arguments, bench_alternated, compare_off, head, off_across_builds, paired, rotated_blocks, stats,
                              time_steps, write_line)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 8
EPISODE = 100
DT = 5.0
COLUMNS = [("pump.oil_level", 0), ("pump.oil_level", 1), ("pump.oil_level", 2), ("sg.tube_wall_temp", 0), "maint.maintenance_actions_performed",
           ("info", "electrical_power"), ("obs", 5), "reward"]


def task_of(clock_limit):
    """8 terms, 3 rules; only the clock rule can fire in these runs"""
    terms = [("reward", 1.0), (("info", "electrical_power"), -0.001, "abs_err", 790.0), (("obs", 5), 0.5, "sq_err", ("obs", 6)),
             (("pump.oil_level", 0), -0.25, "beyond", "<", -1.0), (("sg.tube_wall_temp", 1), -0.01, "excess", ">", 1e9),
             ("flags", -3.0, "bits", 0xF00), ("maintenance", -2.0, "delta"), (("pump.oil_level", 1), 1.5, "delta")]
    rules = [("done", -100.0), ("prim.sim_time", ">", clock_limit, -1.0), ("reward", "nonfinite", -5.0)]
    return dict(reward=terms, terminate=rules, bias=0.125)


def measure(n, block, rounds, bank, only_off):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, autoreset=True, bank_seeds=list(range(1000, 1000 + bank)), noise_generator="device")
    has = hasattr(env, "set_task") and not only_off
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    sp = torch.full((n,), 90.0, dtype=torch.float64, device=dev)
    groups = ((torch.arange(n, device=dev) % EPISODE).view(1, n) == torch.arange(EPISODE, device=dev).view(-1, 1)).to(torch.uint8)
    setups = ["off"] + (["quiet", "terms", "busy", "busy_off", "stats", "windows"] if has else [])
    # the plant clock after local step k of an episode is DT (k + 1): the rule fires on step 100 of an episode, or never
    clock = {"quiet": 1e30, "terms": 1e30, "busy": DT * EPISODE - 0.5 * DT}
    rates, by_task = {}, {}

    def run_block(setup):
        busy = setup in ("busy", "busy_off")
        if has:
            env.enable_column_stats(COLUMNS if setup == "stats" else None)
            env.enable_event_windows(COLUMNS if setup == "windows" else None, [("prim.sim_time", ">", 1e30)], 8, 8, capacity=n)
            if setup in clock:
                env.set_task(keep_terms=setup == "terms", **task_of(clock[setup]))
            else:
                env.set_task(None)
        env._enable_autoreset(EPISODE if setup == "busy_off" else None)      # the episode limit of the setup; the counters begin at zero
        env.restore_from_bank()                                              # every plant's clock back to 0
        if busy:
            for k in range(EPISODE):                                         # stagger the episode clocks: group k ends at steps k + 100 j
                env.step(power_setpoint=sp)
                env.restore_from_bank(groups[k])
        for _ in range(W):
            env.step(power_setpoint=sp)
        first = env.step(power_setpoint=sp)
        before = first[3]["episode_index"].sum().item()
        us = time_steps(stream, lambda: env.step(power_setpoint=sp), block)
        last = env.step(power_setpoint=sp)
        rates[setup] = 100.0 * (last[3]["episode_index"].sum().item() - before) / (block + 1) / n
        if setup in clock:      # of this last step: plants the task ended, in percent
            by_task[setup] = 100.0 * float((last[3]["task_cause"] != 0).sum().item()) / n
        return us

    blocks = rotated_blocks(setups, rounds, run_block)
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": block, "rounds": rounds,
           "bank_entries": bank, "terms": 8, "rules": 3, "setups": {s: stats(v) for s, v in blocks.items()},
           "ended_percent_of_plants_per_step": dict(rates), "ended_by_the_task_percent_of_plants_on_the_last_step": dict(by_task)}
    if has:
        out["quiet_cost_us_per_step"] = paired(blocks, "quiet", "off")
        out["keep_terms_cost_us_per_step"] = paired(blocks, "terms", "off")
        out["one_percent_ending_cost_us_per_step"] = paired(blocks, "busy", "busy_off")
        out["column_stats_cost_us_per_step"] = paired(blocks, "stats", "off")
        out["event_windows_quiet_cost_us_per_step"] = paired(blocks, "windows", "off")
        out["quiet_percent_of_the_step"] = 100.0 * out["quiet_cost_us_per_step"]["median"] / out["setups"]["off"]["median_us"]
        env.set_task(None)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--block", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bank", type=int, default=64, help="entries of the start bank")
    ap.add_argument("--bench-steps", type=int, default=200)
    add_parent_arguments(ap, "task_overhead.json")
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    sizes = {}
    for n in a.n:
        res = measure(n, a.block, a.rounds, a.bank, a.only_off)
        print("%d plants: measured" % n, file=sys.stderr, flush=True)
        if a.parent and not a.only_off:
            this, parent = off_across_builds(__file__, ["--n", n, "--block", a.block, "--rounds", a.rounds, "--bank", a.bank], a.parent, a.process_repeats,
                                             lambda run: run["sizes"][str(n)]["setups"]["off"]["median_us"], 900)
            res["parent_comparison"] = {"off": compare_off(this, parent, res["setups"]["off"])}
        sizes[str(n)] = res
    out = {"what": "per-step time of config 4 with autoreset from a bank and device noise: a task of 8 reward terms and 3 termination rules off, "
                   "on with nothing firing, on with keep_terms, on with about 1 % of the plants ended by it per step; column statistics and "
                   "event windows of 8 columns each beside it, from the same run",
           "sizes": sizes, "head": head(ROOT)}
    if a.parent and not a.only_off:
        out["bench"] = bench_alternated(a.parent, a.process_repeats, a.bench_steps, 20)
    write_line(out, a.out)


if __name__ == "__main__":
    main()
