"""What the column statistics (npb_set_column_stats) cost on BASELINE config 4 at 65 536 and 32 768 plants.

action_test("oil_top_off", range(n), dt = 5) with autoreset from a bank of `--bank` scenarios, device noise and a constant setpoint: no
per-step host input.  Eight columns -- three carried fp64 members, an output member, an int32 member, an info column, an obs column and
the reward --, every statistic, two limits.  One handle per size throughout; statistics and records are switched on and off on it
between blocks, in an order that rotates from round to round.  Setups, event-timed us per step:
  off         statistics off, no episode ending
  on          statistics on, no episode ending: the fold's launch behind every step
  on_records  statistics on and episode records copying and clearing them; episodes of 100 steps, the plants' episode clocks staggered
              beforehand by group p % 100, so about 1 % of the plants truncate on every timed step
  records     the same episodes with records but without statistics: what on_records is to be held against
Reported per setup: the per-step time of each block (median, quartiles, min..max over the blocks), and on minus off of the same round.
The condition that follows from the bytes: the fold moves at most about 104 B per cell, 8 x 65 536 cells = 55 MB against the step's 451
MB, plus one light launch, so it should cost under a quarter of the step it follows (`fold_under_a_quarter_of_the_step`).

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
BUSY_EPISODE = 100
COLUMNS = [("pump.oil_level", 0), ("pump.oil_level", 1), ("pump.oil_level", 2), ("sg.tube_wall_temp", 0), "maint.maintenance_actions_performed",
           ("info", "electrical_power"), ("obs", 5), "reward"]
LIMITS = {0: ("<", 60.0), 5: (">", 845.0)}
STATS = ("min", "max", "sum", "sumsq", "last", "first_beyond", "n_beyond")


def measure(n, block, rounds, bank, only_off):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=5.0, autoreset=True, bank_seeds=list(range(1000, 1000 + bank)), noise_generator="device")
    has_stats = hasattr(env, "enable_column_stats") and not only_off
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    sp = torch.full((n,), 90.0, dtype=torch.float64, device=dev)
    groups = ((torch.arange(n, device=dev) % BUSY_EPISODE).view(1, n) == torch.arange(BUSY_EPISODE, device=dev).view(-1, 1)).to(torch.uint8)
    setups = ["off"] + (["on", "on_records", "records"] if has_stats else [])
    rates = {}

    def run_block(setup):
        busy = setup in ("on_records", "records")
        if hasattr(env, "disable_episode_records"):
            env.disable_episode_records()
        if has_stats:
            env.enable_column_stats(COLUMNS, LIMITS, STATS) if setup in ("on", "on_records") else env.enable_column_stats(None)
        env._enable_autoreset(BUSY_EPISODE if busy else None)      # the episode limit of the setup; the counters begin at zero
        env.restore_from_bank()
        if busy:
            env.enable_episode_records()                           # copies and clears the statistics where they are on
            for k in range(BUSY_EPISODE):                          # stagger the episode clocks: group k truncates at steps k + 100 j
                env.step(power_setpoint=sp)
                env.restore_from_bank(groups[k])
        for _ in range(W):
            env.step(power_setpoint=sp)
        before = env.step(power_setpoint=sp)[3]["episode_index"].sum().item()
        us = time_steps(stream, lambda: env.step(power_setpoint=sp), block)
        after = env.step(power_setpoint=sp)[3]["episode_index"].sum().item()
        rates[setup] = 100.0 * (after - before) / (block + 1) / n
        if busy:                                                   # the drain is the caller's, outside the timed steps; nothing may have been dropped
            env.episode_records()
        return us

    blocks = rotated_blocks(setups, rounds, run_block)
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": block, "rounds": rounds,
           "bank_entries": bank, "columns": len(COLUMNS), "statistics": list(STATS), "limits": len(LIMITS),
           "setups": {s: stats(v) for s, v in blocks.items()}, "ended_percent_of_plants_per_step": dict(rates)}
    if has_stats:
        out["fold_cost_us_per_step"] = paired(blocks, "on", "off")
        out["fold_and_record_copy_cost_us_per_step"] = paired(blocks, "on_records", "records")
        out["fold_percent_of_the_step"] = 100.0 * out["fold_cost_us_per_step"]["median"] / out["setups"]["off"]["median_us"]
        out["fold_under_a_quarter_of_the_step"] = bool(out["fold_cost_us_per_step"]["median"] < 0.25 * out["setups"]["off"]["median_us"])
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--block", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bank", type=int, default=64, help="entries of the start bank")
    ap.add_argument("--bench-steps", type=int, default=200)
    add_parent_arguments(ap, "column_stats_overhead.json")
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
    out = {"what": "per-step time of config 4 with autoreset from a bank and device noise: column statistics (8 columns, every statistic, two limits) "
                   "off and on, and on with episode records copying and clearing them at about 1 % of the plants ending per step",
           "sizes": sizes, "head": head(ROOT)}
    if a.parent and not a.only_off:
        out["bench"] = bench_alternated(a.parent, a.process_repeats, a.bench_steps, 20)
    write_line(out, a.out)


if __name__ == "__main__":
    main()
