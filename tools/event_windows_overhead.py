"""What the event windows (npb_set_event_windows) cost on BASELINE config 4 at 65 536 and 32 768 plants.

action_test("oil_top_off", range(n), dt = 5) with autoreset from a bank of `--bank` scenarios, device noise and a constant setpoint: no
per-step host input.  Eight recorded columns -- three carried fp64 members, an output member, an int32 member, an info column, an obs
column and the reward --, pre = post = 8, one trigger: the plant clock passing a limit, so that what fires and when is set by the
episodes.  One handle per size throughout; the
windows are switched on and off on it between blocks, in an order that rotates from round to round.  Setups, event-timed us per step:
  off        windows off, no episode ending
  quiet      windows on, nothing firing (the limit is never reached): the ring stores and the trigger of every plant behind every step
  busy       windows on; episodes of 100 steps, the plants' episode clocks staggered beforehand by group p % 100, the limit passed at
             step 50 of every episode: about 1 % of the plants arm and about 1 % capture on every timed step
  busy_off   the same episodes without windows: what busy is to be held against
  burst      windows on, no episode ending, every plant passing the limit on the same step of the block and capturing 8 steps later:
             reported as the extra time of the whole block against off, and against quiet: what one capture of every plant costs
Reported per setup: the per-step time of each block (median, quartiles, min..max over the blocks), and on minus off of the same round.
What the bytes say: the quiet launch stores (8 + 1) x 8 B into the ring and reads and writes about 30 B of bookkeeping per plant, 6.7 MB
at 65 536 plants against the step's 451 MB.

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
PRE = POST = 8
BUSY_EPISODE = 100
DT = 5.0
COLUMNS = [("pump.oil_level", 0), ("pump.oil_level", 1), ("pump.oil_level", 2), ("sg.tube_wall_temp", 0), "maint.maintenance_actions_performed",
           ("info", "electrical_power"), ("obs", 5), "reward"]


def measure(n, block, rounds, bank, only_off):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, autoreset=True, bank_seeds=list(range(1000, 1000 + bank)), noise_generator="device")
    has = hasattr(env, "enable_event_windows") and not only_off
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    sp = torch.full((n,), 90.0, dtype=torch.float64, device=dev)
    groups = ((torch.arange(n, device=dev) % BUSY_EPISODE).view(1, n) == torch.arange(BUSY_EPISODE, device=dev).view(-1, 1)).to(torch.uint8)
    setups = ["off"] + (["quiet", "busy", "busy_off", "burst"] if has else [])
    # the plant clock after local step k of an episode is DT (k + 1): passed at step 50 of an episode / at step W + 20 of a block / never
    limit = {"quiet": 1e30, "busy": DT * 50 + 0.5 * DT, "burst": DT * (W + 20) + 0.5 * DT}
    rates, captured = {}, {}

    def run_block(setup):
        busy = setup in ("busy", "busy_off")
        if has:
            if setup in limit:      # room for every capture of the block: none is dropped, every window is copied
                env.enable_event_windows(COLUMNS, [("prim.sim_time", ">", limit[setup])], PRE, POST, capacity=4 * n if busy else n)
            else:
                env.enable_event_windows(None)
        env._enable_autoreset(BUSY_EPISODE if busy else None)      # the episode limit of the setup; the counters begin at zero
        env.restore_from_bank()                                    # every plant's clock back to 0
        if busy:
            for k in range(BUSY_EPISODE):                          # stagger the episode clocks: group k truncates at steps k + 100 j
                env.step(power_setpoint=sp)
                env.restore_from_bank(groups[k])
        for _ in range(W):
            env.step(power_setpoint=sp)
        before = env.step(power_setpoint=sp)[3]["episode_index"].sum().item()
        if has and setup in limit:
            env._ewin["cursor"].zero_()
        us = time_steps(stream, lambda: env.step(power_setpoint=sp), block)
        after = env.step(power_setpoint=sp)[3]["episode_index"].sum().item()
        rates[setup] = 100.0 * (after - before) / (block + 1) / n
        if has and setup in limit:                                 # captures per plant and timed step, in percent; nothing may have been dropped
            count = int(env._ewin["cursor"].item()) & 0xFFFFFFFF
            assert count <= env._ewin["capacity"], (setup, count)
            captured[setup] = 100.0 * count / (block + 1) / n
        return us

    blocks = rotated_blocks(setups, rounds, run_block)

    def per_block(cost):      # a per-step difference as that of the whole block
        return {k: v * float(block) for k, v in cost.items()}
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": block, "rounds": rounds,
           "bank_entries": bank, "columns": len(COLUMNS), "pre": PRE, "post": POST,
           "setups": {s: stats(v) for s, v in blocks.items()}, "ended_percent_of_plants_per_step": dict(rates),
           "captured_percent_of_plants_per_step": dict(captured)}
    if has:
        env.enable_event_windows(COLUMNS, [("prim.sim_time", ">", limit["quiet"])], PRE, POST, capacity=1)
        out["ring_and_bookkeeping_bytes"] = env._ewin["bytes"]
        out["quiet_cost_us_per_step"] = paired(blocks, "quiet", "off")
        out["one_percent_capturing_cost_us_per_step"] = paired(blocks, "busy", "busy_off")
        out["every_plant_capturing_once_cost_us_per_block"] = per_block(paired(blocks, "burst", "off"))
        out["every_plant_capturing_once_beyond_quiet_us_per_block"] = per_block(paired(blocks, "burst", "quiet"))      # the captures alone
        out["quiet_percent_of_the_step"] = 100.0 * out["quiet_cost_us_per_step"]["median"] / out["setups"]["off"]["median_us"]
        env.enable_event_windows(None)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--block", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bank", type=int, default=64, help="entries of the start bank")
    ap.add_argument("--bench-steps", type=int, default=200)
    add_parent_arguments(ap, "event_windows_overhead.json")
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
    out = {"what": "per-step time of config 4 with autoreset from a bank and device noise: event windows (8 columns, pre = post = 8, one limit "
                   "trigger on the plant clock) off, on with nothing firing, on with about 1 % of the plants capturing per step, and on with "
                   "every plant capturing on one step of the block",
           "sizes": sizes, "head": head(ROOT)}
    if a.parent and not a.only_off:
        out["bench"] = bench_alternated(a.parent, a.process_repeats, a.bench_steps, 20)
    write_line(out, a.out)


if __name__ == "__main__":
    main()
