"""What the per-plant work-order summary (npb_set_maintenance_summary) costs on BASELINE config 4 at 65 536 and 32 768 plants.

action_test("oil_top_off", range(n), dt = 5), one handle per size throughout.  The batch is snapshotted once, and every timed block of
every setup replays the same simulated interval: restore(), the oil level of pump FWP-1 set for the setup's state, the same pre-drawn
heat-source noise rows, 8 untimed steps (switching the summary re-uploads the rule's constants and has the rule look at
every wave once), then `--block` steps between two events.  Two states:
  quiet   FWP-1's oil at 100 % in every plant: nothing fires in the interval
  busy    FWP-1's oil spread evenly over [58, 58 + --busy-span] %, so that the plants' oil_top_off orders are created, and three steps
          later completed, at a steady rate through the interval: about 1 % of the plants produce an event per step (the achieved rate
          is counted from the summary's own tables and reported)
and per state the summary off and on (consume mode, two keys), in an order that rotates from round to round.  Reported per setup: the
per-step time of each block (mean, median, quartiles, min, max over the blocks) and, for the summary, on minus off of the same state.

--parent DIR: a checkout of the parent commit, built.  The summary-off setups are then also measured in fresh processes, alternately on
this build and on the parent's (this script run with --package-root), `--process-repeats` times each, and held against each other setup by
setup by overhead_harness.compare_off.  One JSON line per run, all sizes in one object, also written to --out.
"""
import argparse
import os
import sys

import numpy as np

from overhead_harness import add_parent_arguments, compare_off, head, off_across_builds, paired, rotated_blocks, stats, time_steps, write_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [("feedwater", None, None), "oil_top_off"]
W = 8


def measure(n, block, rounds, busy_span, only_off):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), noise_generator="device")
    has_summary = hasattr(env, "enable_maintenance_summary")
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    sp = torch.full((n,), 95.0, dtype=torch.float64, device=dev)
    gen = torch.Generator(device=dev); gen.manual_seed(42)
    z = torch.randn((W + block, n), device=dev, dtype=torch.float64, generator=gen)
    level = {"quiet": torch.full((n,), 100.0, dtype=torch.float64, device=dev),
             "busy": 58.0 + busy_span * (torch.arange(n, dtype=torch.float64, device=dev) + 0.5) / n}
    env.snapshot()
    setups = [(s, on) for s in ("quiet", "busy") for on in ((False,) if only_off or not has_summary else (False, True))]
    events = {}

    def run_block(setup):
        state, on = setup
        env.restore()
        env.set_field("pump.oil_level", level[state], instance=0)
        if has_summary:
            env.enable_maintenance_summary(KEYS if on else None)
        for t in range(W):
            env.step(power_setpoint=sp, noise_z=z[t])
        if on:
            env.clear_maintenance_summary()
        t = iter(range(W, W + block))      # the block's noise rows, one per step
        us = time_steps(stream, lambda: env.step(power_setpoint=sp, noise_z=z[next(t)]), block)
        if on:
            s = env.maintenance_summary()
            events[state] = {"events_per_step": float((s["n_created"][0].sum() + s["n_completed"][0].sum()).item()) / block,
                             "dropped": int(s["dropped"].item())}
        return us

    blocks = rotated_blocks(setups, rounds, run_block)
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": block, "rounds": rounds,
           "setups": {"%s_%s" % (s, "on" if on else "off"): dict(stats(v), mean_us=float(np.mean(v))) for (s, on), v in blocks.items()},
           "events": events}
    for s in ("quiet", "busy"):
        if (s, True) in blocks:      # this script reports the mean beside the harness's median, min and max
            out["summary_cost_us_per_step_" + s] = dict(paired(blocks, (s, True), (s, False)), mean=float(np.mean(blocks[(s, True)]) - np.mean(blocks[(s, False)])))
            out["events"][s]["percent_of_plants_per_step"] = 100.0 * events[s]["events_per_step"] / n
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--block", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--busy-span", type=float, default=16.4, help="oil-level span [%%] the busy state's FWP-1 levels are spread over")
    add_parent_arguments(ap, "maintenance_summary_overhead.json")
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    sizes = {}
    for n in a.n:
        res = measure(n, a.block, a.rounds, a.busy_span, a.only_off)
        if a.parent and not a.only_off:
            this, parent = off_across_builds(__file__, ["--n", n, "--block", a.block, "--rounds", a.rounds, "--busy-span", a.busy_span], a.parent,
                                             a.process_repeats, lambda run: run["sizes"][str(n)]["setups"], 600)
            res["parent_comparison"] = {s: compare_off([r[s]["median_us"] for r in this], [r[s]["median_us"] for r in parent], res["setups"][s])
                                        for s in ("quiet_off", "busy_off")}
        sizes[str(n)] = res
    out = {"what": "per-step time of config 4 with the work-order summary off and on (consume mode, %d keys), nothing firing and about 1 %% "
                   "of the plants producing an event per step; every block replays the same simulated interval" % len(KEYS),
           "expectation": "one launch per quiet fold: +3.5 to +5.9 us measured for an empty operator call on the same machine (README)",
           "sizes": sizes, "head": head(ROOT)}
    write_line(out, a.out)


if __name__ == "__main__":
    main()
