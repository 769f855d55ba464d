"""What the per-plant work-order summary (npb_set_maintenance_summary) costs on BASELINE config 4 at 65 536 and 32 768 plants.

action_test("oil_top_off", range(n), dt = 5), one handle per size throughout (where an arena lands in physical memory moves the step
time from one handle to the next).  The batch is snapshotted once, and every timed block of every setup replays the same simulated
interval: restore(), the oil level of pump FWP-1 set for the setup's state, the same pre-drawn heat-source noise rows, 8 untimed steps
(switching the summary re-uploads the rule's constants and has the rule look at every wave once), then `--block` steps between two
events.  Two states:
  quiet   FWP-1's oil at 100 % in every plant: nothing fires in the interval
  busy    FWP-1's oil spread evenly over [58, 58 + --busy-span] %, so that the plants' oil_top_off orders are created, and three steps
          later completed, at a steady rate through the interval: about 1 % of the plants produce an event per step (the achieved rate
          is counted from the summary's own tables and reported)
and per state the summary off and on (consume mode, two keys), in an order that rotates from round to round.  Reported per setup: the
per-step time of each block (mean, median, quartiles, min, max over the blocks) and, for the summary, on minus off of the same state.

--parent DIR: a checkout of the parent commit, built.  The summary-off setups are then also measured in fresh processes, alternately on
this build and on the parent's (this script run with --package-root), `--process-repeats` times each; `off_agrees` says whether the two
builds' medians differ by no more than the spread of this build's own repeats (blocks and processes).  One JSON line per run, all sizes
in one object, also written to --out.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

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

    def run_block(state, on):
        env.restore()
        env.set_field("pump.oil_level", level[state], instance=0)
        if has_summary:
            env.enable_maintenance_summary(KEYS if on else None)
        for t in range(W):
            env.step(power_setpoint=sp, noise_z=z[t])
        if on:
            env.clear_maintenance_summary()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for k in range(block):
            env.step(power_setpoint=sp, noise_z=z[W + k])
        b.record(stream)
        b.synchronize()
        if on:
            s = env.maintenance_summary()
            events[state] = {"events_per_step": float((s["n_created"][0].sum() + s["n_completed"][0].sum()).item()) / block,
                             "dropped": int(s["dropped"].item())}
        return a.elapsed_time(b) * 1e3 / block

    for s in setups:      # warm-up
        run_block(*s)
    blocks = {s: [] for s in setups}
    for r in range(rounds):
        k = r % len(setups)
        for s in setups[k:] + setups[:k]:
            blocks[s].append(run_block(*s))
    torch.cuda.synchronize(dev)

    def stats(v):
        v = np.asarray(v)
        return {"mean_us": float(v.mean()), "median_us": float(np.median(v)), "p25_us": float(np.percentile(v, 25)),
                "p75_us": float(np.percentile(v, 75)), "min_us": float(v.min()), "max_us": float(v.max()), "blocks": int(v.size)}
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": block, "rounds": rounds,
           "setups": {"%s_%s" % (s, "on" if on else "off"): stats(v) for (s, on), v in blocks.items()}, "events": events}
    for s in ("quiet", "busy"):
        if (s, True) in blocks:
            d = np.asarray(blocks[(s, True)]) - np.asarray(blocks[(s, False)])      # the same round's blocks, paired
            out["summary_cost_us_per_step_" + s] = {"median": float(np.median(d)), "mean": float(d.mean()), "min": float(d.min()), "max": float(d.max())}
            out["events"][s]["percent_of_plants_per_step"] = 100.0 * events[s]["events_per_step"] / n
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--block", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--busy-span", type=float, default=16.4, help="oil-level span [%%] the busy state's FWP-1 levels are spread over")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: compare the summary-off setups across the two builds")
    ap.add_argument("--process-repeats", type=int, default=2)
    ap.add_argument("--package-root", default=ROOT, help="where nuclear_sim_amd is imported from (used for the parent's build)")
    ap.add_argument("--only-off", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maintenance_summary_overhead.json"))
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    sizes = {}
    for n in a.n:
        res = measure(n, a.block, a.rounds, a.busy_span, a.only_off)
        if a.parent and not a.only_off:
            runs = {"this": [], "parent": []}
            for _ in range(a.process_repeats):
                for which, root in (("this", ROOT), ("parent", os.path.abspath(a.parent))):
                    cmd = [sys.executable, os.path.abspath(__file__), "--n", str(n), "--block", str(a.block), "--rounds", str(a.rounds),
                           "--busy-span", str(a.busy_span), "--package-root", root, "--only-off", "--out", ""]
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                    if p.returncode != 0:
                        raise SystemExit("the %s build's run failed:\n%s" % (which, p.stderr[-2000:]))
                    runs[which].append(json.loads(p.stdout.strip().splitlines()[-1])["sizes"][str(n)]["setups"])
            cmp = {}
            for s in ("quiet_off", "busy_off"):
                mine = [r[s]["median_us"] for r in runs["this"]] + [res["setups"][s]["median_us"]]
                theirs = [r[s]["median_us"] for r in runs["parent"]]
                spread = max(max(mine) - min(mine), res["setups"][s]["max_us"] - res["setups"][s]["min_us"])
                diff = float(np.median(theirs) - np.median(mine))
                cmp[s] = {"this_medians_us": mine, "parent_medians_us": theirs, "parent_minus_this_us": diff,
                          "this_spread_us": float(spread), "off_agrees": bool(abs(diff) <= spread)}
            res["parent_comparison"] = cmp
        sizes[str(n)] = res
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        head = None
    out = {"what": "per-step time of config 4 with the work-order summary off and on (consume mode, %d keys), nothing firing and about 1 %% "
                   "of the plants producing an event per step; every block replays the same simulated interval" % len(KEYS),
           "expectation": "one launch per quiet fold: +3.5 to +5.9 us measured for an empty operator call on the same machine (README)",
           "sizes": sizes, "head": head}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
