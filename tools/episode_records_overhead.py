"""What the episode records (npb_set_episode_records) cost on BASELINE config 4 at 65 536 and 32 768 plants.

action_test("oil_top_off", range(n), dt = 5) with autoreset from a bank of `--bank` scenarios, device noise, a constant setpoint and a
two-key work-order summary: no per-step host input.  One handle per size throughout (where an arena lands in physical memory moves the
step time from one handle to the next); the records are switched on and off on it between blocks, in an order that rotates from round
to round.  Setups:
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
and on the parent's (this script run with --package-root and --only-off), `--process-repeats` times each, and bench.py is run
alternately from the two trees.  One JSON line per run, all sizes in one object, also written to --out.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

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
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(steps):
            step(how)
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / steps

    def run_block(state, how):
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

    def name(s, how):
        return "%s_%s" % (s, how)

    def paired(a, b):
        d = np.asarray(blocks[a]) - np.asarray(blocks[b])      # the same round's blocks
        return {"median": float(np.median(d)), "mean": float(d.mean()), "min": float(d.min()), "max": float(d.max())}
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": block, "rounds": rounds,
           "bank_entries": bank, "summary_keys": len(KEYS), "worst_episode_steps": worst_steps,
           "setups": {name(*s): stats(v) for s, v in blocks.items()},
           "ended_percent_of_plants_per_step": {name(*s): v for s, v in rates.items()},
           "worst": {name(*s): {"truncating_step_us": float(np.median([w["truncating_step_us"] for w in v[1:]])),
                                "other_steps_us": float(np.median([w["other_steps_us"] for w in v[1:]]))} for s, v in worst.items() if len(v) > 1}}
    if has_records:
        out["records_cost_us_per_step_quiet"] = paired(("quiet", "on"), ("quiet", "off"))
        out["records_cost_us_per_step_busy"] = paired(("busy", "on"), ("busy", "off"))
        out["composed_cost_us_per_step_busy"] = paired(("busy", "composed"), ("busy", "off"))
        out["records_cost_us_per_step_worst_episode"] = paired(("worst", "on"), ("worst", "off"))
        out["episode_kernel_cost_us_per_step_busy"] = paired(("busy", "off"), ("quiet", "off"))
        out["composed_rows_per_step_median"] = float(np.median(composed_rows)) if composed_rows else 0.0
        if "worst_on" in out["worst"]:
            w = out["worst"]
            out["records_cost_us_truncating_step"] = w["worst_on"]["truncating_step_us"] - w["worst_off"]["truncating_step_us"]
            out["episode_kernel_cost_us_truncating_step"] = w["worst_off"]["truncating_step_us"] - w["worst_off"]["other_steps_us"]
    env.close()
    return out


def bench_alternated(parent, repeats, steps, warmup):
    """bench.py from this tree and from the parent's, alternately: ms per step of each run"""
    runs = {"this": [], "parent": []}
    for _ in range(repeats):
        for which, root in (("this", ROOT), ("parent", parent)):
            p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                               capture_output=True, text=True, timeout=900, cwd=root)
            if p.returncode != 0:
                raise SystemExit("bench.py of the %s tree failed:\n%s" % (which, p.stderr[-2000:]))
            runs[which].append(json.loads(p.stdout.strip().splitlines()[-1])["ms_per_step"])
    return {"steps": steps, "warmup": warmup, "this_ms_per_step": runs["this"], "parent_ms_per_step": runs["parent"],
            "parent_minus_this_ms": float(np.median(runs["parent"]) - np.median(runs["this"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--block", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bank", type=int, default=64, help="entries of the start bank")
    ap.add_argument("--worst-steps", type=int, default=16, help="episode length of the worst state")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: quiet_off and bench.py across the two builds")
    ap.add_argument("--process-repeats", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--package-root", default=ROOT, help="where nuclear_sim_amd is imported from (used for the parent's build)")
    ap.add_argument("--only-off", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_records_overhead.json"))
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    sizes = {}
    for n in a.n:
        res = measure(n, a.block, a.rounds, a.bank, a.worst_steps, a.only_off)
        print("%d plants: measured" % n, file=sys.stderr, flush=True)
        if a.parent and not a.only_off:
            runs = {"this": [], "parent": []}
            for _ in range(a.process_repeats):
                for which, root in (("this", ROOT), ("parent", os.path.abspath(a.parent))):
                    cmd = [sys.executable, os.path.abspath(__file__), "--n", str(n), "--block", str(a.block), "--rounds", str(a.rounds),
                           "--bank", str(a.bank), "--package-root", root, "--only-off", "--out", ""]
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                    if p.returncode != 0:
                        raise SystemExit("the %s build's run failed:\n%s" % (which, p.stderr[-2000:]))
                    runs[which].append(json.loads(p.stdout.strip().splitlines()[-1])["sizes"][str(n)]["setups"]["quiet_off"]["median_us"])
                    print("%d plants: quiet_off of the %s build in a fresh process" % (n, which), file=sys.stderr, flush=True)
            mine = runs["this"] + [res["setups"]["quiet_off"]["median_us"]]
            spread = max(max(mine) - min(mine), res["setups"]["quiet_off"]["max_us"] - res["setups"]["quiet_off"]["min_us"])
            diff = float(np.median(runs["parent"]) - np.median(mine))
            res["parent_comparison"] = {"quiet_off": {"this_medians_us": mine, "parent_medians_us": runs["parent"], "parent_minus_this_us": diff,
                                                      "this_spread_us": float(spread), "off_agrees": bool(abs(diff) <= spread)}}
        sizes[str(n)] = res
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        head = None
    out = {"what": "per-step time of config 4 with autoreset from a bank, device noise and a two-key work-order summary, episode records off and on: "
                   "nothing ending, about 1 % of the plants truncating per step (one lane of a wave at the most), the one step on which every plant "
                   "truncates at once, and the composed host path at 1 %",
           "sizes": sizes, "head": head}
    if a.parent and not a.only_off:
        out["bench"] = bench_alternated(os.path.abspath(a.parent), a.process_repeats, a.bench_steps, 20)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
