"""What a sample of the state log costs behind a step, for the log of every plant and for a log with a watch list.

    python tools/watched_log_overhead.py [--sizes 32768 65536] [--rounds 5] [--block 100]

Config 4 plants (BatchedPlantEnv.action_test("oil_top_off", seeds), automatic maintenance on, diagnostics on: the diagnostics build of the
step kernel, which a log of the reference layout with diagnostics needs), a StateLog of the reference layout with diagnostics=True.  One
worker process per batch size; in it, on ONE env, these cases:
  a                step() alone
  b                step() + record() of the log of every plant.  Its ring holds TWO samples and is overwritten (clear() when full): the
                   default ring of 256 samples does not fit the device at these sizes
  c_64_scattered, c_1024_scattered, c_1024_consecutive, c_n16_scattered, c_n4_scattered, c_all
                   step() + record() of a log with that watch list (n16 = n / 16 plants, n4 = n / 4, all = every plant); scattered =
                   drawn without replacement by numpy's default_rng(0) and sorted, consecutive = one run in the middle of the batch.
                   Rings of two samples, as b
After a warm-up of every case, `--rounds` rounds; in each round every case is timed once, in an order that rotates with the round:
  per launch       one block of `--block` iterations between two device events, ending in a synchronise: wall time per iteration, what a
                   caller pays (the host's share included: a full record() is several dozen launches)
  following step   `--block` more iterations with an event before and after each step(): the device time of the step that FOLLOWS a
                   sample, which is what the sample did to the caches (median of the block; the events bracket the step's own launches, so
                   where the host is the bottleneck they hold its gaps too -- case a, measured the same way, is the yardstick)
Reported per case: median, quartiles, min and max over the rounds.  The yardsticks are this run's own a and b.

The one condition that follows from the bytes (1 024 scattered plants of 65 536 move at most one cache line per element, an eighth of the
full sample's traffic, into a 64th of its ring): c_1024_scattered - a < (b - a) / 2 at 65 536 plants.  Exit status 1 if it does not hold.
Everything else is reported, not gated; c_n16_scattered, c_n4_scattered and c_all against b say where the break-even lies.  One JSON line, written to --out.
"""
import argparse
import json
import os
import sys

from overhead_harness import fresh_process, head, stats, time_steps, write_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING = 2


def watch_lists(n):
    import numpy as np
    rng = np.random.default_rng(0)
    scattered = lambda k: sorted(int(p) for p in rng.choice(n, size=k, replace=False))
    return {"c_64_scattered": scattered(64), "c_1024_scattered": scattered(1024),
            "c_1024_consecutive": list(range(n // 2, n // 2 + 1024)), "c_n16_scattered": scattered(n // 16),
            "c_n4_scattered": scattered(n // 4), "c_all": list(range(n))}


def worker(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    from nuclear_sim_amd.statelog import StateLog
    n = a.worker
    env = BatchedPlantEnv.action_test("oil_top_off", seeds=range(n), diagnostics=True)
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    setpoint = torch.full((n,), 95.0, dtype=torch.float64, device=dev)
    # the heat source's noise as a column the caller holds, as bench.py passes it: the env's own host generator draws 256 steps at a time,
    # a pause of tens of milliseconds that would land in whichever block is being timed
    noise = torch.randn(n, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    logs = {"a": None, "b": StateLog(env, capacity=RING, diagnostics=True)}
    lists = watch_lists(n)
    for name, ids in lists.items():
        logs[name] = StateLog(env, capacity=RING, diagnostics=True, plants=ids)
    rows = {"a": 0, "b": len(logs["b"].columns) + len(logs["b"]._res_keys) + 170 + 1}      # members, result keys, diagnostics rows, done
    rows.update({name: int(logs[name]._buf.shape[1]) for name in lists})

    def iteration(log, k):
        env.step(power_setpoint=setpoint, noise_z=noise)
        if log is not None:
            if len(log) == RING:
                log.clear()
            log.record(k, k * env.dt)

    def per_launch(log, iters):
        k = iter(range(iters))
        return time_steps(stream, lambda: iteration(log, next(k)), iters)

    def following_step(log, iters):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        iteration(log, 0)
        for k in range(iters):
            ev[k][0].record(stream)
            env.step(power_setpoint=setpoint, noise_z=noise)
            ev[k][1].record(stream)
            if log is not None:
                if len(log) == RING:
                    log.clear()
                log.record(k, k * env.dt)
        torch.cuda.synchronize(dev)
        return float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]))

    for _ in range(200):
        env.step(power_setpoint=setpoint, noise_z=noise)
    names = list(logs)
    for name in names:
        per_launch(logs[name], 20)
    launch = {name: [] for name in names}
    follow = {name: [] for name in names}
    for r in range(a.rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            launch[name].append(per_launch(logs[name], a.block))
            follow[name].append(following_step(logs[name], a.block))
    info = {"per_launch_us": launch, "following_step_us": follow, "rows_per_sample": rows,
            "n_watched": {name: len(ids) for name, ids in lists.items()},
            "step_kernel": env.last_step_kernel(), "device": torch.cuda.get_device_name(dev)}
    for log in logs.values():
        if log is not None:
            log.close()
    env.close()
    print(json.dumps(info))      # the worker's last line: what fresh_process reads


def over_rounds(v):
    """the harness's stats, its count named for what a value is here: one per round"""
    s = stats(v)
    s["rounds"] = s.pop("blocks")
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[32768, 65536])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--worker-timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "watched_log_overhead.json"))
    ap.add_argument("--worker", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    sizes = {}
    meta = {}
    for n in a.sizes:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(n), "--rounds", str(a.rounds), "--block", str(a.block)]
        w = fresh_process(cmd, a.worker_timeout)
        meta = {"step_kernel": w["step_kernel"], "device": w["device"]}
        cases = {}
        for name in w["per_launch_us"]:
            cases[name] = {"per_launch": over_rounds(w["per_launch_us"][name]), "following_step": over_rounds(w["following_step_us"][name]),
                           "rows_per_sample": w["rows_per_sample"][name], "n_watched": w["n_watched"].get(name)}
        med = lambda name: cases[name]["per_launch"]["median_us"]
        full_cost = med("b") - med("a")
        for name in cases:
            if name != "a":
                cases[name]["sample_cost_us"] = med(name) - med("a")
                cases[name]["sample_cost_of_full"] = (med(name) - med("a")) / full_cost
            cases[name]["following_step_vs_a"] = cases[name]["following_step"]["median_us"] / cases["a"]["following_step"]["median_us"]
        sizes[str(n)] = cases
        sys.stderr.write("%d plants: a %.1f us, b %.1f us per launch\n" % (n, med("a"), med("b"))); sys.stderr.flush()
    res = {"what": "per-launch time of step() alone (a; setpoint and heat-source noise as columns the caller holds), with a record() of the log of every plant behind it (b, ring of %d samples, overwritten) and "
                   "with a record() of a log with a watch list (c_*), config 4 plants with diagnostics, reference layout with diagnostics; and the "
                   "device time of the step that follows the sample" % RING,
           "ring_samples": RING, "block_iterations": a.block, "rounds": a.rounds, "sizes": sizes}
    res.update(meta)
    if "65536" in sizes:
        c = sizes["65536"]
        res["gate_1024_scattered_under_half_of_full_at_65536"] = bool(c["c_1024_scattered"]["sample_cost_us"] < 0.5 * c["b"]["sample_cost_us"])
    res["head"] = head(ROOT)
    write_line(res, a.out)
    return 0 if res.get("gate_1024_scattered_under_half_of_full_at_65536", True) else 1


if __name__ == "__main__":
    sys.exit(main() or 0)
