"""What a call of perform_turbine_maintenance (npb_perform_turbine_maintenance) behind every step costs, at 65 536 and 32 768 plants.

The method of tools/turbine_maintenance_overhead.py: BASELINE config 3's plant and inputs (dt = 1 s, constant heat source with 0.1 %
noise, the per-plant load-following setpoint trace of bench.py), one handle per batch size throughout.  The batch is snapshotted once
and every timed block replays the same simulated interval: restore(), 8 untimed iterations, then `--block` iterations between one pair
of events.  The setups, in an order that rotates from round to round:
  step            step() alone: the yardstick (the step kernels are the parent commit's, byte for byte)
  none            step(); perform_turbine_maintenance(...) with no plant ordered (action -1 everywhere)
  component_none  step(); perform_component_maintenance(...) with no plant ordered: the sibling's empty call, measured in the same run
  one_pct         ... with 1 % of the plants ordered (fixed seed), the mix of `all_mixed`
  all_one         ... with every plant ordering the lubrication system's turbine_oil_change: every wave sweeps turb, all lanes together
  all_mixed       ... with every plant ordered, kinds mixed within a wave: a quarter each the turbine's routine maintenance, the replacement
                  of a random bearing, the lubrication system's oil change (turb, 35 columns) and the overhaul of a random stage (3 columns)
The order columns are device tensors built once, so a call is the launch alone.  Reported per batch size and setup: ms per iteration
of each block (mean, median, quartiles, min, max) and the difference to `step` in microseconds.  One JSON line, also written to --out.
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np
import torch

from overhead_harness import head, rotated_blocks, time_steps, write_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nuclear_sim_amd import _lib  # noqa: E402
from nuclear_sim_amd.env import BatchedPlantEnv  # noqa: E402

SETUPS = ("step", "none", "component_none", "one_pct", "all_one", "all_mixed")
KERNEL = "npb_operator_turbine_maint_kernel"


def measure(n, B, rounds, only):
    W, total = 8, 256
    env = BatchedPlantEnv(n, dt=1.0, heat_source="constant", noise_enabled=True, noise_std_percent=0.1)
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    gid = torch.arange(n, device=dev, dtype=torch.float64)
    period = 600.0 + 60.0 * (gid % 16)
    tt = torch.arange(total, device=dev, dtype=torch.float64)[:, None]
    target = 90.0 + 10.0 * torch.sin(2.0 * np.pi * tt / period[None, :])
    sp = torch.empty_like(target)
    sp[0] = target[0]
    for t in range(1, total):      # rate-limited to 0.02 % per step, as bench.py's
        d = target[t] - sp[t - 1]
        sp[t] = torch.where(d.abs() > 0.02, sp[t - 1] + 0.02 * torch.sign(d), target[t])
    gen = torch.Generator(device=dev); gen.manual_seed(42)
    z = torch.randn((total, n), device=dev, dtype=torch.float64, generator=gen)
    rng = np.random.default_rng(149)
    T = _lib.turbine_action_index
    kinds = rng.integers(0, 4, n)
    mix = np.choose(kinds, [T("turbine", "routine_maintenance"), T("bearing", "turbine_bearing_replacement"), T("lubrication", "turbine_oil_change"),
                            T("stage", "overhaul")]).astype(np.int32)
    units = torch.as_tensor(np.where(kinds == 3, rng.integers(0, 14, n), rng.integers(0, 4, n)).astype(np.int32), device=dev)
    one = np.full(n, -1, dtype=np.int32)
    chosen = rng.choice(n, n // 100, replace=False)
    one[chosen] = mix[chosen]
    orders = {"none": torch.full((n,), -1, dtype=torch.int32, device=dev), "component_none": torch.full((n,), -1, dtype=torch.int32, device=dev),
              "one_pct": torch.as_tensor(one, device=dev), "all_one": torch.full((n,), T("lubrication", "turbine_oil_change"), dtype=torch.int32, device=dev),
              "all_mixed": torch.as_tensor(mix, device=dev)}
    env.snapshot()

    def iteration(name, t):
        env.step(power_setpoint=sp[t % total], noise_z=z[t % total])
        if name == "component_none":
            env.perform_component_maintenance("condenser", orders[name], unit=units)
        elif name != "step":
            env.perform_turbine_maintenance("turbine", orders[name], unit=units)

    def run_block(name):
        env.restore()
        for t in range(W):
            iteration(name, t)
        t = iter(range(W, W + B))
        return time_steps(stream, lambda: iteration(name, next(t)), B) / 1e3        # ms per iteration

    setups = [s for s in SETUPS if only in (None, s)]
    for q in range(2):                      # clocks: with the rotation's own warm-up block, ~100 ms of the same launches before anything is timed
        for name in setups:
            run_block(name)
    blocks = rotated_blocks(setups, rounds, run_block)
    ordered = {name: int((orders[name] >= 0).sum().item()) for name in orders if only in (None, name)}
    kernel = env.last_step_kernel()
    env.close()

    def stats(v):
        v = np.asarray(v)
        return {"mean_ms": float(v.mean()), "median_ms": float(np.median(v)), "p25_ms": float(np.percentile(v, 25)),
                "p75_ms": float(np.percentile(v, 75)), "min_ms": float(v.min()), "max_ms": float(v.max()), "blocks": int(v.size)}
    S = {s: stats(v) for s, v in blocks.items()}
    out = {"n_plants": n, "step_kernel": kernel, "plants_ordered": ordered, "setups": S}
    if "step" in S:
        out["overhead_us_vs_step"] = {s: {"median": 1e3 * (S[s]["median_ms"] - S["step"]["median_ms"]), "mean": 1e3 * (S[s]["mean_ms"] - S["step"]["mean_ms"]),
                                          "min": 1e3 * (S[s]["min_ms"] - S["step"]["min_ms"])} for s in setups if s != "step"}
    return out


def collect_traces(directory):
    """{"<n>": {"<setup>": {"average_us", "calls"}}} from the rocprofv3 kernel statistics under directory/<n>_<setup>/"""
    out = {}
    for d in sorted(glob.glob(os.path.join(directory, "*_*"))):
        n, _, setup = os.path.basename(d).partition("_")
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if KERNEL in (row.get("Name") or ""):
                    avg = float(row.get("AverageNs") or row.get("Average") or "nan")
                    out.setdefault(n, {})[setup] = {"average_us": avg / 1e3, "calls": int(float(row.get("Calls") or 0))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[65536, 32768])
    ap.add_argument("--block", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--only", choices=SETUPS, default=None)
    ap.add_argument("--collect-traces", metavar="DIR", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "turbine_maintenance_overhead.json"))
    a = ap.parse_args()
    if a.collect_traces:
        res = json.load(open(a.out))
        res["kernel_trace"] = {"kernel": KERNEL, "what": "rocprofv3 --kernel-trace --stats, one run per batch size and setup: average duration of the kernel",
                               "by_plants": collect_traces(a.collect_traces)}
    else:
        res = {"what": "ms per iteration of step() alone and of step(); perform_turbine_maintenance(...) with no plant, 1 % of the plants and every plant "
                       "ordered (one type: the lubrication system's turbine_oil_change; mixed: a quarter each turbine routine_maintenance, bearing "
                       "replacement, lubrication oil change, stage overhaul), and of step(); perform_component_maintenance(...) with no plant ordered; "
                       "BASELINE config 3 plant and inputs; every block replays the same simulated interval",
               "device": torch.cuda.get_device_name(0), "block_iterations": a.block, "rounds": a.rounds,
               # a sweep of what an order touches: turb (35 eight-byte columns) read and written, or a stage's three columns
               "expected_bytes_per_plant_turb_order": 35 * 8 * 2, "expected_bytes_per_plant_stage_order": 3 * 8 * 2,
               "by_plants": {str(n): measure(n, a.block, a.rounds, a.only) for n in a.n}, "head": head(ROOT)}
    write_line(res, a.out)


if __name__ == "__main__":
    main()
