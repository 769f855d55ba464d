"""What the maintenance event log (npb_set_maintenance_log) costs on BASELINE config 4 at 65 536 plants.

action_test("oil_top_off", range(n), dt = 5), one handle throughout.  The batch is snapshotted once, and every timed block of every setup
replays the SAME simulated interval: restore(), the same pre-drawn heat-source noise rows, 8 untimed steps (switching the log
re-uploads the rule's constants and has the rule look at every wave once), then `--block` steps, each bracketed by its own pair of
events.  The setups, in an order that rotates from round to round:
  off          the log off
  on_drain48   the log on, drained every 48 steps (cursor read, copy of the records, cursor zeroed: env.maintenance_log_records)
  composed     the log off; what a caller without it writes: gather the two counters after every step (npb_get_field on the
               device), diff them against the step before in torch, nonzero, host sync
Reported per setup: the per-step time of each block (mean and median over the blocks, quartiles, min, max), the per-step
distribution inside the blocks (median and max step, the steps whose maintenance rule ran on many waves), and the host time of
the drains.  One JSON line, also written to --out.  The kernels' own times: run this under
`rocprofv3 --kernel-trace --stats -- python tools/maintenance_log_overhead.py --rounds 2`.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

from overhead_harness import head, stats, time_steps, write_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nuclear_sim_amd import _lib  # noqa: E402
from nuclear_sim_amd.env import BatchedPlantEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--block", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maintenance_log_overhead.json"))
    a = ap.parse_args()
    n, B, W = a.n, a.block, 8
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), noise_generator="device")
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    sp = torch.full((n,), 95.0, dtype=torch.float64, device=dev)
    gen = torch.Generator(device=dev); gen.manual_seed(42)
    z = torch.randn((W + B, n), device=dev, dtype=torch.float64, generator=gen)    # the same noise rows in every block
    env.snapshot()
    prev = {}
    drain_ms = []
    events = {"on_drain48": 0, "composed": 0}

    def step(t):
        return env.step(power_setpoint=sp, noise_z=z[t])

    def step_log(t, k):
        step(t)
        if (k + 1) % 48 == 0:
            t0 = time.perf_counter()
            events["on_drain48"] += len(env.maintenance_log_records())
            drain_ms.append(1e3 * (time.perf_counter() - t0))

    def step_composed(t, k):
        step(t)
        c = env.get_field("maint.work_orders_created"); p = env.get_field("maint.maintenance_actions_performed")
        idx = torch.nonzero((c != prev["c"]) | (p != prev["p"])).flatten()
        events["composed"] += int(idx.numel())          # the host sync
        prev["c"], prev["p"] = c, p

    steps = {"off": lambda t, k: step(t), "on_drain48": step_log, "composed": step_composed}

    def run_block(name):
        env.restore()
        if name == "on_drain48":
            env.enable_maintenance_log(1 << 20)
        else:
            env.enable_maintenance_log(None)
        for t in range(W):
            step(t)
        prev["c"] = env.get_field("maint.work_orders_created"); prev["p"] = env.get_field("maint.maintenance_actions_performed")
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(B)]
        f = steps[name]
        ks = iter(range(B))

        def bracketed():      # the step between its own pair of events, inside the block's
            k = next(ks)
            ev[k][0].record(stream)
            f(W + k, k)
            ev[k][1].record(stream)
        us = time_steps(stream, bracketed, B)
        per_step = [x.elapsed_time(y) * 1e3 for x, y in ev]        # us: the step launch (and, composed, its gathers) per step
        return us, per_step

    setups = list(steps)
    # (not the harness's rotated_blocks: the event counts and the drain times are zeroed between the warm-up and the rounds)
    for name in setups:              # warm-up
        run_block(name)
    events["on_drain48"] = events["composed"] = 0
    drain_ms.clear()
    blocks = {s: [] for s in setups}
    per_step = {s: [] for s in setups}
    for r in range(a.rounds):
        order = setups[r % 3:] + setups[:r % 3]
        for name in order:
            bt, ps = run_block(name)
            blocks[name].append(bt); per_step[name].append(ps)

    S = {s: dict(stats(v), mean_us=float(np.mean(v))) for s, v in blocks.items()}
    for s in setups:
        ps = np.asarray(per_step[s])                 # [rounds, B]
        med = np.median(ps, axis=0)                  # per step index, over the rounds: the same simulated step every time
        S[s]["step_median_us"] = float(np.median(ps))
        S[s]["step_max_us"] = float(ps.max())
        S[s]["slow_steps"] = [[int(k), float(med[k])] for k in np.nonzero(med > 3 * np.median(med))[0]]
    off = S["off"]
    res = {"what": "per-step time of config 4 with the maintenance event log off, on (drained every 48 steps) and composed from the "
                   "counters; every block replays the same simulated interval",
           "n_plants": n, "device": torch.cuda.get_device_name(dev), "storage": env.storage, "step_kernel": env.last_step_kernel(),
           "block_steps": B, "rounds": a.rounds, "events_logged_per_block": events["on_drain48"] // a.rounds,
           "plants_with_events_per_block_composed": events["composed"] // a.rounds,
           "drain_ms": {"median": float(np.median(drain_ms)), "max": float(np.max(drain_ms)), "count": len(drain_ms)},
           "setups": S,
           "overhead_vs_off_pct": {s: {"mean": 100.0 * (S[s]["mean_us"] / off["mean_us"] - 1.0),
                                       "median": 100.0 * (S[s]["median_us"] / off["median_us"] - 1.0)} for s in setups if s != "off"},
           "head": head(ROOT)}
    write_line(res, a.out)


if __name__ == "__main__":
    main()
