"""What the automatic maintenance of steam generators and condenser (npb_set_component_maintenance) costs per step on BASELINE config 4.

action_test("oil_top_off", range(n), dt = 5) at 32 768 and 65 536 plants, ONE handle per size throughout; the feature is switched on and off on
that handle through the C ABI.  After the usual preconditioning (untimed steps until the clocks have settled) every timed block replays
the SAME simulated interval: restore(), the same pre-drawn heat-source noise rows, `--warm` untimed steps, then `--block` steps, each
bracketed by its own pair of events.  The cases, in an order that rotates from round to round:
  pumps_in_step    the feature off: maintenance=True as before, the pump rule inside the step kernels (npb_step*_maint_kernel)
  on_quiet         the feature on, nothing crossing: the plain step kernel + npb_maint_all_kernel, whose every wave screens and leaves
  on_due_1pct      the feature on, 1 % of the plants (every 100th: spread over the waves) with three fouled generators and a fouled
                   condenser poked in before the untimed steps, which create their orders: during the timed block each of them holds
                   due orders and has one carried out at every check
Reported per size and case: the per-launch median (and mean, quartiles) of a step() in microseconds, and the two on-cases relative to
pumps_in_step.  One JSON line, also written to --out.  The kernels' own times: run this under
`rocprofv3 --kernel-trace --stats -- python tools/auto_component_overhead.py --rounds 2`.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

from overhead_harness import write_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nuclear_sim_amd import _lib  # noqa: E402
from nuclear_sim_amd.env import BatchedPlantEnv  # noqa: E402

CASES = ("pumps_in_step", "on_quiet", "on_due_1pct")


def measure(n, a):
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), noise_generator="device", component_maintenance=True)
    L, dev = env.L, env.device
    table = _lib.NpbComponentMaintTable()
    L.npb_default_component_maintenance_table(ctypes.byref(table))
    sp = torch.full((n,), 95.0, dtype=torch.float64, device=dev)
    gen = torch.Generator(device=dev); gen.manual_seed(42)
    z = torch.randn((a.warm + a.block, n), device=dev, dtype=torch.float64, generator=gen)
    env.snapshot()
    some = (torch.arange(n, device=dev) % 100 == 0)
    thick = 23.0 * (1.0 - (1.0 - 0.36) ** 0.5) / 2.0      # 36 % of a support plate's hole blocked (tools/make_auto_component_golden.py)
    created = {}

    def poke():
        for i in range(3):
            for k in range(7):
                col = env.get_field("sg.tsp_magnetite", instance=i, k=k)
                env.set_field("sg.tsp_magnetite", torch.where(some, torch.full_like(col, thick), col), instance=i, k=k)
        for name, v in (("cond.biofouling_thickness", 3.0), ("cond.scale_thickness", 2.0), ("cond.corrosion_product_thickness", 1.2)):
            col = env.get_field(name)
            env.set_field(name, torch.where(some, torch.full_like(col, v), col))

    def block(case):
        _lib.check(L.npb_set_component_maintenance(env._h, None if case == "pumps_in_step" else ctypes.byref(table)), env._h)
        env.restore()
        if case == "on_due_1pct":
            poke()
        for t in range(a.warm):
            env.step(power_setpoint=sp, noise_z=z[t])
        # (not the harness's time_steps: every launch has its own pair of events, and the block one synchronise at its end)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.block)]
        for k in range(a.block):
            ev[k][0].record()
            env.step(power_setpoint=sp, noise_z=z[a.warm + k])
            ev[k][1].record()
        torch.cuda.synchronize(dev)
        created[case] = int(env.get_field("maint.work_orders_created").sum().item())
        performed = int(env.get_field("maint.maintenance_actions_performed").sum().item())
        return [1e3 * s.elapsed_time(e) for s, e in ev], performed

    for _ in range(a.precondition):      # the clocks: the step kernel needs a couple of hundred launches to reach its steady time
        env.step(power_setpoint=sp, noise_z=z[0])
    torch.cuda.synchronize(dev)
    samples = {c: [] for c in CASES}
    performed = {}
    for r in range(a.rounds):
        for j in range(len(CASES)):
            c = CASES[(j + r) % len(CASES)]
            us, performed[c] = block(c)
            samples[c] += us
    out = {}
    for c in CASES:
        s = np.array(samples[c])
        out[c] = {"median_us": float(np.median(s)), "mean_us": float(s.mean()), "p25_us": float(np.percentile(s, 25)), "p75_us": float(np.percentile(s, 75)),
                  "launches": int(s.size), "work_orders_created_in_batch": created[c], "actions_performed_in_batch": performed[c],
                  "last_step_kernel": None}
    base = out["pumps_in_step"]["median_us"]
    for c in CASES[1:]:
        out[c]["median_over_pumps_in_step"] = out[c]["median_us"] / base
        out[c]["median_minus_pumps_in_step_us"] = out[c]["median_us"] - base
    out["on_quiet"]["last_step_kernel"] = out["on_due_1pct"]["last_step_kernel"] = env.last_step_kernel()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[32768, 65536])
    ap.add_argument("--block", type=int, default=12)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--precondition", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auto_component_overhead.json"))
    a = ap.parse_args()
    res = {"workload": "action_test('oil_top_off', range(n), dt=5), fp64 storage", "block": a.block, "warm": a.warm, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "sizes": {str(n): measure(n, a) for n in a.sizes}}
    write_line(res, a.out)


if __name__ == "__main__":
    main()
