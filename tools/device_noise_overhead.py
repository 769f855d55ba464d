"""What generating the heat-source noise on the device costs (npb_noise_fill, BatchedPlantEnv(noise_generator="device")) at
65 536 plants seeded 42 + i (BASELINE config 3) with blocks of 256 rows.

  fill        the fill kernel's time per [256, n] block, from device events around npb_noise_fill (median of --fills after warm-up)
  device      env.step() with noise_generator="device": a fill every 256 steps, on the step's stream
  predrawn    the same env and loop fed a pre-drawn [256, n] block as noise_z (what bench.py does: no generator in the loop)
  host        the host generator (HeatSourceNoise) at the same seeds: its construction and its draw per block (host work only)

One handle throughout -- where an arena lands in physical memory moves the step time from one handle to the next (npb_api.hip,
probe_placement).  After --warmup steps of each loop, --rounds rounds of --steps steps alternate between `device` and
`predrawn`, each timed by a host clock around work that ends in a device synchronise.  Both loops take the same load-following
setpoints.  Prints one JSON line (per-step times in us) and writes it to --out.  The kernels' own times: run this under
`rocprofv3 --kernel-trace --stats -- python tools/device_noise_overhead.py --rounds 1 --no-host`.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

from overhead_harness import time_steps, write_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nuclear_sim_amd import _lib  # noqa: E402
from nuclear_sim_amd.env import BatchedPlantEnv, HeatSourceNoise  # noqa: E402


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": float(np.median(xs)), "q1": float(np.percentile(xs, 25)), "q3": float(np.percentile(xs, 75)),
            "min": float(xs.min()), "max": float(xs.max()), "all": [round(float(x), 3) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2048, help="steps per timed round (a multiple of --block keeps the fills per round equal)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=512)
    ap.add_argument("--fills", type=int, default=30)
    ap.add_argument("--no-host", action="store_true", help="skip the host generator's timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_noise_overhead.json"))
    a = ap.parse_args()
    n, B = a.n, a.block
    seeds = 42 + np.arange(n, dtype=np.int64)
    if not torch.cuda.is_available():
        raise SystemExit("device_noise_overhead.py measures the GPU: no HIP device")
    env = BatchedPlantEnv(n, dt=1.0, heat_source="constant", noise_enabled=True, noise_std_percent=0.1, noise_seeds=seeds,
                          noise_generator="device")
    dev = env.device
    L, h = env.L, env._h
    stream = torch.cuda.current_stream(dev)
    gid = torch.arange(n, device=dev, dtype=torch.float64)
    tt = torch.arange(B, device=dev, dtype=torch.float64)[:, None]
    setpoints = (90.0 + 10.0 * torch.sin(2.0 * np.pi * tt / (600.0 + 60.0 * (gid % 16))[None, :])).contiguous()

    # the fill kernel alone, on a generator of its own handle (the env's stream is left where it is)
    gen_env = BatchedPlantEnv(n, noise_enabled=True)
    _lib.check(L.npb_noise_seed(gen_env._h, seeds.ctypes.data_as(ctypes.c_void_p), gen_env._stream()), gen_env._h)
    blk = torch.empty((B, n), dtype=torch.float64, device=dev)
    predrawn = torch.empty((B, n), dtype=torch.float64, device=dev)
    _lib.check(L.npb_noise_fill(gen_env._h, B, ctypes.c_void_p(predrawn.data_ptr()), gen_env._stream()), gen_env._h)
    def one_fill():
        _lib.check(L.npb_noise_fill(gen_env._h, B, ctypes.c_void_p(blk.data_ptr()), gen_env._stream()), gen_env._h)
    fill_us = [time_steps(stream, one_fill, 1) for _ in range(a.fills + 3)][3:]
    gen_env.close()

    t_dev = [0]
    t_pre = [0]

    def run(kind, steps):
        for _ in range(steps):
            if kind == "device":
                env.step(power_setpoint=setpoints[t_dev[0] % B])
                t_dev[0] += 1
            else:
                env.step(power_setpoint=setpoints[t_pre[0] % B], noise_z=predrawn[t_pre[0] % B])
                t_pre[0] += 1

    run("device", a.warmup)
    run("predrawn", a.warmup)
    torch.cuda.synchronize(dev)
    per_step = {"device": [], "predrawn": []}
    for r in range(a.rounds):
        for kind in (("device", "predrawn") if r % 2 == 0 else ("predrawn", "device")):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            run(kind, a.steps)
            torch.cuda.synchronize(dev)
            per_step[kind].append((time.perf_counter() - t0) / a.steps * 1e6)
    kernel = env.last_step_kernel()
    env.close()

    fill = stats(fill_us)
    dev_s, pre_s = stats(per_step["device"]), stats(per_step["predrawn"])
    out = {"plants": n, "block": B, "seeds": "42 + i", "step_kernel": kernel,
           "fill_us_per_block": fill, "fill_us_per_step_amortised": fill["median"] / B,
           "step_us_device_noise": dev_s, "step_us_predrawn_noise": pre_s,
           "steps_per_round": a.steps, "rounds": a.rounds,
           "fill_share_of_step": fill["median"] / B / pre_s["median"],
           "device_vs_predrawn_step_time": dev_s["median"] / pre_s["median"] - 1.0}
    if not a.no_host:
        t0 = time.perf_counter()
        hn = HeatSourceNoise(seeds, block=B)             # host arrays only: no device involved
        out["host_construct_s"] = time.perf_counter() - t0
        draws = []
        for _ in range(2):
            t0 = time.perf_counter()
            hn.next()                                   # the first row of a block draws the whole block
            draws.append(time.perf_counter() - t0)
            for _ in range(B - 1):
                hn.next()
        out["host_draw_ms_per_block"] = stats([x * 1e3 for x in draws])
        out["host_draw_us_per_step"] = out["host_draw_ms_per_block"]["median"] * 1e3 / B
    write_line(out, a.out)


if __name__ == "__main__":
    main()
