"""What drawing the data-gen runner's power profile on the device costs (npb_profile_fill, BatchedPlantEnv(power_profile=...)), at
65 536 and 32 768 plants seeded 42 + i with blocks of 256 rows and profiles of --horizon steps, in one process.

  profile_fill  npb_profile_fill's time per [256, n] block (the generator's fill kernel plus the filter kernel), from device events
  noise_fill    npb_noise_fill's time per [256, n] block on the same seeds, for scale: the profile's draws come from the same kernel
  profile       env.step() with the profile attached: a fill every 256 steps, on the step's stream
  prebuilt      the same env and loop fed a pre-built [256, n] block of setpoints as power_setpoint (no profile work in the loop)

Both loops run with the heat-source noise generated on the device.  One handle per size throughout -- where an arena lands in
physical memory moves the step time from one handle to the next.  After --warmup steps of each loop, --rounds rounds of --steps steps
alternate between `profile` and `prebuilt`, each timed by a host clock around work that ends in a device synchronise.  Prints one JSON
line (per-step times in us) and writes it to --out.
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
from nuclear_sim_amd.env import BatchedPlantEnv, PowerProfile  # noqa: E402


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": float(np.median(xs)), "q1": float(np.percentile(xs, 25)), "q3": float(np.percentile(xs, 75)),
            "min": float(xs.min()), "max": float(xs.max()), "all": [round(float(x), 3) for x in xs]}


def timed(stream, fills, call):
    return stats([time_steps(stream, call, 1) for _ in range(fills + 3)][3:])


def measure(n, a):
    B = a.block
    seeds = 42 + np.arange(n, dtype=np.int64)
    env = BatchedPlantEnv(n, dt=1.0, heat_source="constant", noise_enabled=True, noise_std_percent=0.1, noise_seeds=seeds,
                          noise_generator="device", power_profile=dict(seeds=seeds, steps=a.horizon, block=B))
    dev = env.device
    stream = torch.cuda.current_stream(dev)

    # the two fills alone, on a handle of their own (the env's streams are left where they are)
    gen = BatchedPlantEnv(n, noise_enabled=True)
    L = gen.L
    rows = PowerProfile(gen, seeds, a.horizon, block=B)
    prebuilt = rows.fill(B)[0]
    blk = torch.empty((2, B, n), dtype=torch.float64, device=dev)
    profile_fill = timed(stream, a.fills, lambda: _lib.check(L.npb_profile_fill(gen._h, B, ctypes.c_void_p(blk[0].data_ptr()),
                                                                                 ctypes.c_void_p(blk[1].data_ptr()), None, gen._stream()), gen._h))
    _lib.check(L.npb_noise_seed(gen._h, seeds.ctypes.data_as(ctypes.c_void_p), gen._stream()), gen._h)
    noise_fill = timed(stream, a.fills, lambda: _lib.check(L.npb_noise_fill(gen._h, B, ctypes.c_void_p(blk[0].data_ptr()), gen._stream()), gen._h))
    gen.close()

    t_pre = [0]

    def run(kind, steps):
        for _ in range(steps):
            if kind == "profile":
                env.step()
            else:
                env.step(power_setpoint=prebuilt[t_pre[0] % B])
                t_pre[0] += 1

    run("profile", a.warmup)
    run("prebuilt", a.warmup)
    torch.cuda.synchronize(dev)
    per_step = {"profile": [], "prebuilt": []}
    for r in range(a.rounds):
        for kind in (("profile", "prebuilt") if r % 2 == 0 else ("prebuilt", "profile")):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            run(kind, a.steps)
            torch.cuda.synchronize(dev)
            per_step[kind].append((time.perf_counter() - t0) / a.steps * 1e6)
    kernel = env.last_step_kernel()
    env.close()
    pro, pre = stats(per_step["profile"]), stats(per_step["prebuilt"])
    return {"plants": n, "step_kernel": kernel,
            "profile_fill_us_per_block": profile_fill, "noise_fill_us_per_block": noise_fill,
            "profile_fill_us_per_step_amortised": profile_fill["median"] / B,
            "profile_fill_vs_noise_fill": profile_fill["median"] / noise_fill["median"],
            "step_us_profile": pro, "step_us_prebuilt_setpoints": pre,
            "profile_fill_share_of_step": profile_fill["median"] / B / pre["median"],
            "profile_vs_prebuilt_step_time": pro["median"] / pre["median"] - 1.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=600, help="steps of one profile (the runner's num_steps)")
    ap.add_argument("--steps", type=int, default=1024, help="steps per timed round (a multiple of --block keeps the fills per round equal)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=256)
    ap.add_argument("--fills", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "power_profile_overhead.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("power_profile_overhead.py measures the GPU: no HIP device")
    out = {"block": a.block, "horizon": a.horizon, "seeds": "42 + i", "steps_per_round": a.steps, "rounds": a.rounds,
           "sizes": [measure(n, a) for n in a.n]}
    write_line(out, a.out)


if __name__ == "__main__":
    main()
