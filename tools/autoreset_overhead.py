"""What same-step autoreset (npb_set_autoreset: the episode kernel behind every npb_step) costs at 65 536 plants.

One handle throughout -- where an arena lands in physical memory moves the step time from one handle to the next (npb_api.hip,
probe_placement), so comparing two handles would measure placement.  After >= 200 warm-up launches, blocks of `--block`
event-timed steps alternate between the setups:
  off            autoreset off
  on_idle        autoreset on, no plant terminates or reaches a limit
  on_1pct        autoreset on, max_episode_steps = 100 with the counters staggered (early restore(mask_k)): ~1 % reset per step
  composed_1pct  autoreset off, the same bookkeeping composed in Python: torch counters, done | len >= max, restore(mask),
                 get_observation, torch.where -- what a caller without the feature writes
  on_all         autoreset on, max_episode_steps = 1: every plant resets on every step (a full arena copy per step; not a target)
Prints one JSON line (per-step time in us: median, quartiles, min, max over the blocks) and writes it to --out.
The episode kernel's own time: run this under `rocprofv3 --kernel-trace --stats -- python tools/autoreset_overhead.py --rounds 2`.
"""
import argparse
import os
import sys

import numpy as np
import torch

from overhead_harness import head, stats, time_steps, write_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nuclear_sim_amd import _lib  # noqa: E402
from nuclear_sim_amd.env import BatchedPlantEnv  # noqa: E402

MAX = 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--block", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autoreset_overhead.json"))
    a = ap.parse_args()
    n = a.n
    env = BatchedPlantEnv(n, autoreset=True)
    L, h = env.L, env._h
    dev = env.device
    lane = torch.arange(n, device=dev)
    stream = torch.cuda.current_stream(dev)

    def set_autoreset(on, max_steps=0):
        _lib.check(L.npb_set_autoreset(h, int(on), int(max_steps)), h)

    def stagger():
        """autoreset on with limit MAX and plant p's counter at (k - p) mod MAX: ~1 % of the plants reach the limit on each step"""
        set_autoreset(True, MAX)
        for k in range(MAX):
            env.step()
            env.restore(lane % MAX == k)

    # the composed path's own counters (staggered the same way)
    c_len = torch.zeros(n, dtype=torch.int32, device=dev)
    c_ret = torch.zeros(n, dtype=torch.float64, device=dev)
    c_final = torch.zeros((n, 22), dtype=torch.float64, device=dev)

    def composed_step():
        nonlocal c_len, c_ret, c_final
        obs, rew, done, info = env.step()
        c_len += 1
        c_ret += rew
        trunc = (c_len >= MAX) & (done == 0)
        reset = (done != 0) | trunc
        c_final = torch.where(reset[:, None], obs, c_final)     # final observation of the reset plants
        step_obs = obs.clone()
        new_obs = env.restore(reset)
        obs = torch.where(reset[:, None], new_obs, step_obs)
        c_len = torch.where(reset, torch.zeros_like(c_len), c_len)
        c_ret = torch.where(reset, torch.zeros_like(c_ret), c_ret)
        return obs, rew, done, trunc, c_final

    def prepare(name):
        if name == "off":
            set_autoreset(False)
        elif name == "on_idle":
            set_autoreset(True, 0)
        elif name == "on_1pct":
            stagger()
        elif name == "composed_1pct":
            set_autoreset(False)
            c_len.copy_(((lane % MAX) + 1) % MAX)
            c_ret.zero_()
        elif name == "on_all":
            set_autoreset(True, 1)

    def run_block(name, steps):
        return time_steps(stream, composed_step if name == "composed_1pct" else env.step, steps)

    setups = ["off", "on_idle", "on_1pct", "composed_1pct", "on_all"]
    # warm-up: >= 200 launches of every setup's kernels
    for name in setups:
        prepare(name)
        run_block(name, 200)
    # resets per step of the 1 % setups, measured once (outside the timed blocks)
    prepare("on_1pct")
    resets = []
    for _ in range(20):
        _, _, d, info = env.step()
        resets.append(int(((d != 0) | (info["truncated"] != 0)).sum().item()))
    times = {s: [] for s in setups}
    for r in range(a.rounds):      # (not the harness's rotation: on_all, a full arena copy per step, runs every second round only)
        for name in setups:
            if name == "on_all" and r % 2:
                continue
            prepare(name)
            times[name].append(run_block(name, a.block))

    S = {s: stats(v) for s, v in times.items()}
    off = S["off"]["median_us"]
    res = {"what": "per-step time of npb_step with and without same-step autoreset, one handle", "n_plants": n,
           "device": torch.cuda.get_device_name(dev), "storage": env.storage, "step_kernel": env.last_step_kernel(),
           "block_steps": a.block, "rounds": a.rounds, "max_episode_steps_1pct": MAX,
           "resets_per_step_1pct": {"mean": float(np.mean(resets)), "min": int(min(resets)), "max": int(max(resets))},
           "setups": S,
           "overhead_vs_off_pct": {s: 100.0 * (S[s]["median_us"] / off - 1.0) for s in setups if s != "off"},
           "head": head(ROOT)}
    write_line(res, a.out)
    env.close()


if __name__ == "__main__":
    main()
