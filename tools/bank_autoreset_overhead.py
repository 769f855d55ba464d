"""What the autoreset costs when it restarts plants from a start bank (npb_set_start_bank: the episode kernel behind every
npb_step, restoring from the bank) against the snapshot autoreset, at 65 536 plants.

One handle throughout, as in tools/autoreset_overhead.py -- where an arena lands in physical memory moves the step time from one
handle to the next (npb_api.hip, probe_placement).  The bank is a second batch of --bank plants, copied in before each bank block.  After >= 200
warm-up launches, blocks of `--block` event-timed steps alternate between the setups:
  snap_idle   snapshot autoreset, no plant terminates or reaches a limit
  bank_idle   bank autoreset, no plant terminates or reaches a limit
  snap_1pct   snapshot autoreset, max_episode_steps = 100 with the counters staggered (early restore(mask_k)): ~1 % reset per step
  bank_1pct   bank autoreset, the same resets, each into a random entry of the bank (advance 0, slots redrawn once per block)
  bank_all    bank autoreset, max_episode_steps = 1: every plant resets on every step
Prints one JSON line (per-step time in us: median, quartiles, min, max over the blocks) and writes it to --out.
The episode kernels' own time: run this under `rocprofv3 --kernel-trace --stats -- python tools/bank_autoreset_overhead.py --rounds 2`.
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
    ap.add_argument("--bank", type=int, default=65536, help="bank entries M")
    ap.add_argument("--block", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bank_autoreset_overhead.json"))
    a = ap.parse_args()
    n, M = a.n, a.bank
    env = BatchedPlantEnv(n, autoreset=True)
    bank = BatchedPlantEnv(M)         # construction states with one pump's oil level drawn per entry
    bank.set_field("pump.oil_level", np.random.default_rng(1).uniform(91.0, 99.0, M), instance=1)
    L, h = env.L, env._h
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    lane = torch.arange(n, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)

    def set_autoreset(on, max_steps=0):
        _lib.check(L.npb_set_autoreset(h, int(on), int(max_steps)), h)

    def random_slots():
        return torch.randint(0, M, (n,), device=dev, generator=gen, dtype=torch.int32)

    def stagger(restore):
        """limit MAX with plant p's counter at (k - p) mod MAX: ~1 % of the plants reach the limit on each step"""
        set_autoreset(True, MAX)
        for k in range(MAX):
            env.step()
            restore(lane % MAX == k)

    def prepare(name):
        set_autoreset(False)
        if name.startswith("snap"):
            env.set_start_bank(None)
        else:               # the bank copied in again (outside the timed blocks), random entries for every plant
            env.set_start_bank(bank, slots=random_slots(), advance=0)
        if name.endswith("idle"):
            set_autoreset(True, 0)
        elif name.endswith("1pct"):
            stagger(env.restore if name.startswith("snap") else env.restore_from_bank)
            if name.startswith("bank"):
                env.next_start_slots.copy_(random_slots())
        elif name.endswith("all"):
            set_autoreset(True, 1)

    def run_block(steps):
        return time_steps(stream, env.step, steps)

    setups = ["snap_idle", "bank_idle", "snap_1pct", "bank_1pct", "bank_all"]
    for name in setups:      # warm-up: >= 200 launches of every setup's kernels
        prepare(name)
        run_block(200)
    resets = {}
    for name in ("snap_1pct", "bank_1pct"):     # resets per step of the 1 % setups, measured once (outside the timed blocks)
        prepare(name)
        r = []
        for _ in range(20):
            _, _, d, info = env.step()
            r.append(int(((d != 0) | (info["truncated"] != 0)).sum().item()))
        resets[name] = {"mean": float(np.mean(r)), "min": int(min(r)), "max": int(max(r))}
    times = {s: [] for s in setups}
    for r in range(a.rounds):      # (not the harness's rotation: bank_all, a full arena copy per step, runs every second round only)
        for name in setups:
            if name == "bank_all" and r % 2:
                continue
            prepare(name)
            times[name].append(run_block(a.block))

    S = {s: stats(v) for s, v in times.items()}
    res = {"what": "per-step time of npb_step with the autoreset restoring from a start bank vs from the snapshot, one handle",
           "n_plants": n, "bank_entries": M, "device": torch.cuda.get_device_name(dev), "storage": env.storage,
           "step_kernel": env.last_step_kernel(), "block_steps": a.block, "rounds": a.rounds, "max_episode_steps_1pct": MAX,
           "resets_per_step": resets, "setups": S,
           "bank_vs_snapshot_pct": {"idle": 100.0 * (S["bank_idle"]["median_us"] / S["snap_idle"]["median_us"] - 1.0),
                                    "1pct": 100.0 * (S["bank_1pct"]["median_us"] / S["snap_1pct"]["median_us"] - 1.0)},
           "head": head(ROOT)}
    write_line(res, a.out)
    bank.close()
    env.close()


if __name__ == "__main__":
    main()
