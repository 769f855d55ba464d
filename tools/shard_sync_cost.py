"""What one normaliser and one set of advantage moments across shards cost on one device (npb_normalizer_shard_delta,
npb_normalizer_apply_shards, npb_rollout_moments_part, npb_rollout_moments_combine).

Setups, event-timed us per call, a block being `--calls` calls in a row, the order rotating from round to round:
  sync_w1 / 2 / 8 / 64   env.normalizer_sync at S = 17 (tools/policy_cost.py's 16 columns and the return stream) through an exchange on
                         the device that copies this shard's vector into row 0 of a [W, 3 S] buffer whose other rows are empty deltas:
                         the delta launch, the copy, the combine launch and the finish launch.  After a block's first call the shard has
                         folded nothing new and its own delta is empty too: the launches and the loop over W are what is timed
  moments                env.rollout_moments over a float32 [128, 65 536] tensor: the four launches of npb_rollout_moments
  moments_shards_w1      env.rollout_moments_shards over the same tensor through an identity exchange: the same two column passes, a
                         part finish and a combine launch behind each: six launches in place of four, and the host's side of
                         two exchanges between them.  Both and the blocks' spread are recorded, no ratio is asserted
exchange_bytes_per_shard (24 S, and 16 twice) is stated, not measured: no all-gather across devices is timed.
With --parent DIR (a built checkout of the parent commit): `moments`, which the parent's library has too, in fresh processes alternately
on this build and on the parent's, held against each other by overhead_harness.compare_off; and with --bench-steps bench.py alternately
from the two trees.  --resources FILE: the remarks of a -Rpass-analysis=kernel-resource-usage build of npb_minibatch.hip.
One JSON line, also written to --out (profiles/shard_sync_cost.json).

Built on tools/overhead_harness.py like the *_overhead.py scripts; it is not named as they are because tests/test_overhead_harness_cpu.py
pins their list.
"""
import argparse
import os
import sys

from overhead_harness import add_parent_arguments, bench_alternated, compare_off, head, off_across_builds, rotated_blocks, stats, time_steps, write_line
from policy_cost import DT, columns, resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 2, 8, 64)
ROWS, COLS = 128, 65536


def measure(n, calls, rounds, only_off):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT)
    env.set_features(columns(), stack=1)
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    x = torch.randn((ROWS, COLS), generator=torch.Generator(device="cpu").manual_seed(0)).to(dev)
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "rounds": rounds, "calls_per_block": calls, "moments_tensor": [ROWS, COLS, "float32"]}
    steps = {"moments": lambda: env.rollout_moments(x)}
    if not only_off and hasattr(env, "normalizer_sync"):
        env.set_normalizer("all", reward={"gamma": 0.99, "clip": 5.0})
        S = env._norm_streams()
        for _ in range(4):
            env.step()
        buffers = {W: torch.zeros((W, 3 * S), dtype=torch.float64, device=dev) for W in WIDTHS}

        def exchange(W):
            def gather(vec):
                buffers[W][0].copy_(vec)
                return buffers[W]
            return gather
        for W in WIDTHS:
            steps["sync_w%d" % W] = lambda g=exchange(W): env.normalizer_sync(g)
        steps["moments_shards_w1"] = lambda: env.rollout_moments_shards(lambda vec: vec[None], x)
        out.update({"streams": S, "exchange_bytes_per_shard": {"normalizer": 24 * S, "moments": [16, 16]}})

    def run_block(setup):
        for _ in range(3):
            steps[setup]()
        return time_steps(stream, steps[setup], calls)
    blocks = rotated_blocks(list(steps), rounds, run_block)
    out.update({"setups": {s: stats(v) for s, v in blocks.items()}, "moments_off": stats(blocks["moments"]),
                "moments_spread_us": max(blocks["moments"]) - min(blocks["moments"])})
    if "moments_shards_w1" in blocks:
        out["moments_shards_w1_spread_us"] = max(blocks["moments_shards_w1"]) - min(blocks["moments_shards_w1"])
        out["last_moments"] = {"moments": env.rollout_moments(x).cpu().tolist(), "moments_shards_w1": env.rollout_moments_shards(lambda vec: vec[None], x).cpu().tolist()}
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096, help="plants of the env whose normaliser is synchronised")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bench-steps", type=int, default=0, help="with --parent: bench.py --steps K alternately from the two trees (0 = not run)")
    ap.add_argument("--resources", default=None, help="the output of a -Rpass-analysis=kernel-resource-usage build of npb_minibatch.hip")
    add_parent_arguments(ap, "shard_sync_cost.json")
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    res = measure(a.n, a.calls, a.rounds, a.only_off)
    if a.parent and not a.only_off:
        argv = ["--n", a.n, "--calls", a.calls, "--rounds", a.rounds]
        this, parent = off_across_builds(__file__, argv, a.parent, a.process_repeats, lambda run: run["result"]["moments_off"]["median_us"], 900)
        res["parent_comparison"] = {"moments_off": compare_off(this, parent, res["moments_off"])}
        if a.bench_steps:
            res["bench"] = bench_alternated(a.parent, a.process_repeats, a.bench_steps, 20)
    out = {"what": "normalizer_sync at S = 17 through a device-side exchange at W = 1, 2, 8 and 64; the four moments calls at W = 1 against "
                   "rollout_moments over a float32 [128, 65 536] tensor on the same build; event-timed us per call.  exchange_bytes_per_shard is "
                   "stated, not measured; no all-gather across devices is timed",
           "result": res, "head": head(ROOT)}
    if a.resources:
        out["kernel_resources"] = resources(a.resources)
    write_line(out, a.out)


if __name__ == "__main__":
    main()
