"""What the normaliser (npb_set_normalizer: running observation and reward normalisation folded on the device) costs on BASELINE config 4
at 65 536 and 32 768 plants.

action_test("oil_top_off", range(n), dt = 5) with autoreset from a bank of `--bank` scenarios (no episode limit: nothing restarts), device
noise and a constant setpoint: no per-step host input.  The features are tools/features_overhead.py's 16 columns, K = 4 frames, float32;
the normaliser takes the 14 of them that are eligible (the setpoint error and the BITS column are not).  One handle per size throughout;
the normaliser is set, frozen and dropped on it between blocks, in an order that rotates from round to round.  Setups, event-timed us per
step, each without and with (`_r`) the return stream (gamma 0.99, clip 5):
  off          the features alone: what every other setup is held against
  training     the normaliser on: the partials kernel, the finish kernel and, with the return stream, the reward kernel more
  frozen       normalizer_training(False): no fold launches; with the return stream the reward kernel still runs
  torch        the features alone, and the same update by hand in torch on the same build, the way a user writes it today:
               npb_gather_fields for the members and the step's output tensors for the rest (the raw columns), torch.var_mean over the
               plants, Chan's merge of (count, mean, M2) on the device, the broadcast (x - mean) * rsqrt(var + eps) with the clip into a
               float32 frame; with the return stream the discounted return, its merge, and the reward scaled and clipped.  It does not
               put the frame into the stack: the device's features keep doing that
Reported per setup: the per-step time of each block (median, quartiles, min..max over the blocks), and every setup minus off of the same
round.  What the bytes say: the partials kernel reads 14 values per plant, about 100 B, 7 MB at 65 536 plants against the step's 451 MB,
and writes 3 x 15 x 256 partials; its time is launch and barrier latency, not traffic.

--parent DIR: a checkout of the parent commit, built.  `off` is then also measured in fresh processes, alternately on this build and on
the parent's (this script run with --package-root and --only-off), `--process-repeats` times each, and held against each other by
overhead_harness.compare_off.  bench.py is run alternately from the two trees and its ms per step printed beside it.  One JSON line per
run, all sizes in one object, also written to --out (profiles/normalizer_overhead.json).

Built on tools/overhead_harness.py like the *_overhead.py scripts; it is not named as they are because tests/test_overhead_harness_cpu.py
pins their list.
"""
import argparse
import ctypes
import os
import sys

from features_overhead import DT, INFO, MEMBERS, STACK, W, columns
from overhead_harness import (add_parent_arguments, bench_alternated, compare_off, head, off_across_builds, paired, rotated_blocks, stats,
                              time_steps, write_line)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA, CLIP, EPS = 0.99, 5.0, 1e-8
ELIGIBLE = [j for j in range(16) if j not in (12, 15)]      # 12: a setpoint error; 15: BITS


class TorchNormalizer:
    """the same update by hand: raw columns gathered, batch moments, Chan's merge, the broadcast; and the return's with ``reward``"""

    def __init__(self, env, reward):
        import torch
        from nuclear_sim_amd.env import INFO_COLUMNS
        from nuclear_sim_amd.schema import SCHEMA
        self.torch, self.env, self.reward = torch, env, reward
        ks = [SCHEMA.slot(m[0], m[1]) for m in MEMBERS]
        self.plan = ((ctypes.c_int * len(ks))(*[0 if kd == "f64" else 1 for kd, _ in ks]), (ctypes.c_int * len(ks))(*[sl for _, sl in ks]))
        self.members = torch.empty((len(ks), env.n), dtype=torch.float64, device=env.device)
        self.info_idx = torch.tensor([INFO_COLUMNS.index(name) for name in INFO], device=env.device)
        z = dict(dtype=torch.float64, device=env.device)
        self.count, self.mean, self.M2 = torch.zeros((), **z), torch.zeros(14, **z), torch.zeros(14, **z)
        self.rcount, self.rmean, self.rM2, self.ret = torch.zeros((), **z), torch.zeros((), **z), torch.zeros((), **z), torch.zeros(env.n, **z)

    def merge(self, count, mean, M2, x, dim):
        torch = self.torch
        var, batch = torch.var_mean(x, dim=dim, unbiased=False)
        nb = float(x.shape[dim])
        total = count + nb
        delta = batch - mean
        return total, mean + delta * (nb / total), M2 + var * nb + delta * delta * (count * nb / total)

    def update(self, obs, reward, done):
        torch, env = self.torch, self.env
        env.L.npb_gather_fields(env._h, len(MEMBERS), self.plan[0], self.plan[1], ctypes.c_void_p(self.members.data_ptr()), env._stream())
        raw = torch.cat([self.members.t(), env._info[:, self.info_idx], obs[:, 7:8], reward.view(-1, 1)], dim=1)      # [n, 14]
        self.count, self.mean, self.M2 = self.merge(self.count, self.mean, self.M2, raw, 0)
        frame = ((raw - self.mean) * torch.rsqrt(self.M2 / self.count + EPS)).clamp(-CLIP, CLIP).to(torch.float32)
        scaled = None
        if self.reward:
            self.ret = torch.where(done != 0, torch.zeros_like(self.ret), self.ret * GAMMA) + reward
            self.rcount, self.rmean, self.rM2 = self.merge(self.rcount, self.rmean, self.rM2, self.ret, 0)
            scaled = (reward * torch.rsqrt(self.rM2 / self.rcount + EPS)).clamp(-CLIP, CLIP)
        return frame, scaled


def measure(n, block, rounds, bank, only_off):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, autoreset=True, bank_seeds=list(range(1000, 1000 + bank)), noise_generator="device")
    has = hasattr(env, "set_normalizer") and not only_off
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    sp = torch.full((n,), 90.0, dtype=torch.float64, device=dev)
    env.set_features(columns(), stack=STACK, final=True)
    setups = ["off"] + ([s + r for r in ("", "_r") for s in ("training", "frozen", "torch")] if has else [])
    by_hand = {}

    def step(setup):
        out = env.step(power_setpoint=sp)
        if setup.startswith("torch"):
            by_hand[setup].update(out[0], out[1], out[2])
        return out

    def run_block(setup):
        if has:
            env.set_normalizer(None)
            if setup.startswith(("training", "frozen")):
                env.set_normalizer(ELIGIBLE, reward={"gamma": GAMMA, "clip": CLIP} if setup.endswith("_r") else None, eps=EPS)
            if setup.startswith("torch"):
                by_hand[setup] = TorchNormalizer(env, setup.endswith("_r"))
        for _ in range(W):      # (a frozen normaliser has statistics to be frozen with)
            step(setup)
        if setup.startswith("frozen"):
            env.normalizer_training(False)
        step(setup)
        return time_steps(stream, lambda: step(setup), block)

    blocks = rotated_blocks(setups, rounds, run_block)
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": block, "rounds": rounds,
           "bank_entries": bank, "columns": 16, "normalised_columns": len(ELIGIBLE), "stack": STACK, "dtype": "float32",
           "setups": {s: stats(v) for s, v in blocks.items()}}
    if has:
        out["cost_us_per_step"] = {s: paired(blocks, s, "off") for s in setups[1:]}
        out["training_percent_of_the_step"] = 100.0 * out["cost_us_per_step"]["training"]["median"] / out["setups"]["off"]["median_us"]
        out["device_is_below_by_hand"] = {"columns": bool(out["cost_us_per_step"]["training"]["median"] < out["cost_us_per_step"]["torch"]["median"]),
                                          "columns_and_return": bool(out["cost_us_per_step"]["training_r"]["median"] < out["cost_us_per_step"]["torch_r"]["median"])}
        env.set_normalizer(None)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--block", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bank", type=int, default=64, help="entries of the start bank")
    ap.add_argument("--bench-steps", type=int, default=200)
    add_parent_arguments(ap, "normalizer_overhead.json")
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    sizes = {}
    for n in a.n:
        res = measure(n, a.block, a.rounds, a.bank, a.only_off)
        print("%d plants: measured" % n, file=sys.stderr, flush=True)
        if a.parent and not a.only_off:
            this, parent = off_across_builds(__file__, ["--n", n, "--block", a.block, "--rounds", a.rounds, "--bank", a.bank], a.parent, a.process_repeats,
                                             lambda run: run["sizes"][str(n)]["setups"]["off"]["median_us"], 900)
            res["parent_comparison"] = {"off": compare_off(this, parent, res["setups"]["off"])}
        sizes[str(n)] = res
    out = {"what": "per-step time of config 4 with autoreset from a bank and device noise, features of 16 columns, 4 frames, float32: alone "
                   "(off), with the normaliser on 14 of the columns training and frozen, without and with (_r) the return stream, and with "
                   "the same update written by hand in torch on the same build beside the features",
           "sizes": sizes, "head": head(ROOT)}
    if a.parent and not a.only_off:
        out["bench"] = bench_alternated(a.parent, a.process_repeats, a.bench_steps, 20)
    write_line(out, a.out)


if __name__ == "__main__":
    main()
