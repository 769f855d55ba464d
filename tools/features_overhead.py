"""What features (npb_set_features: the caller's policy inputs as a frame stack kept on the device) cost on BASELINE config 4 at 65 536 and
32 768 plants.

action_test("oil_top_off", range(n), dt = 5) with autoreset from a bank of `--bank` scenarios, device noise and a constant setpoint: no
per-step host input.  The features are 16 columns -- 8 state members, 4 info columns, 2 obs columns (one against a second column), the
step's reward and the trip flags' pump bits -- each with a ref, a scale and a clip, K = 4 frames, float32: a [n, 4, 16] tensor.  One
handle per size throughout; the features are
set and dropped on it between blocks, in an order that rotates from round to round.  Setups, event-timed us per step:
  off        no features, no episode ending                                                                                   (a)
  on         features on, nothing restarting: pass A behind every step, and pass B finding nothing                            (b)
  busy       features on with `final`; max_episode_steps = 100 with the plants' episode clocks staggered beforehand by group
             p % 100: about 1 % of the plants are truncated and restart from the bank on every timed step                    (c)
  busy_off   the same episodes without features: what busy is to be held against
  torch      no features; the same frames formed the way a user forms them today on the same build -- npb_gather_fields for the
             members, the step's output tensors for the rest, torch ops for the transform, torch.roll for the stack -- WITHOUT any
             restart handling                                                                                                 (d)
Reported per setup: the per-step time of each block (median, quartiles, min..max over the blocks), and on minus off of the same round.
What the bytes say: pass A reads 17 values and two bookkeeping words per plant, reads 3 x 16 floats of the plant's stack and writes 4 x
16: some 600 B, 39 MB at 65 536 plants against the step's 451 MB.

--parent DIR: a checkout of the parent commit, built.  `off` is then also measured in fresh processes, alternately on this build and on
the parent's (this script run with --package-root and --only-off), `--process-repeats` times each, and held against each other by
overhead_harness.compare_off.  bench.py is run alternately from the two trees and its ms per step printed beside it.  One JSON line per
run, all sizes in one object, also written to --out.
"""
import argparse
import ctypes
import os
import sys

from overhead_harness import (add_parent_arguments, bench_alternated, compare_off, head, off_across_builds, paired, rotated_blocks, stats,
                              time_steps, write_line)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 8
EPISODE = 100
DT = 5.0
STACK = 4
MEMBERS = [("pump.oil_level", 0), ("pump.oil_level", 1), ("pump.vibration_level", 0), ("pump.motor_temperature", 0), ("sg.tube_wall_temp", 0),
           ("sg.water_level", 1), ("prim.fuel_temperature", 0), ("prim.coolant_temperature", 0)]
INFO = ["electrical_power", "steam_flow", "steam_pressure", "thermal_efficiency"]
PUMP_TRIPS = 0xF00


def columns():
    """the 16 columns as set_features takes them"""
    cols = [(m, {"ref": 50.0, "scale": 0.02, "clip": (-5.0, 5.0)}) for m in MEMBERS]
    cols += [(("info", name), {"ref": 100.0, "scale": 0.001, "clip": (-5.0, 5.0)}) for name in INFO]
    cols += [(("obs", 5), {"ref": ("obs", 6), "clip": (-5.0, 5.0)}), (("obs", 7), {"ref": 0.5, "scale": 2.0, "clip": (-5.0, 5.0)}),
             ("reward", {"scale": 0.1, "clip": (-5.0, 5.0), "nan_to": 0.0}), ("flags", {"bits": PUMP_TRIPS})]
    return cols


class TorchFrames:
    """(d): the same [n, 4, 16] float32 stack, formed per step with what the package offers without set_features"""

    def __init__(self, env):
        import torch
        from nuclear_sim_amd.env import INFO_COLUMNS
        from nuclear_sim_amd.schema import SCHEMA
        self.torch, self.env = torch, env
        ks = [SCHEMA.slot(m[0], m[1]) for m in MEMBERS]
        self.plan = ((ctypes.c_int * len(ks))(*[0 if kd == "f64" else 1 for kd, _ in ks]), (ctypes.c_int * len(ks))(*[sl for _, sl in ks]))
        self.members = torch.empty((len(ks), env.n), dtype=torch.float64, device=env.device)
        self.info_idx = torch.tensor([INFO_COLUMNS.index(name) for name in INFO], device=env.device)
        self.stack = torch.zeros((env.n, STACK, 16), dtype=torch.float32, device=env.device)

    def update(self, obs, reward, info):
        torch, env = self.torch, self.env
        env.L.npb_gather_fields(env._h, len(MEMBERS), self.plan[0], self.plan[1], ctypes.c_void_p(self.members.data_ptr()), env._stream())
        m = ((self.members - 50.0) * 0.02).clamp(-5.0, 5.0)
        i = ((env._info[:, self.info_idx] - 100.0) * 0.001).clamp(-5.0, 5.0)
        o = torch.stack([(obs[:, 5] - obs[:, 6]).clamp(-5.0, 5.0), ((obs[:, 7] - 0.5) * 2.0).clamp(-5.0, 5.0),
                         torch.nan_to_num(reward * 0.1, nan=0.0).clamp(-5.0, 5.0), ((info["trip_flags"] & PUMP_TRIPS) != 0).to(torch.float64)], dim=1)
        frame = torch.cat([m.t(), i, o], dim=1).to(torch.float32)
        self.stack = torch.roll(self.stack, -1, dims=1)
        self.stack[:, -1] = frame
        return self.stack


def measure(n, block, rounds, bank, only_off):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, autoreset=True, bank_seeds=list(range(1000, 1000 + bank)), noise_generator="device")
    has = hasattr(env, "set_features") and not only_off
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    sp = torch.full((n,), 90.0, dtype=torch.float64, device=dev)
    groups = ((torch.arange(n, device=dev) % EPISODE).view(1, n) == torch.arange(EPISODE, device=dev).view(-1, 1)).to(torch.uint8)
    setups = ["off"] + (["on", "torch", "busy", "busy_off"] if has else [])
    by_hand = TorchFrames(env) if has else None
    rates, agree = {}, {}

    def step(setup):
        out = env.step(power_setpoint=sp)
        if setup == "torch":
            by_hand.update(out[0], out[1], out[3])
        return out

    def run_block(setup):
        busy = setup in ("busy", "busy_off")
        env._enable_autoreset(EPISODE if busy else None)      # the episode limit of the setup; the counters begin at zero
        if has:
            env.set_features(columns() if setup in ("on", "busy") else None, stack=STACK, final=True)
        env.restore_from_bank()                               # every plant's clock back to 0
        if busy:
            for k in range(EPISODE):                          # stagger the episode clocks: group k ends at steps k + 100 j
                env.step(power_setpoint=sp)
                env.restore_from_bank(groups[k])
        for _ in range(W):
            step(setup)
        first = step(setup)
        before = first[3]["episode_index"].sum().item()
        us = time_steps(stream, lambda: step(setup), block)
        last = step(setup)
        rates[setup] = 100.0 * (last[3]["episode_index"].sum().item() - before) / (block + 1) / n
        return us

    if has:      # what (d) forms is what the device forms, where nothing restarts: the newest frame of both after a few steps
        env.set_features(columns(), stack=STACK, final=True)
        for _ in range(STACK + 1):
            out = env.step(power_setpoint=sp)
            mine = by_hand.update(out[0], out[1], out[3])
        agree = {"max_abs_difference_of_the_stacks": float((mine - env.features()).abs().max().item())}
        env.set_features(None)
    blocks = rotated_blocks(setups, rounds, run_block)
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": block, "rounds": rounds,
           "bank_entries": bank, "columns": 16, "stack": STACK, "dtype": "float32", "setups": {s: stats(v) for s, v in blocks.items()},
           "ended_percent_of_plants_per_step": dict(rates)}
    if has:
        out["by_hand_against_the_device"] = agree
        out["on_cost_us_per_step"] = paired(blocks, "on", "off")
        out["by_hand_in_torch_cost_us_per_step"] = paired(blocks, "torch", "off")
        out["one_percent_restarting_cost_us_per_step"] = paired(blocks, "busy", "busy_off")
        out["on_percent_of_the_step"] = 100.0 * out["on_cost_us_per_step"]["median"] / out["setups"]["off"]["median_us"]
        out["on_is_below_by_hand"] = bool(out["on_cost_us_per_step"]["median"] < out["by_hand_in_torch_cost_us_per_step"]["median"])
        env.set_features(None)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--block", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bank", type=int, default=64, help="entries of the start bank")
    ap.add_argument("--bench-steps", type=int, default=200)
    add_parent_arguments(ap, "features_overhead.json")
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
    out = {"what": "per-step time of config 4 with autoreset from a bank and device noise: features of 16 columns, 4 frames, float32 off, on with "
                   "nothing restarting, on with about 1 % of the plants truncated per step and their final stacks kept; the same frames formed "
                   "by hand in torch on the same build, without restart handling, beside it",
           "sizes": sizes, "head": head(ROOT)}
    if a.parent and not a.only_off:
        out["bench"] = bench_alternated(a.parent, a.process_repeats, a.bench_steps, 20)
    write_line(out, a.out)


if __name__ == "__main__":
    main()
