"""What controls (npb_set_controls: the caller's policy outputs decoded on the device in front of the step) cost on BASELINE config 4 at
65 536 and 32 768 plants.

action_test("oil_top_off", range(n), dt = 5) with device noise: no per-step host input.  The controls are four axes, float32 input: a rod
RATE, a valve TARGET (offset 50, max_magnitude 0.05), a flow RATE and a power-setpoint COLUMN (offset 90, clip 80 .. 100), with hold
intervals 1 and 4.  The policy's output is one fixed [n, 4] tensor of small values (rates of +-0.02, targets and setpoints within +-0.5 of
the offset) whose sign is flipped in place before every step -- in EVERY setup, so that launch is in none of the differences -- so the
actuators move on every plant and every step, store included, and stay where the plants run as they do without controls.  One handle per
size throughout; the controls are set and dropped on it between blocks, in an order that rotates from round to round.  Setups, event-timed
us per step:
  off        no controls; the caller's constant setpoint column                                                                (a)
  on         controls on, interval 1: the decode kernel in front of every step                                                 (b)
  on4        the same with interval 4: three steps of four apply the held values without reading the input                     (c)
  torch      no controls; the same decode the way a user does it today on the same build -- the cast, the clips, the sign split
             into an up and a down move with the range limits, the target's bounded move, one npb_get_field and one npb_set_field
             per actuator (three of each) and the setpoint column -- WITHOUT a hold and without restart handling              (d)
Reported per setup: the per-step time of each block (median, quartiles, min..max over the blocks), and each setup minus off of the same
round.  What the bytes say: the kernel reads 16 B of input and three bookkeeping words per plant, reads and writes held and prev (2 x 4 x
8 B), reads three members and writes back those that moved, writes one column: some 150 B, 10 MB at 65 536 plants against the step's 451 MB.

--parent DIR: a checkout of the parent commit, built.  `off` is then also measured in fresh processes, alternately on this build and on
the parent's (this script run with --package-root and --only-off), `--process-repeats` times each, and held against each other by
overhead_harness.compare_off.  bench.py is run alternately from the two trees and its ms per step printed beside it.  One JSON line per
run, all sizes in one object, also written to --out.
"""
import argparse
import os
import sys

from overhead_harness import (add_parent_arguments, bench_alternated, compare_off, head, off_across_builds, paired, rotated_blocks, stats,
                              time_steps, write_line)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 8
DT = 5.0
MAX_MAGNITUDE = 0.05
AXES = [("rod", "rate"), ("valve", "target", {"offset": 50.0, "max_magnitude": MAX_MAGNITUDE}), ("flow", "rate"),
        ("power_setpoint", "column", {"offset": 90.0, "clip": (80.0, 100.0)})]


class TorchDecode:
    """(d): the same decode with what the package offers without set_controls"""

    def __init__(self, env):
        import torch
        self.torch, self.env = torch, env
        P = env.params
        self.rod, self.flow, self.valve = (float(v) * float(P.dt) for v in (P.max_control_rod_speed, P.max_flow_change_rate, P.max_valve_speed))

    def rate(self, name, y, per_unit, lo, hi):
        torch, env = self.torch, self.env
        pos = env.get_field(name)
        up, down = (pos + per_unit * y).clamp(max=hi), (pos - per_unit * (-y)).clamp(min=lo)
        env.set_field(name, torch.where(y > 0, up, torch.where(y < 0, down, pos)))

    def setpoint(self, x):
        """the three actuators moved through get_field / set_field; returns the setpoint column for step()"""
        torch, env = self.torch, self.env
        x = x.to(torch.float64)
        self.rate("prim.control_rod_position", x[:, 0].clamp(-1.0, 1.0), self.rod, 0.0, 100.0)
        self.rate("prim.coolant_flow_rate", x[:, 2].clamp(-1.0, 1.0), self.flow, 5000.0, 50000.0)
        y, pos = x[:, 1] + 50.0, env.get_field("prim.steam_valve_position")
        up, down = (pos + self.valve * MAX_MAGNITUDE).clamp(max=100.0), (pos - self.valve * MAX_MAGNITUDE).clamp(min=0.0)
        env.set_field("prim.steam_valve_position", torch.where(y > pos, torch.minimum(up, y), torch.where(y < pos, torch.maximum(down, y), pos)))
        return (x[:, 3] + 90.0).clamp(80.0, 100.0)


def measure(n, block, rounds, only_off):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, noise_generator="device")
    has = hasattr(env, "set_controls") and not only_off
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    sp = torch.full((n,), 90.0, dtype=torch.float64, device=dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    scale = torch.tensor([0.02, 0.5, 0.02, 0.5])
    policy = ((torch.rand((n, 4), generator=g) * 2.0 - 1.0) * scale).to(device=dev, dtype=torch.float32)
    setups = ["off"] + (["on", "on4", "torch"] if has else [])
    by_hand = TorchDecode(env) if has else None
    state = {"x": policy}

    def step(setup):
        state["x"].neg_()      # the policy's new output, in every setup
        if setup in ("on", "on4"):
            return env.step()
        if setup == "torch":
            return env.step(power_setpoint=by_hand.setpoint(state["x"]))
        return env.step(power_setpoint=sp)

    def run_block(setup):
        if has:
            env.set_controls(AXES if setup in ("on", "on4") else None, interval=4 if setup == "on4" else 1)
            if setup in ("on", "on4"):
                env.controls_input().copy_(policy)
                state["x"] = env.controls_input()      # the policy writes into the bound tensor
            else:
                state["x"] = policy
        for _ in range(W):
            step(setup)
        return time_steps(stream, lambda: step(setup), block)

    agree = {}
    if has:      # what (d) decodes is what the device decodes: the three members and the setpoint column after one step of each
        twin = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, noise_generator="device")
        env.set_controls(AXES)
        env.controls_input().copy_(policy)
        env.step()
        twin.step(power_setpoint=TorchDecode(twin).setpoint(policy))
        agree = {"max_abs_difference_of_" + name.split(".")[1]: float((env.get_field(name) - twin.get_field(name)).abs().max().item())
                 for name in ("prim.control_rod_position", "prim.coolant_flow_rate", "prim.steam_valve_position", "prim.power_level")}
        twin.close()
        env.set_controls(None)
    blocks = rotated_blocks(setups, rounds, run_block)
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": block, "rounds": rounds,
           "axes": 4, "dtype": "float32", "setups": {s: stats(v) for s, v in blocks.items()}}
    if has:
        out["by_hand_against_the_device"] = agree
        out["on_cost_us_per_step"] = paired(blocks, "on", "off")
        out["on_interval_4_cost_us_per_step"] = paired(blocks, "on4", "off")
        out["by_hand_in_torch_cost_us_per_step"] = paired(blocks, "torch", "off")
        out["on_percent_of_the_step"] = 100.0 * out["on_cost_us_per_step"]["median"] / out["setups"]["off"]["median_us"]
        out["on_is_below_by_hand"] = bool(out["on_cost_us_per_step"]["median"] < out["by_hand_in_torch_cost_us_per_step"]["median"])
        env.set_controls(None)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--block", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bench-steps", type=int, default=200)
    add_parent_arguments(ap, "controls_overhead.json")
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    sizes = {}
    for n in a.n:
        res = measure(n, a.block, a.rounds, a.only_off)
        print("%d plants: measured" % n, file=sys.stderr, flush=True)
        if a.parent and not a.only_off:
            this, parent = off_across_builds(__file__, ["--n", n, "--block", a.block, "--rounds", a.rounds], a.parent, a.process_repeats,
                                             lambda run: run["sizes"][str(n)]["setups"]["off"]["median_us"], 900)
            res["parent_comparison"] = {"off": compare_off(this, parent, res["setups"]["off"])}
        sizes[str(n)] = res
    out = {"what": "per-step time of config 4 with device noise: controls of four axes (rod RATE, valve TARGET, flow RATE, power-setpoint COLUMN), "
                   "float32 input, off, on with interval 1 and with interval 4; the same decode done by hand in torch on the same build, "
                   "without a hold and without restart handling, beside it",
           "sizes": sizes, "head": head(ROOT)}
    if a.parent and not a.only_off:
        out["bench"] = bench_alternated(a.parent, a.process_repeats, a.bench_steps, 20)
    write_line(out, a.out)


if __name__ == "__main__":
    main()
