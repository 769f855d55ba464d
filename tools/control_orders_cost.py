"""What order rules on the controls' axes (npb_set_control_orders: a policy output on a VALUE axis orders maintenance on the device) cost on
BASELINE config 4 at 65 536 and 32 768 plants.

action_test("oil_top_off", range(n), dt = 5) with device noise: no per-step host input.  The controls are three axes, float32 input -- a
rod RATE whose input is 0.0 (nothing moves) and two VALUE axes -- set in EVERY setup, so their decode is in none of the differences.  The
rules are four, threshold 0.0, min_interval 1: a pump's oil top-off and a generator's TSP cleaning on the first VALUE axis, the condenser's
tube cleaning and a stage's overhaul on the second.  The policy's output is a fixed [n, 3] tensor per firing pattern; no maintenance log
is set.  One handle per size throughout; the rules are set and dropped on it between blocks, in an order that rotates from round to
round.  Setups, event-timed us per step:
  off            controls, no rules                                                                                            (a)
  quiet          rules on, every plant below the thresholds: the first pass alone, no wave reaches the arena                   (b)
  one_pct        rules on, 1 % of the plants above them on every step, one to a wave                                           (c)
  all            rules on, every plant above them on every step                                                                (d)
  empty_ops      no rules; the three perform_* calls with nothing ordered (action -1 everywhere) in front of every step: what the
                 quiet cost is held against                                                                                    (e)
  hand_quiet     no rules; the same orders by hand on the same build: the controls' held values thresholded in torch into int32 action
                 columns and one perform_* call per rule (four calls of the three entry points, device columns), the quiet pattern   (f)
  hand_one_pct   the same with the 1 % pattern -- without min_interval, restart handling or a fired column                      (g)
Reported per setup: the per-step time of each block (median, quartiles, min..max over the blocks), and each setup minus off of the same
round.  Two comparisons are the criterion: the quiet cost against the empty operator launches of the same run, and `off` against the
parent's build.

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
AXES = [("rod", "rate"), (None, "value"), (None, "value")]
RULES = [(1, "pump", "oil_top_off", {"unit": 1}), (1, "steam_generator", "tsp_chemical_cleaning", {"unit": 2}),
         (2, "condenser", "condenser_tube_cleaning"), (2, "stage", "overhaul", {"unit": 7})]
SETUPS = ("off", "quiet", "one_pct", "all", "empty_ops", "hand_quiet", "hand_one_pct")


class ByHand:
    """(f), (g): the rules with what the package offers without set_control_orders"""

    def __init__(self, env):
        import torch
        from nuclear_sim_amd import _lib
        self.torch, self.env = torch, env
        n, dev = env.n, env.device
        self.rules = _lib.control_orders_request(RULES)
        self.none = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.action = [torch.full((n,), R["action"], dtype=torch.int32, device=dev) for R in self.rules]
        self.unit = [torch.full((n,), R["unit"], dtype=torch.int32, device=dev) for R in self.rules]
        self.component = [o[1] for o in RULES]

    def order(self, held):
        torch, env = self.torch, self.env
        for R, action, unit, component in zip(self.rules, self.action, self.unit, self.component):
            column = torch.where(held[R["axis"]] > R["threshold"], action, self.none)
            if R["family"] == "pump":
                env.perform_maintenance(column, unit)
            elif R["family"] == "component":
                env.perform_component_maintenance(component, column, unit)
            else:
                env.perform_turbine_maintenance(component, column, unit)

    def empty(self):
        env = self.env
        env.perform_maintenance(self.none, self.unit[0])
        env.perform_component_maintenance(self.component[1], self.none, self.unit[1])
        env.perform_turbine_maintenance(self.component[3], self.none, self.unit[3])


def measure(n, block, rounds, only_off):
    import torch
    from nuclear_sim_amd.env import BatchedPlantEnv
    env = BatchedPlantEnv.action_test("oil_top_off", range(n), dt=DT, noise_generator="device")
    has = hasattr(env, "set_control_orders") and not only_off
    dev = env.device
    stream = torch.cuda.current_stream(dev)
    env.set_controls(AXES)
    x = {"quiet": torch.zeros((n, 3), dtype=torch.float32, device=dev)}
    x["quiet"][:, 1:] = -1.0
    x["all"] = x["quiet"].clone()
    x["all"][:, 1:] = 1.0
    x["one_pct"] = x["quiet"].clone()
    waves = (n + 63) // 64
    first = torch.arange(0, min(waves, max(1, n // 100)), device=dev) * 64      # one plant in each of the first n / 100 waves
    x["one_pct"][first + 17, 1:] = 1.0
    pattern = {"off": "quiet", "quiet": "quiet", "one_pct": "one_pct", "all": "all", "empty_ops": "quiet", "hand_quiet": "quiet", "hand_one_pct": "one_pct"}
    setups = ["off"] + (list(SETUPS[1:]) if has else [])
    by_hand = ByHand(env) if has else None

    def step(setup):
        if setup == "empty_ops":
            by_hand.empty()
        elif setup.startswith("hand_"):
            # the held values the step's decode is about to form: value axes are the input itself (scale 1, offset 0, no clip)
            by_hand.order(env.controls_input().to(torch.float64).t())
        return env.step()

    def run_block(setup):
        if has:
            env.set_control_orders(RULES if setup in ("quiet", "one_pct", "all") else None)
        env.controls_input().copy_(x[pattern[setup]])
        for _ in range(W):
            step(setup)
        return time_steps(stream, lambda: step(setup), block)

    fired = {}
    if has:      # the patterns fire what they say
        env.set_control_orders(RULES)
        for name in ("quiet", "one_pct", "all"):
            env.controls_input().copy_(x[name])
            env.step()
            fired[name] = int(env.control_orders()["fired"][0].sum().item())
        env.set_control_orders(None)
    blocks = rotated_blocks(setups, rounds, run_block)
    out = {"n_plants": n, "device": torch.cuda.get_device_name(dev), "step_kernel": env.last_step_kernel(), "block_steps": block, "rounds": rounds,
           "rules": 4, "setups": {s: stats(v) for s, v in blocks.items()}}
    if has:
        out["plants_firing_per_step"] = fired
        for s in setups[1:]:
            out[s + "_cost_us_per_step"] = paired(blocks, s, "off")
        quiet, empty = out["quiet_cost_us_per_step"]["median"], out["empty_ops_cost_us_per_step"]["median"]
        out["quiet_percent_of_the_step"] = 100.0 * quiet / out["setups"]["off"]["median_us"]
        out["quiet_is_below_the_three_empty_operator_launches"] = bool(quiet < empty)
        out["quiet_is_below_by_hand"] = bool(quiet < out["hand_quiet_cost_us_per_step"]["median"])
        out["one_pct_is_below_by_hand"] = bool(out["one_pct_cost_us_per_step"]["median"] < out["hand_one_pct_cost_us_per_step"]["median"])
        env.set_control_orders(None)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 32768])
    ap.add_argument("--block", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bench-steps", type=int, default=200)
    add_parent_arguments(ap, "control_orders_overhead.json")
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
    out = {"what": "per-step time of config 4 with device noise and controls of three axes (a rod RATE at rest, two VALUE axes): four order rules "
                   "(pump oil top-off, generator TSP cleaning, condenser tube cleaning, stage overhaul; threshold 0, min_interval 1) off, on with "
                   "nothing firing, with 1 % of the plants firing one to a wave and with every plant firing; the three perform_* calls with "
                   "nothing ordered, and the same orders by hand in torch plus one perform_* call per rule, beside it",
           "sizes": sizes, "head": head(ROOT)}
    if a.parent and not a.only_off:
        out["bench"] = bench_alternated(a.parent, a.process_repeats, a.bench_steps, 20)
    write_line(out, a.out)


if __name__ == "__main__":
    main()
